// Device code of iwae_refine (gfx950): everything of a per-image variational
// refinement between the gradient passes (RefineArgs in iwae_kernels.h).  The
// parameters, Adam moments and gradients-of-parameters are [N][d_i] per layer;
// a sample row is (image b, sample s): its latents, noise and latent gradients
// are sample-major rows ((s N + b) d_i), its scalars image-major [N][k].
//
// Mapping.  One workgroup of 1024 threads (16 waves) owns one image in every
// launch, so nothing an image needs ever crosses a workgroup: no atomics, no
// tickets, and the order of every sum is a function of (k, d_i) alone, whatever
// the grid and the chunking of the gradient passes.  The launches are bound by
// the latency of their dependent loads, not by traffic (150 KB per image at
// k = 50, D = 150), so an image gets the largest workgroup and the loops over
// a lane's loads are unrolled to have several in flight.  The phases of an
// update, each closed by a barrier:
//   1. log q* of the k samples.  A group of lanes (16 while every d_i <= 64,
//      else the whole wave) owns a sample at a time, samples grp, grp + 1024 / G,
//      ...: a lane sums its columns in layer, then column order, the group
//      folds by an xor butterfly (__shfl_xor), lane 0 writes log w_s into the
//      image's k floats of the workspace (k up to 2^20 does not fit the LDS).
//   2. max_s and sum_s log w, then sum_s exp and sum_s exp^2: thread t takes
//      samples t, t + 1024, ... in order, a wave folds its 64 partials by an
//      xor butterfly, the 16 wave partials combine in one fixed binary tree;
//      the IWAE weights a_s replace log w_s in the workspace.
//   3. the gradients, 256 columns of a layer per round (a wave reads runs of 64
//      contiguous floats of a sample's row): wave w sums samples w, w + 16, ...
//      in order, a column's 16 partials combine in the same fixed tree, and
//      thread t < 256 applies Adam and the clamp to the round's column t (its
//      parameters and moments were fetched beside the sums' loads).
//   4. the next pass's draw: thread t takes (sample, column quad) pairs t, t +
//      1024, ... of each layer; float4 stores where d_i % 4 == 0.
// The noise of a pass is kept in the workspace next to the latents (phases 1
// and 3 read it again): an injected buffer and a Philox draw then look alike,
// and Philox is not run three times per element.
// Large k: the samples of an image stay with its workgroup (strided as above);
// they are not split over workgroups.
#include <algorithm>
#include <cmath>

#include "iwae_kernels.h"

namespace iwae {

namespace {

constexpr float kHalfLog2Pi = 0.918938533204672742f;
constexpr int kThreads = 1024, kWaves = kThreads / 64;   // one workgroup per image
constexpr int kCols = 256;                                // columns per round of the gradient sums

template <int G>
__device__ __forceinline__ float rf_group_sum(float v) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

// log w_s = log p(h_s) + log p(x|h_1s) - log q*_s of image b's samples into a.lw (or out, when given)
template <int G>
__device__ __forceinline__ void rf_log_weights(const RefineArgs& a, int b, float* out) {
  const int sub = threadIdx.x & (G - 1), grp = threadIdx.x / G;
  for (int s = grp; s < a.k; s += kThreads / G) {
    const size_t row = (size_t)s * a.N + b;
    const size_t c = (size_t)b * a.k + s;
    const float lp = a.lph[c] + a.lpx[c];           // (fetched beside the noise)
    float v = 0.f;
    for (int i = 0; i < a.L; ++i) {
      const int d = a.d[i];
      const float* e = a.epsw[i] + row * d;
      const float* ls = a.logstd[i] + (size_t)b * d;
#pragma unroll 4
      for (int j = sub; j < d; j += G) {
        const float ev = e[j];
        v += __builtin_fmaf(-0.5f * ev, ev, -ls[j]);
      }
    }
    v = rf_group_sum<G>(v);
    if (sub == 0) out[c] = lp - (v - kHalfLog2Pi * (float)a.D);
  }
}

// The wave's 64 values folded by an xor butterfly (every lane ends with the same bits), lane 0's into sh[wave];
// after the barrier every thread combines the kWaves partials in one fixed tree.
__device__ __forceinline__ float rf_tree(const float* p, int stride, bool take_max) {
  float t[kWaves];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t[w] = p[w * stride];
#pragma unroll
  for (int n = kWaves >> 1; n > 0; n >>= 1)
#pragma unroll
    for (int w = 0; w < n; ++w) t[w] = take_max ? fmaxf(t[2 * w], t[2 * w + 1]) : t[2 * w] + t[2 * w + 1];
  return t[0];
}

__device__ __forceinline__ void rf_block2(float& u, float& v, bool u_is_max, float* sa, float* sb) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float uo = __shfl_xor(u, o, 64), vo = __shfl_xor(v, o, 64);
    u = u_is_max ? fmaxf(u, uo) : u + uo;
    v += vo;
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sa[wave] = u; sb[wave] = v; }
  __syncthreads();
  u = rf_tree(sa, 1, u_is_max);
  v = rf_tree(sb, 1, false);
  __syncthreads();
}

// max, sum exp(. - max), sum exp^2 and the plain sum of image b's k values at lw: every thread returns the same four
__device__ __forceinline__ void rf_reduce(const float* lw, int k, float* sa, float* sb, float& m, float& e1, float& e2,
                                          float& tot) {
  const int tid = threadIdx.x;
  float mv = -INFINITY, tv = 0.f;
  for (int s = tid; s < k; s += kThreads) {
    const float v = lw[s];
    mv = fmaxf(mv, v);                           // (a NaN weight reaches the outputs through the sums)
    tv += v;
  }
  rf_block2(mv, tv, true, sa, sb);
  m = mv; tot = tv;
  float x1 = 0.f, x2 = 0.f;
  for (int s = tid; s < k; s += kThreads) {
    const float e = expf(lw[s] - m);
    x1 += e;
    x2 = __builtin_fmaf(e, e, x2);
  }
  rf_block2(x1, x2, false, sa, sb);
  e1 = x1; e2 = x2;
}

// Phases 1 to 3 of image b: the bound, the gradients of (m, ls), Adam ascent and the clamp
template <int G>
__device__ __forceinline__ void rf_update(const RefineArgs& a, int b, float* sa, float* sb) {
  const int tid = threadIdx.x;
  float* lw = a.lw + (size_t)b * a.k;
  rf_log_weights<G>(a, b, a.lw);
  __syncthreads();
  float m, e1, e2, tot;
  rf_reduce(lw, a.k, sa, sb, m, e1, e2, tot);
  const float invk = 1.f / (float)a.k;
  if (tid == 0 && a.bound) a.bound[b] = a.objective ? m + logf(e1) - logf((float)a.k) : tot * invk;
  if (a.objective) {
    for (int s = tid; s < a.k; s += kThreads) lw[s] = expf(lw[s] - m) / e1;
    __syncthreads();
  }
  const int lane = tid & 63, wave = tid >> 6;
  for (int i = 0; i < a.L; ++i) {
    const int d = a.d[i];
    const float* __restrict__ gi = a.g[i];
    const float* __restrict__ ei = a.epsw[i];
    for (int j0 = 0; j0 < d; j0 += kCols) {
      // thread t < kCols updates column j0 + t afterwards: its parameters and moments are fetched beside the sums' loads
      const bool upd = tid < kCols && j0 + tid < d;
      const size_t p = (size_t)b * d + j0 + tid;
      float pm = 0.f, ls = 0.f, m1 = 0.f, m2 = 0.f, s1 = 0.f, s2 = 0.f;
      if (upd) {
        pm = a.mean[i][p]; ls = a.logstd[i][p];
        if (!a.zero) { m1 = a.m1m[i][p]; m2 = a.m2m[i][p]; s1 = a.m1s[i][p]; s2 = a.m2s[i][p]; }
      }
      float gm[kCols / 64], gl[kCols / 64];
#pragma unroll
      for (int c = 0; c < kCols / 64; ++c) gm[c] = gl[c] = 0.f;
#pragma unroll 2
      for (int s = wave; s < a.k; s += kWaves) {
        const size_t o = ((size_t)s * a.N + b) * d + j0 + lane;
        const float w = a.objective ? lw[s] : invk;
#pragma unroll
        for (int c = 0; c < kCols / 64; ++c) {
          if (j0 + 64 * c + lane < d) {
            const float wg = w * gi[o + 64 * c];
            gm[c] += wg;
            gl[c] = __builtin_fmaf(wg, ei[o + 64 * c], gl[c]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < kCols / 64; ++c) { sa[c * kThreads + tid] = gm[c]; sb[c * kThreads + tid] = gl[c]; }
      __syncthreads();
      if (upd) {                                     // (wave w < 4 takes the columns of chunk w)
        const float Gm = rf_tree(sa + wave * kThreads + lane, 64, false);
        const float Sl = rf_tree(sb + wave * kThreads + lane, 64, false);
        const float Gl = __builtin_fmaf(Sl, expf(ls), 1.f);
        m1 = m1 + (Gm - m1) * a.omb1;
        m2 = m2 + (Gm * Gm - m2) * a.omb2;
        a.m1m[i][p] = m1; a.m2m[i][p] = m2;
        a.mean[i][p] = pm + (m1 * a.lr_n) / (sqrtf(m2) + a.eps_hat);
        s1 = s1 + (Gl - s1) * a.omb1;
        s2 = s2 + (Gl * Gl - s2) * a.omb2;
        a.m1s[i][p] = s1; a.m2s[i][p] = s2;
        ls = ls + (s1 * a.lr_n) / (sqrtf(s2) + a.eps_hat);
        ls = ls < a.ls_min ? a.ls_min : ls > a.ls_max ? a.ls_max : ls;      // (a NaN stays a NaN)
        a.logstd[i][p] = ls;
      }
      __syncthreads();
    }
  }
}

// Phase 4 of image b: h = fmaf(exp(ls), eps, m) for the k samples of pass a.pass, latents and noise into the workspace
__device__ __forceinline__ void rf_draw(const RefineArgs& a, int b) {
  const uint64_t base = *a.rng_base + a.pass;
  for (int i = 0; i < a.L; ++i) {
    const int d = a.d[i], nq = (d + 3) >> 2;
    const float* __restrict__ mu = a.mean[i] + (size_t)b * d;       // (nothing below writes the parameters)
    const float* __restrict__ ls = a.logstd[i] + (size_t)b * d;
    const float* __restrict__ inj = a.eps_in[i];
    const long long n = (long long)a.k * nq;
    for (long long t = threadIdx.x; t < n; t += kThreads) {
      const int s = (int)(t / nq), q = (int)(t - (long long)s * nq), j = 4 * q;
      const size_t o = ((size_t)s * a.N + b) * d + j;
      const int w = std::min(4, d - j);
      float e[4] = {0.f, 0.f, 0.f, 0.f}, hv[4];
      if (inj) {
        for (int c = 0; c < w; ++c) e[c] = inj[o + c];
      } else {
        const float4 z = philox_normal4(a.seed, base, (unsigned)((long long)b * a.k + s), (unsigned)(a.noise_layer + i),
                                        (unsigned)q);
        e[0] = z.x; e[1] = z.y; e[2] = z.z; e[3] = z.w;
      }
      for (int c = 0; c < w; ++c) hv[c] = __builtin_fmaf(expf(ls[j + c]), e[c], mu[j + c]);
      if (a.vec[i]) {                              // d % 4 == 0: the quad is whole and 16-byte aligned
        *reinterpret_cast<float4*>(a.lat[i] + o) = make_float4(hv[0], hv[1], hv[2], hv[3]);
        *reinterpret_cast<float4*>(a.epsw[i] + o) = make_float4(e[0], e[1], e[2], e[3]);
      } else {
        for (int c = 0; c < w; ++c) { a.lat[i][o + c] = hv[c]; a.epsw[i][o + c] = e[c]; }
      }
    }
  }
}

}  // namespace

// Pass 0's samples at the caller's parameters
__global__ __launch_bounds__(kThreads) void refine_begin_kernel(RefineArgs a) { rf_draw(a, blockIdx.x); }

// Iteration t's reduction and Adam update, then pass t + 1's samples at the updated parameters
template <int G>
__global__ __launch_bounds__(kThreads) void refine_step_kernel(RefineArgs a) {
  __shared__ float sa[kCols / 64 * kThreads], sb[kCols / 64 * kThreads];
  rf_update<G>(a, blockIdx.x, sa, sb);
  rf_draw(a, blockIdx.x);                          // (rf_update ends on a barrier: the new parameters are visible)
}

// The last update; the evaluation pass's samples where there is one
template <int G>
__global__ __launch_bounds__(kThreads) void refine_end_kernel(RefineArgs a) {
  __shared__ float sa[kCols / 64 * kThreads], sb[kCols / 64 * kThreads];
  rf_update<G>(a, blockIdx.x, sa, sb);
  if (a.draw) rf_draw(a, blockIdx.x);
}

// Per image: log w of the evaluation samples, logpx = logsumexp_s log_w - log k, ess = (sum e)^2 / sum e^2, the copy of
// the samples; thread 0 of workgroup 0 moves the noise position on by the call's passes.
template <int G>
__global__ __launch_bounds__(kThreads) void refine_finish_kernel(RefineArgs a) {
  __shared__ float sa[kCols / 64 * kThreads], sb[kCols / 64 * kThreads];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (b == 0 && tid == 0 && a.rng_adv) {
    a.rng_adv[1] = a.rng_adv[0] + (a.n_adv - 1);
    a.rng_adv[0] += a.n_adv;
  }
  if (!a.eval) return;
  for (int i = 0; i < a.L; ++i) {
    if (!a.lat_out[i]) continue;
    const int d = a.d[i];
    const long long n = (long long)a.k * d;
    for (long long t = tid; t < n; t += kThreads) {
      const int s = (int)(t / d), j = (int)(t - (long long)s * d);
      const size_t o = ((size_t)s * a.N + b) * d + j;
      a.lat_out[i][o] = a.lat[i][o];
    }
  }
  if (!a.log_w) return;
  rf_log_weights<G>(a, b, a.log_w);
  __syncthreads();
  if (!a.logpx && !a.ess) return;
  float m, e1, e2, tot;
  rf_reduce(a.log_w + (size_t)b * a.k, a.k, sa, sb, m, e1, e2, tot);
  if (tid == 0) {
    if (a.logpx) a.logpx[b] = m + logf(e1) - logf((float)a.k);
    if (a.ess) a.ess[b] = e1 * e1 / e2;
  }
}

hipError_t launch_refine_begin(hipStream_t st, const RefineArgs& a) {
  if (a.N <= 0) return hipSuccess;
  hipLaunchKernelGGL(refine_begin_kernel, dim3(a.N), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_refine_step(hipStream_t st, const RefineArgs& a) {
  if (a.N <= 0) return hipSuccess;
  if (a.group == 16) hipLaunchKernelGGL(refine_step_kernel<16>, dim3(a.N), dim3(kThreads), 0, st, a);
  else if (a.group == 64) hipLaunchKernelGGL(refine_step_kernel<64>, dim3(a.N), dim3(kThreads), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_refine_end(hipStream_t st, const RefineArgs& a) {
  if (a.N <= 0) return hipSuccess;
  if (a.group == 16) hipLaunchKernelGGL(refine_end_kernel<16>, dim3(a.N), dim3(kThreads), 0, st, a);
  else if (a.group == 64) hipLaunchKernelGGL(refine_end_kernel<64>, dim3(a.N), dim3(kThreads), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_refine_finish(hipStream_t st, const RefineArgs& a) {
  if (a.N <= 0) return hipSuccess;
  const dim3 grid(a.eval ? a.N : 1);
  if (a.group == 16) hipLaunchKernelGGL(refine_finish_kernel<16>, grid, dim3(kThreads), 0, st, a);
  else if (a.group == 64) hipLaunchKernelGGL(refine_finish_kernel<64>, grid, dim3(kThreads), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace iwae
