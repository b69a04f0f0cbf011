// Device code of iwae_ais (gfx950): everything of an annealed-importance-
// sampling transition between the gradient launches (AisArgs in
// iwae_kernels.h).  A chain is one (image b, sample s) row, c = b k + s; its
// latents, momenta and gradients are sample-major rows ((s N + b) d_i), its
// scalars image-major [N][k].
//
// Mapping.  The launches move 3 to 5 floats per latent column and are bound by
// memory and launch latency, so the only choice is how the lanes meet the rows.
// A chain's rows are 5 to a few hundred contiguous floats: a group of lanes
// (16 while every d_i <= 64, else the whole wave) own one chain and walk each
// layer's row in strides of the group, so a group's loads of a row are
// contiguous and at d = 6 a wave still serves four chains.  The kinetic energy
// is each lane's sum over its columns in layer, then column order, folded by
// an xor butterfly over the group (__shfl_xor: four ds_bpermute per chain at 16
// lanes, nothing beside the launch's latency): one order, whatever the grid.
// ais_step_kernel has no reduction and is plain elementwise, one thread per
// float4 (or float) of a layer.
#include <algorithm>
#include <cmath>

#include "iwae_kernels.h"

namespace iwae {

namespace {

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

// U = -(c_q log q + c_ph log p(h) + c_px log p(x|h)) of chain c; a term whose coefficient is 0 is left out
__device__ __forceinline__ float ais_energy(const AisArgs& a, size_t c) {
  float v = 0.f;
  if (a.cq != 0.f) v += a.cq * a.lq[c];
  if (a.cph != 0.f) v += a.cph * a.lph[c];
  if (a.cpx != 0.f) v += a.cpx * a.lpx[c];
  return -v;
}

}  // namespace

// Per chain: momenta (injected, or Philox normals), 1/2 |r|^2, log_w += dbeta Delta, H_old, then the first
// half kick r += eps/2 g and the drift q = cur + eps r into the proposal buffers.
template <int G>
__global__ __launch_bounds__(256) void ais_begin_kernel(AisArgs a) {
  const int sub = threadIdx.x & (G - 1);
  const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
  if (c >= a.chains) return;
  const int b = (int)(c / a.k), s = (int)(c - (long long)b * a.k);
  const size_t row = (size_t)s * a.N + b;
  const float eps = a.step0 > 0.f ? a.step0 : a.step[c];
  const float he = 0.5f * eps;
  const uint64_t base = *a.rng_base + a.t_off;
  float ke = 0.f;
  for (int i = 0; i < a.L; ++i) {
    const int d = a.d[i];
    const size_t o = row * d;
    const float* __restrict__ cur = a.cur[i] + o;
    const float* __restrict__ g = a.g[i] + o;
    float* __restrict__ r = a.r[i] + o;
    float* __restrict__ q = a.q[i] + o;
    for (int j = sub; j < d; j += G) {
      float rv;
      if (a.mom[i]) {
        rv = a.mom[i][o + j];
      } else {
        const float4 n = philox_normal4(a.seed, base, (unsigned)c, (unsigned)(a.mom_layer + i), (unsigned)(j >> 2));
        rv = f4_at(n, j & 3);
      }
      ke = __builtin_fmaf(rv, rv, ke);
      rv = __builtin_fmaf(he, g[j], rv);
      r[j] = rv;
      q[j] = __builtin_fmaf(eps, rv, cur[j]);
    }
  }
  ke = group_sum<G>(ke);
  if (sub == 0) {
    const float delta = a.init ? (a.lph[c] + a.lpx[c]) - a.lq[c] : a.lpx[c];
    if (a.log_w) a.log_w[c] = (a.zero ? 0.f : a.log_w[c]) + a.dbeta * delta;
    a.H_old[c] = ais_energy(a, (size_t)c) + 0.5f * ke;
  }
}

// Elementwise over a layer (blockIdx.y): r += eps g, q += eps r with the chain's own eps
__global__ __launch_bounds__(256) void ais_step_kernel(AisArgs a) {
  const int i = blockIdx.y;
  const int d = a.d[i];
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int w = a.vec[i] ? 4 : 1;
  const long long e = t * w;                       // first element of this thread
  const long long per = (long long)a.N * d;
  if (e >= per * a.k) return;
  const int s = (int)(e / per);
  const int b = (int)((e - (long long)s * per) / d);
  const size_t c = (size_t)b * a.k + s;
  const float eps = a.step0 > 0.f ? a.step0 : a.step[c];
  if (a.vec[i]) {                                  // d % 4 == 0: the four columns are one chain's
    const float4 g = *reinterpret_cast<const float4*>(a.g[i] + e);
    float4 r = *reinterpret_cast<float4*>(a.r[i] + e);
    float4 q = *reinterpret_cast<float4*>(a.q[i] + e);
    r.x = __builtin_fmaf(eps, g.x, r.x); r.y = __builtin_fmaf(eps, g.y, r.y);
    r.z = __builtin_fmaf(eps, g.z, r.z); r.w = __builtin_fmaf(eps, g.w, r.w);
    q.x = __builtin_fmaf(eps, r.x, q.x); q.y = __builtin_fmaf(eps, r.y, q.y);
    q.z = __builtin_fmaf(eps, r.z, q.z); q.w = __builtin_fmaf(eps, r.w, q.w);
    *reinterpret_cast<float4*>(a.r[i] + e) = r;
    *reinterpret_cast<float4*>(a.q[i] + e) = q;
  } else {
    const float r = __builtin_fmaf(eps, a.g[i][e], a.r[i][e]);
    a.r[i][e] = r;
    a.q[i][e] = __builtin_fmaf(eps, r, a.q[i][e]);
  }
}

// Per chain: the last half kick, 1/2 |r|^2, H_new, accept iff log u < H_old - H_new (false for a NaN), the
// state's select, the accept count and the step's adaptation.
template <int G>
__global__ __launch_bounds__(256) void ais_end_kernel(AisArgs a) {
  const int sub = threadIdx.x & (G - 1);
  const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
  if (c >= a.chains) return;
  const int b = (int)(c / a.k), s = (int)(c - (long long)b * a.k);
  const size_t row = (size_t)s * a.N + b;
  const float eps = a.step0 > 0.f ? a.step0 : a.step[c];
  const float he = 0.5f * eps;
  float ke = 0.f;
  for (int i = 0; i < a.L; ++i) {
    const int d = a.d[i];
    const size_t o = row * d;
    const float* __restrict__ g = a.g[i] + o;
    const float* __restrict__ r = a.r[i] + o;
    for (int j = sub; j < d; j += G) {
      const float rv = __builtin_fmaf(he, g[j], r[j]);
      ke = __builtin_fmaf(rv, rv, ke);
    }
  }
  ke = group_sum<G>(ke);
  int acc = 0;
  if (sub == 0) {
    const float H_new = ais_energy(a, (size_t)c) + 0.5f * ke;
    float uv;
    if (a.u) uv = a.u[c];
    else uv = philox_uniform4(a.seed, *a.rng_base + a.t_off, (unsigned)c, (unsigned)a.u_layer, 0u).x;
    acc = logf(uv) < a.H_old[c] - H_new ? 1 : 0;
    if (a.accepts) a.accepts[c] = (a.zero ? 0.f : a.accepts[c]) + (float)acc;
    a.step[c] = fminf(fmaxf(eps * (acc ? a.inc : a.dec), a.smin), a.smax);
  }
  acc = __shfl(acc, 0, G);
  if (!acc) return;
  for (int i = 0; i < a.L; ++i) {
    const int d = a.d[i];
    const size_t o = row * d;
    const float* __restrict__ q = a.q[i] + o;
    float* __restrict__ cur = a.cur[i] + o;
    for (int j = sub; j < d; j += G) cur[j] = q[j];
  }
}

// Per image (one workgroup): logpx = logsumexp_s log_w - log k and ess = (sum e)^2 / sum e^2, e = exp(log_w -
// max): thread i takes samples i, i + 256, ... in order, the 256 partials fold in a fixed tree.  Thread 0 of
// workgroup 0 moves the noise position on by the call's transitions.
__global__ __launch_bounds__(256) void ais_finish_kernel(const float* __restrict__ log_w, int k, float* logpx,
                                                         float* ess, uint64_t* rng_base, unsigned n_adv) {
  __shared__ float sa[256], sb[256];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && tid == 0 && rng_base) {
    rng_base[1] = rng_base[0] + (n_adv - 1);
    rng_base[0] += n_adv;
  }
  if (!log_w || (!logpx && !ess)) return;
  const float* lw = log_w + (size_t)blockIdx.x * k;
  float m = -INFINITY;
  for (int s = tid; s < k; s += 256) m = fmaxf(m, lw[s]);
  sa[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sa[tid] = fmaxf(sa[tid], sa[tid + o]);
    __syncthreads();
  }
  m = sa[0];
  __syncthreads();
  float e1 = 0.f, e2 = 0.f;
  for (int s = tid; s < k; s += 256) {
    const float e = expf(lw[s] - m);
    e1 += e;
    e2 = __builtin_fmaf(e, e, e2);
  }
  sa[tid] = e1; sb[tid] = e2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sa[tid] += sa[tid + o]; sb[tid] += sb[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    if (logpx) logpx[blockIdx.x] = m + logf(sa[0]) - logf((float)k);
    if (ess) ess[blockIdx.x] = sa[0] * sa[0] / sb[0];
  }
}

static unsigned ais_chain_blocks(const AisArgs& a) { return (unsigned)((a.chains * a.group + 255) / 256); }

hipError_t launch_ais_begin(hipStream_t st, const AisArgs& a) {
  if (a.chains <= 0) return hipSuccess;
  if (a.group == 16) hipLaunchKernelGGL(ais_begin_kernel<16>, dim3(ais_chain_blocks(a)), dim3(256), 0, st, a);
  else if (a.group == 64) hipLaunchKernelGGL(ais_begin_kernel<64>, dim3(ais_chain_blocks(a)), dim3(256), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_ais_step(hipStream_t st, const AisArgs& a) {
  if (a.chains <= 0 || a.L <= 0) return hipSuccess;
  long long most = 0;
  for (int i = 0; i < a.L; ++i) most = std::max(most, a.chains * a.d[i] / (a.vec[i] ? 4 : 1));
  if (most <= 0) return hipSuccess;
  hipLaunchKernelGGL(ais_step_kernel, dim3((unsigned)((most + 255) / 256), a.L), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ais_end(hipStream_t st, const AisArgs& a) {
  if (a.chains <= 0) return hipSuccess;
  if (a.group == 16) hipLaunchKernelGGL(ais_end_kernel<16>, dim3(ais_chain_blocks(a)), dim3(256), 0, st, a);
  else if (a.group == 64) hipLaunchKernelGGL(ais_end_kernel<64>, dim3(ais_chain_blocks(a)), dim3(256), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_ais_finish(hipStream_t st, const float* log_w, int N, int k, float* logpx, float* ess,
                             uint64_t* rng_base, unsigned n_adv) {
  if (N <= 0) return hipSuccess;
  const bool red = log_w && (logpx || ess);
  hipLaunchKernelGGL(ais_finish_kernel, dim3(red ? N : 1), dim3(256), 0, st, log_w, k, logpx, ess, rng_base, n_adv);
  return hipGetLastError();
}

}  // namespace iwae
