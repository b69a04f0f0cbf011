// Thermodynamic variational objective (Masrani, Le & Wood 2019): per image, the
// J + 1 self-normalised softmaxes of its k log weights at the partition's
// temperatures, their means, the two Riemann sums around the IWAE value and the
// covariance-form row coefficients (TvoArgs, iwae_kernels.h).
// bound_kernel's discipline: one wave per image, lanes over samples, the image's
// log weights staged in the wave's LDS slice (k <= 1024) or re-read by the lane
// that owns them, every reduction in a fixed order, no float atomics.
#include "iwae_kernels.h"
#include "iwae_bound.h"

namespace iwae {

constexpr int kTvoWaves = 16;

// Last-arriving workgroup detection (agent-scope release/acquire, counter form;
// bound_kernel's).
__device__ __forceinline__ bool tvo_last_block(unsigned* ticket) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1);
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  return s_last != 0;
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One image on one wave.  sh: the wave's staging (1024 floats); sj: its
// per-temperature results, Z_j in sj[j] and the centred mean
// md_j = m_j - max in sj[kTvoMaxPart + 1 + j].  Returns (lower, upper, iwae) in
// every lane.
__device__ __forceinline__ float3 tvo_image(const TvoArgs& a, int b, float* sh, float* sj) {
  const int lane = threadIdx.x & 63;
  const int kS = a.kS, J = a.J;
  const size_t row0 = (size_t)b * kS;
  const bool staged = kS <= 1024;
  const float* g = a.lw_in ? a.lw_in + row0 : a.lw_out + row0;
  // the log weights, their maximum, and whether every one is finite
  float mx = -INFINITY;
  bool bad = false;
  for (int q = lane; q < kS; q += 64) {
    float v;
    if (a.lw_in) {
      v = g[q];
    } else {
      const int r = (int)row0 + q;
      v = __fsub_rn(__fadd_rn(a.logp[r], row_sum_parts(a.part, a.ldpart, a.npart, r)), a.logq[r]);
      a.lw_out[r] = v;
    }
    if (staged) sh[q] = v;
    mx = fmaxf(mx, v);
    bad |= !(fabsf(v) <= 3.402823466e38f);
  }
  if (staged) wave_lds_sync();
  mx = wave_max(mx);
  // (one maximum serves every temperature: all beta >= 0.  A NaN or an infinity
  // anywhere in the image makes the shift, and with it every output, NaN)
  if (__any(bad)) mx = __builtin_nanf("");
  auto lw = [&](int q) { return staged ? sh[q] : g[q]; };
  // pass 1, j ascending: Z_j = sum_s exp(beta_j (lw_s - max)) and the centred mean
  for (int j = 0; j <= J; ++j) {
    const float bj = a.beta[j];
    float z = 0.f, sd = 0.f;
    for (int q = lane; q < kS; q += 64) {
      const float d = lw(q) - mx;
      const float e = expf(bj * d);
      z += e;
      sd += e * d;
    }
    z = wave_sum(z);
    sd = wave_sum(sd);
    if (lane == 0) {
      sj[j] = z;
      sj[kTvoMaxPart + 1 + j] = sd / z;
    }
  }
  wave_lds_sync();
  // the Riemann sums and the IWAE value (beta_J = 1: Z_J is its sum of exponentials)
  float lower = 0.f, upper = 0.f;
  for (int j = 0; j < J; ++j) {
    const float dj = a.beta[j + 1] - a.beta[j];
    lower += dj * (mx + sj[kTvoMaxPart + 1 + j]);
    upper += dj * (mx + sj[kTvoMaxPart + 2 + j]);
  }
  const float iw = logf(sj[J] / (float)kS) + mx;
  if (lane == 0) {
    if (a.lower) a.lower[b] = lower;
    if (a.upper) a.upper[b] = upper;
    if (a.iwae) a.iwae[b] = iw;
  }
  // pass 2: a row's two coefficients, j ascending
  if (a.a_theta || a.a_theta2 || a.a_phi) {
    for (int q = lane; q < kS; q += 64) {
      const float d = lw(q) - mx;
      float at = 0.f, ap = 0.f;
      for (int j = 0; j < J; ++j) {
        const float bj = a.beta[j];
        const float dj = a.beta[j + 1] - bj;
        const float w = expf(bj * d) / sj[j];
        const float c = d - sj[kTvoMaxPart + 1 + j];
        at += dj * (w * (1.f + bj * c));
        ap += dj * (w * ((1.f - bj) * c - 1.f));
      }
      const size_t r = row0 + q;
      if (a.a_theta) a.a_theta[r] = a.s_theta * at;
      if (a.a_theta2) a.a_theta2[r] = a.s_theta * at;
      if (a.a_phi) a.a_phi[r] = a.s_phi * ap;
    }
  }
  // (the next image of this wave overwrites sh and sj: every lane is past its reads)
  wave_lds_sync();
  return make_float3(lower, upper, iw);
}

__global__ __launch_bounds__(kTvoWaves * 64) void tvo_kernel(TvoArgs a) {
  __shared__ float sh_all[kTvoWaves][1024];
  __shared__ float sj_all[kTvoWaves][2 * (kTvoMaxPart + 1)];
  __shared__ float red[3][kTvoWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int b = blockIdx.x * kTvoWaves + wave; b < a.Bimg; b += gridDim.x * kTvoWaves) {
    const float3 v = tvo_image(a, b, sh_all[wave], sj_all[wave]);
    s0 += v.x; s1 += v.y; s2 += v.z;
  }
  if (!a.values) return;
  bool finalize;
  if (gridDim.x == 1) {
    // one workgroup: per-wave sums in a fixed order, no global round trip
    if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; red[2][wave] = s2; }
    __syncthreads();
    finalize = true;
  } else {
    finalize = tvo_last_block(a.ticket);
    if (finalize) {
      s0 = s1 = s2 = 0.f;
      for (int i = threadIdx.x; i < a.Bimg; i += blockDim.x) {
        s0 += a.lower[i]; s1 += a.upper[i]; s2 += a.iwae[i];
      }
      s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
      if (lane == 0) { red[0][wave] = s0; red[1][wave] = s1; red[2][wave] = s2; }
      __syncthreads();
    }
  }
  if (finalize && threadIdx.x == 0) {
    for (int v = 0; v < 3; ++v) {
      float tot = 0.f;
      for (int i = 0; i < kTvoWaves; ++i) tot += red[v][i];
      a.values[v] = -(tot / (float)a.Bimg);
    }
    // the Philox base of the next pass, the Adam step of this one (bound_finalize's)
    if (a.rng_base) { a.rng_base[1] = a.rng_base[0]; a.rng_base[0] += 1; }
    if (a.adam_step) *a.adam_step += 1;
    if (gridDim.x > 1) *a.ticket = 0u;
  }
}

// workgroups of a launch: bound_grid's rule
int tvo_grid(const TvoArgs& a) {
  const long long rows = (long long)a.Bimg * a.kS;
  return (a.Bimg <= 4 * kTvoWaves || rows <= 8192) ? 1 : (a.Bimg + kTvoWaves - 1) / kTvoWaves;
}

hipError_t launch_tvo(hipStream_t st, const TvoArgs& a) {
  if (a.Bimg <= 0) return hipSuccess;
  if (a.kS < 1 || a.J < 1 || a.J > kTvoMaxPart) return hipErrorInvalidValue;
  if (!a.lw_in && (!a.lw_out || !a.logp || !a.logq || !a.part)) return hipErrorInvalidValue;
  const int grid = tvo_grid(a);
  if (a.values && grid > 1 && (!a.ticket || !a.lower || !a.upper || !a.iwae)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tvo_kernel, dim3(grid), dim3(kTvoWaves * 64), 0, st, a);
  return hipGetLastError();
}

}  // namespace iwae
