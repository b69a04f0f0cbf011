// Imputation of missing pixels under the importance-weighted posterior (Mattei
// & Frellsen 2019, iwae_impute), gfx950: the small kernels around the masked
// first pass.  The pixel mask is [images][x_dim], non-zero = observed.
//
//   impute_stage_kernel    the chunk's images staged twice by select: mask ? x : 0
//                          (the encoder's input) and mask ? x : -1 (the pixels
//                          the masked mega_fwd_kernel reads)
//   impute_rowsum_kernel   layer-wise first pass: a row's masked Bernoulli
//                          log-likelihood from its stored logits
//   impute_fill_kernel     x_mean = mask ? x : sum_s w~_s p(x | h_{1,s})
//   impute_draw_kernel     x_draw = mask ? x : (u < p(x | h_{1,s*}))
//
// Every kernel selects by the mask and never multiplies by it, so whatever a
// missing entry of x holds (NaN, Inf) gives the bits a 0 there gives.
// Deterministic: fixed reduction order, each output written by one lane.
#include "iwae_bound.h"

namespace iwae {

constexpr float kImpOff0 = 9.1327896e-7f;    // 1 - 0.999999f - 1e-7f: 1 - p without the f32 cancellation (F:126)

__global__ __launch_bounds__(256) void impute_stage_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                           int n, int xdim, float* x_in, int ld_in, float* xm,
                                                           int ld_m) {
  const int W = xm ? ld_m : xdim;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * W) return;
  const int r = (int)(i / W), j = (int)(i - (long long)r * W);
  if (j >= xdim) {
    xm[(size_t)r * ld_m + j] = 0.f;            // padding: an observed 0 the column bound masks anyway
    return;
  }
  const bool obs = mask[(size_t)r * xdim + j] != 0.f;
  const float v = x[(size_t)r * xdim + j];
  x_in[(size_t)r * ld_in + j] = obs ? v : 0.f;
  if (xm) xm[(size_t)r * ld_m + j] = obs ? v : -1.f;
}
hipError_t launch_impute_stage(hipStream_t st, const float* x, const float* mask, int n, int xdim, float* x_in,
                               int ld_in, float* xm, int ld_m) {
  const long long t = (long long)n * (xm ? ld_m : xdim);
  if (t <= 0) return hipSuccess;
  hipLaunchKernelGGL(impute_stage_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, x, mask, n, xdim, x_in,
                     ld_in, xm, ld_m);
  return hipGetLastError();
}

// One wave per row: lane l adds columns l, l + 64, ... in order, then the
// butterfly sum.  Exact expf / logf (evaluation only); both probabilities are
// formed without cancellation and neither exponential's overflow reaches a
// product (1 / (1 + inf) = 0).  p is bern_probs_kernel's expression.
__global__ __launch_bounds__(256) void impute_rowsum_kernel(float* Z, int ldz, int rows, int kS,
                                                            const float* __restrict__ x_in, int ld_in,
                                                            const float* __restrict__ mask, int xdim, float* part,
                                                            int to_probs) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                       // (wave-uniform)
  const int b = (int)(r / kS);
  float* z = Z + (size_t)r * ldz;
  const float* xr = x_in + (size_t)b * ld_in;
  const float* mr = mask + (size_t)b * xdim;
  float acc = 0.f;
  for (int j = lane; j < xdim; j += 64) {
    const float zv = z[j], xv = xr[j];
    const float p1 = (1.f / (1.f + expf(-zv))) * kProbScale + kProbShift;
    const float p0 = (1.f / (1.f + expf(zv))) * kProbScale + kImpOff0;
    const float v = xv * logf(p1) + (1.f - xv) * logf(p0);
    acc += mr[j] != 0.f ? v : 0.f;
    if (to_probs) z[j] = p1;
  }
  acc = wave_sum(acc);
  if (lane == 0) *reinterpret_cast<float4*>(part + (size_t)r * 4) = make_float4(acc, 0.f, 0.f, 0.f);
}
hipError_t launch_impute_rowsum(hipStream_t st, float* Z, int ldz, int rows, int kS, const float* x_in, int ld_in,
                                const float* mask, int xdim, float* part, int to_probs) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(impute_rowsum_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, Z, ldz, rows, kS, x_in,
                     ld_in, mask, xdim, part, to_probs);
  return hipGetLastError();
}

// VEC: x_dim a multiple of 4 and x / mask 16-byte aligned (out always is): one float4 per thread
template <bool VEC>
__global__ __launch_bounds__(256) void impute_fill_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                          int n, int xdim, float* out, int ldo) {
  const int W = VEC ? xdim >> 2 : xdim;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * W) return;
  const int r = (int)(i / W), c = (int)(i - (long long)r * W);
  if (VEC) {
    const float4 xv = reinterpret_cast<const float4*>(x + (size_t)r * xdim)[c];
    const float4 mv = reinterpret_cast<const float4*>(mask + (size_t)r * xdim)[c];
    float4* o = reinterpret_cast<float4*>(out + (size_t)r * ldo) + c;
    float4 v = *o;
    v.x = mv.x != 0.f ? xv.x : v.x;
    v.y = mv.y != 0.f ? xv.y : v.y;
    v.z = mv.z != 0.f ? xv.z : v.z;
    v.w = mv.w != 0.f ? xv.w : v.w;
    *o = v;
  } else if (mask[(size_t)r * xdim + c] != 0.f) {
    out[(size_t)r * ldo + c] = x[(size_t)r * xdim + c];
  }
}
hipError_t launch_impute_fill(hipStream_t st, const float* x, const float* mask, int n, int xdim, float* out, int ldo) {
  if (n <= 0) return hipSuccess;
  const bool vec = !(xdim & 3) && !(((uintptr_t)x | (uintptr_t)mask) & 15);
  const long long t = (long long)n * (vec ? xdim >> 2 : xdim);
  const dim3 grid((unsigned)((t + 255) / 256)), block(256);
  if (vec) hipLaunchKernelGGL(impute_fill_kernel<true>, grid, block, 0, st, x, mask, n, xdim, out, ldo);
  else hipLaunchKernelGGL(impute_fill_kernel<false>, grid, block, 0, st, x, mask, n, xdim, out, ldo);
  return hipGetLastError();
}

// One thread per (row, column quad), gen_pixels_kernel's uniforms
__global__ __launch_bounds__(256) void impute_draw_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                          const float* __restrict__ p, int ldp,
                                                          const float* __restrict__ u, int n, int xdim, float* out,
                                                          int ldo, uint64_t seed, const uint64_t* rng_base, int layer) {
  const int ng = (xdim + 3) >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * ng) return;
  const int r = (int)(i / ng), g = (int)(i - (long long)r * ng);
  const float4 u4 = pixel_uniform4(u, r, g, xdim, seed, rng_base, layer);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = 4 * g + q;
    if (j >= xdim) break;
    const float d = f4_at(u4, q) < p[(size_t)r * ldp + j] ? 1.f : 0.f;
    out[(size_t)r * ldo + j] = mask[(size_t)r * xdim + j] != 0.f ? x[(size_t)r * xdim + j] : d;
  }
}
hipError_t launch_impute_draw(hipStream_t st, const float* x, const float* mask, const float* p, int ldp,
                              const float* u, int n, int xdim, float* out, int ldo, uint64_t seed,
                              const uint64_t* rng_base, int layer) {
  const long long t = (long long)n * ((xdim + 3) >> 2);
  if (t <= 0) return hipSuccess;
  hipLaunchKernelGGL(impute_draw_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, x, mask, p, ldp, u, n,
                     xdim, out, ldo, seed, rng_base, layer);
  return hipGetLastError();
}

}  // namespace iwae
