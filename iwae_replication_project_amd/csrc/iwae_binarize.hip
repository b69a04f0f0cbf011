// Dynamic binarisation (the stochastic "MNIST" setting, PDF p7 s3.1,
// iwae_binarize), gfx950: one streaming launch gathers the caller's grey-level
// rows by an index list and draws every pixel ~ Bernoulli(grey level).
//
//   binarize_kernel<VEC>   out[i][j] = (u < x[perm[i]][j] || x[perm[i]][j] >= 1)
//
// One thread per (output row, column quad); u is the caller's buffer or the
// Philox uniforms of (output row, layer, quad) -- iwae_generate's pixel layout.
// The x >= 1 clause: philox_uniform4 rounds c >= 0xFFFFFF80 to exactly 1.0f, so
// without it a grey level of 1 would miss about 3e-8 of its draws; with it a
// 0/1 image is a fixed point.  NaN, 0 and negative grey levels give 0.
// A source index outside [0, n_src) gives a row of zeros by select: the load
// itself goes to row 0.  No LDS, no atomics, each output written by one lane,
// and a thread reads its quad before it writes it (out may be x itself when
// the rows are not permuted).
#include "iwae_kernels.h"

namespace iwae {

// Every quad runs its ten Philox rounds, also where all four grey levels are
// <= 0, >= 1 or NaN and the result does not depend on u (MNIST's background):
// the kernel is bound by HBM bytes, and a branch around the rounds measured 3
// to 5 us SLOWER on the float4 path at 60000 x 784 (MNIST-like, dense) and no
// faster on all zeros (profiles/binarize_skip_ab.json).

__device__ __forceinline__ float bin_pixel(float u, float x) { return (u < x || x >= 1.f) ? 1.f : 0.f; }

// VEC: x_dim a multiple of 4 and x 16-byte aligned (out always is): one float4 load and store per thread
template <bool VEC>
__global__ __launch_bounds__(256) void binarize_kernel(const float* x, long long n_src,
                                                       const long long* __restrict__ perm,
                                                       const float* __restrict__ u, int n, int xdim, float* out,
                                                       int ldo, uint64_t seed, const uint64_t* __restrict__ rng_base,
                                                       int layer) {
  const int ng = (xdim + 3) >> 2;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * ng) return;
  const int r = (int)(i / ng), g = (int)(i - (long long)r * ng);
  const long long s = perm ? perm[r] : (long long)r;
  const bool ok = (unsigned long long)s < (unsigned long long)n_src;
  const float* xr = x + (size_t)(ok ? s : 0) * xdim;
  const int j = 4 * g;
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n_src > 0) {                                       // (uniform: an empty x has no row 0 to read)
    if (VEC) xv = reinterpret_cast<const float4*>(xr)[g];
    else xv = make_float4(xr[j], xr[min(j + 1, xdim - 1)], xr[min(j + 2, xdim - 1)], xr[min(j + 3, xdim - 1)]);
  }
  xv.x = ok ? xv.x : 0.f;
  xv.y = ok ? xv.y : 0.f;
  xv.z = ok ? xv.z : 0.f;
  xv.w = ok ? xv.w : 0.f;
  const float4 u4 = pixel_uniform4(u, r, g, xdim, seed, rng_base, layer);
  const float4 o = make_float4(bin_pixel(u4.x, xv.x), bin_pixel(u4.y, xv.y), bin_pixel(u4.z, xv.z),
                               bin_pixel(u4.w, xv.w));
  float* orow = out + (size_t)r * ldo;
  if (VEC) {
    reinterpret_cast<float4*>(orow)[g] = o;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j + q < xdim) orow[j + q] = f4_at(o, q);
  }
}

hipError_t launch_binarize(hipStream_t st, const float* x, long long n_src, const long long* perm, const float* u,
                           int n, int xdim, float* out, int ldo, uint64_t seed, const uint64_t* rng_base, int layer) {
  const long long t = (long long)n * ((xdim + 3) >> 2);
  if (t <= 0) return hipSuccess;
  if (t + 255 >= (1LL << 32)) return hipErrorInvalidValue;       // a launch holds fewer than 2^32 threads
  const bool vec = !(xdim & 3) && !((uintptr_t)x & 15);
  const dim3 grid((unsigned)((t + 255) / 256)), block(256);
  if (vec) hipLaunchKernelGGL(binarize_kernel<true>, grid, block, 0, st, x, n_src, perm, u, n, xdim, out, ldo, seed,
                              rng_base, layer);
  else hipLaunchKernelGGL(binarize_kernel<false>, grid, block, 0, st, x, n_src, perm, u, n, xdim, out, ldo, seed,
                          rng_base, layer);
  return hipGetLastError();
}

}  // namespace iwae
