// Internal kernel interfaces of libiwae_hip.so (gfx950 only).
//
// Storage conventions shared by every kernel:
//  * all matrices are row-major float32 with a leading dimension that is a
//    multiple of 4 floats (16 B), so every row starts 16-byte aligned;
//  * columns between the logical width and the leading dimension are ZERO and
//    stay zero (buffers are memset at allocation and no kernel writes there),
//    except the "ones column" of GEMM inputs: an activation X[rows][fin] used as
//    a Dense input keeps X[:, fin] == 1.0 so that X_aug @ W_aug = X W + b with
//    W_aug = [W; b] ([fin+1][ld] -- exactly Keras' kernel-then-bias order), and
//    X_aug^T dZ yields dW and db in one GEMM;
//  * rows are image-major: row = b*k + s.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iwae {

constexpr float kProbScale = 0.999999f;      // F:126  (1-10**(-6)) as float32
constexpr float kLn2 = 0.693147180559945309f;
constexpr float kProbShift = 1e-7f;          // F:126  10**(-7)
constexpr float kScaleEps = 1e-6f;           // F:37
constexpr float kKerasEps = 1e-7f;           // keras.backend.epsilon()
constexpr float kHalfLog2Pi = 0.918938533204672742f;

// ------------------------------------------------------------ fast math ----
// Hardware transcendentals (v_exp_f32 / v_log_f32 / v_rcp_f32 / v_sin_f32,
// ~1 ulp) instead of the correctly-rounded library routines: the epilogues
// and prologues of the small-batch kernels are VALU-latency bound, and the
// parity budget (1e-4 relative on losses and gradients) is ~1000x their error.
__device__ __forceinline__ float fexp(float x) { return __expf(x); }
__device__ __forceinline__ float flog(float x) { return __logf(x); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }

// tanh: odd Taylor polynomial below |x| = 1/16 (truncation < 4e-9 relative),
// (1 - e)/(1 + e) with e = exp(-2|x|) above (< 2e-7 absolute).
__device__ __forceinline__ float ftanh(float x) {
  const float ax = fabsf(x);
  const float e = __expf(-2.f * ax);
  const float big = (1.f - e) * frcp(1.f + e);
  const float x2 = x * x;
  const float small = ax * __builtin_fmaf(x2, __builtin_fmaf(x2, 0.133333333f, -0.333333333f), 1.f);
  return copysignf(ax < 0.0625f ? small : big, x);
}

// Philox4x32-10 (Salmon et al. 2011) -> four N(0,1) by Box-Muller on both
// uniform pairs.  Counter = (row, layer << 20 | column group, base_lo,
// base_hi), key = seed; normal q of group g is the noise of column 4g + q.
// Every kernel that draws noise (fused and layer-wise paths, training and NLL)
// uses this one function, so both paths draw the identical stream.
// One Philox multiply: the 64-bit product of a 32-bit constant and a counter
// word (a single v_mad_u64_u32 in its place measured +0.2 % on the NLL: kept plain)
__device__ __forceinline__ void philox_mul(unsigned k, unsigned c, unsigned& lo, unsigned& hi) {
  lo = k * c;
  hi = __umulhi(k, c);
}
// a ^ b ^ k in one gfx950 v_bitop3_b32 (truth table 0x96); k is the
// wave-uniform Philox key word
__device__ __forceinline__ unsigned philox_xor3(unsigned a, unsigned b, unsigned k) {
  unsigned r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "s"(k));
  return r;
}
__device__ __forceinline__ float4 philox_normal4(uint64_t seed, uint64_t base, unsigned row, unsigned layer,
                                                 unsigned grp) {
  unsigned c0 = row, c1 = (layer << 20) | grp, c2 = (unsigned)base, c3 = (unsigned)(base >> 32);
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    unsigned lo0, hi0, lo1, hi1;
    philox_mul(0xD2511F53u, c0, lo0, hi0);
    philox_mul(0xCD9E8D57u, c2, lo1, hi1);
    c0 = philox_xor3(hi1, c1, k0); c1 = lo1; c2 = philox_xor3(hi0, c3, k1); c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  constexpr float k2m32 = 2.3283064365386963e-10f;
  const float u0 = ((float)c0 + 0.5f) * k2m32, u1 = ((float)c1 + 0.5f) * k2m32;   // (0, 1]
  const float u2 = ((float)c2 + 0.5f) * k2m32, u3 = ((float)c3 + 0.5f) * k2m32;
  // sqrt(-2 ln u) = sqrt(-2 ln2 * log2 u); v_sin/v_cos take revolutions
  const float r0 = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(u0));
  const float r1 = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(u2));
  return make_float4(r0 * __builtin_amdgcn_cosf(u1), r0 * __builtin_amdgcn_sinf(u1),
                     r1 * __builtin_amdgcn_cosf(u3), r1 * __builtin_amdgcn_sinf(u3));
}
// Normals 2*half and 2*half+1 of philox_normal4(...) (bitwise the same values):
// one Box-Muller pair, for a lane that owns two of the four columns.
__device__ __forceinline__ float2 philox_normal2(uint64_t seed, uint64_t base, unsigned row, unsigned layer,
                                                 unsigned grp, bool half) {
  unsigned c0 = row, c1 = (layer << 20) | grp, c2 = (unsigned)base, c3 = (unsigned)(base >> 32);
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    unsigned lo0, hi0, lo1, hi1;
    philox_mul(0xD2511F53u, c0, lo0, hi0);
    philox_mul(0xCD9E8D57u, c2, lo1, hi1);
    c0 = philox_xor3(hi1, c1, k0); c1 = lo1; c2 = philox_xor3(hi0, c3, k1); c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  constexpr float k2m32 = 2.3283064365386963e-10f;
  const unsigned ca = half ? c2 : c0, cb = half ? c3 : c1;
  const float ua = ((float)ca + 0.5f) * k2m32, ub = ((float)cb + 0.5f) * k2m32;
  const float r = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(ua));
  return make_float2(r * __builtin_amdgcn_cosf(ub), r * __builtin_amdgcn_sinf(ub));
}
// The four uniforms of the same block (same ten rounds, same counter layout):
// u = (c + 0.5) * 2^-32, the pixel draws of iwae_generate (uniform q of group
// g is the draw of column 4g + q).
__device__ __forceinline__ float4 philox_uniform4(uint64_t seed, uint64_t base, unsigned row, unsigned layer,
                                                  unsigned grp) {
  unsigned c0 = row, c1 = (layer << 20) | grp, c2 = (unsigned)base, c3 = (unsigned)(base >> 32);
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    unsigned lo0, hi0, lo1, hi1;
    philox_mul(0xD2511F53u, c0, lo0, hi0);
    philox_mul(0xCD9E8D57u, c2, lo1, hi1);
    c0 = philox_xor3(hi1, c1, k0); c1 = lo1; c2 = philox_xor3(hi0, c3, k1); c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  constexpr float k2m32 = 2.3283064365386963e-10f;
  return make_float4(((float)c0 + 0.5f) * k2m32, ((float)c1 + 0.5f) * k2m32, ((float)c2 + 0.5f) * k2m32,
                     ((float)c3 + 0.5f) * k2m32);
}
// The four uniforms of pixel columns 4g .. 4g + 3 of row r: the caller's [rows][xdim] buffer (columns
// past xdim repeat the last), else Philox (row, layer, group g) -- the one pixel layout of gen_kernel,
// gen_pixels_kernel and impute_draw_kernel.
__device__ __forceinline__ float4 pixel_uniform4(const float* __restrict__ u, int r, int g, int xdim, uint64_t seed,
                                                 const uint64_t* rng_base, int layer) {
  if (u) {
    const float* s = u + (size_t)r * xdim;
    const int j = 4 * g;
    return make_float4(s[j], s[min(j + 1, xdim - 1)], s[min(j + 2, xdim - 1)], s[min(j + 3, xdim - 1)]);
  }
  return philox_uniform4(seed, *rng_base, (unsigned)r, (unsigned)layer, (unsigned)g);
}
__device__ __forceinline__ float f4_at(const float4& v, int q) {
  return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
}

// ------------------------------------------------- unconditional loads ----
// Loads that may fall outside a tile are issued through a buffer resource with
// a per-lane byte offset; an invalid lane gets offset kOOB, which the hardware
// range check turns into a 0 -- no exec-masked branch around the load (hipcc
// turns `cond ? load : 0` into a branch + vmcnt(0) wait per load, i.e. one
// dependent memory round trip per element).  The base must be wave-uniform
// (made provable with readfirstlane); valid offsets stay below 2 GiB.
constexpr unsigned kOOB = 0x7FFFFFF0u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes = kOOB) {
  const uint64_t a = (uint64_t)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
  const uint64_t u = ((uint64_t)hi << 32) | lo;
  return __builtin_amdgcn_make_buffer_rsrc((void*)u, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ float bld1(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ float4 bld4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// TFP Normal(loc, s).log_prob(h) = -0.5 (h/s - loc/s)^2 - (0.5 log 2pi + log s)
__device__ __forceinline__ float normal_logp(float h, float mu, float sc) {
  const float rs = frcp(sc);
  const float z = h * rs - mu * rs;
  return -0.5f * (z * z) - (kHalfLog2Pi + flog(sc));
}

// ---------------------------------------------------------------- GEMM ----
enum GemmKind { GEMM_FWD = 0, GEMM_BWD_DATA = 1, GEMM_BWD_WEIGHT = 2 };
// EPI_BERN_MASK: EPI_BERN over a pixel-masked image (aux < 0 marks a missing
// pixel: its log-probability, Keras-BCE term and g are selected to 0)
enum GemmEpi { EPI_STORE = 0, EPI_TANH = 1, EPI_BERN = 2, EPI_TANH_GRAD = 3, EPI_BERN_MASK = 4 };

struct GemmArgs {
  const float* A; const float* B; float* C;
  int lda, ldb, ldc;
  int M, N, K;
  int kchunk;                 // K range per blockIdx.z (multiple of 64)
  long long c_split_stride;   // C offset per blockIdx.z (split-K slabs)
  const float* aux; int ldaux;  // TANH_GRAD: Y (tanh output); BERN: x_in; BERN_MASK: mask ? x : -1
  const float* rowscale;      // STORE/TANH_GRAD: C[m][:] *= rowscale[m]
  const float* kscale;        // BWD_WEIGHT: B[k][:] *= kscale[k]
  float* part; float* part2; int ldpart;  // BERN: per-32-column row partials
  int x_row_div;              // BERN: x row = m / x_row_div
  float wa, wb;               // BERN: g = (wa*dTFP + wb*dBCE) * dp/dlogit
  int store_g;                // BERN: write g into C
  int need_bce;               // BERN: write Keras-BCE partials into part2
  int x3;                     // 1: bf16x3 products on v_mfma_f32_32x32x16_bf16 (else exact f32 MFMA)
  const __bf16* Bhi; const __bf16* Blo; int ldbx;   // x3: pre-split B as [n][ldbx] (k contiguous), else null
  // f32, A not transposed: A is the caller's rows of a_ones floats (lda =
  // a_ones, a multiple of 4) and column a_ones is a virtual ones column (the
  // bias row of W_aug); the column-0 workgroups also copy A into a_copy
  int a_ones; float* a_copy; int a_copy_ld;
};

// tile: 0 = 64x64 (4 waves), 1 = 128x128 (4 waves, 2x2 MFMA tiles each)
hipError_t launch_gemm(hipStream_t st, GemmKind kind, GemmEpi epi, int tile, int splits,
                       bool kscale, const GemmArgs& a);

// Few-row Dense layer (M <= 32 rows: the per-image first encoder layer of a
// small batch): C[M][N] = act(A[M][K] . B).  One workgroup per 16-column tile
// (N-split, so the K x N weights are streamed once over many CUs), its 8 waves
// split K, partial tiles summed through LDS; exact f32 MFMA.
//   bt = 0: B(k,n) = W[k*ldw + n]  (forward, W_aug = [W; b], K = fin + 1)
//   bt = 1: B(k,n) = W[n*ldw + k]  (backward dX = dZ W^T, K = fout, N = fin)
//   act: 0 store, 1 tanh, 2 times (1 - Y^2)
struct SmArgs {
  const float* A; int lda;
  const float* W; int ldw; int bt;
  float* C; int ldc;
  int M, N, K;
  int act; const float* Y; int ldy;
  // split K over kslabs workgroup columns (blockIdx.y): partial sums into slabs
  // C + ks * c_slab (no activation; the reader sums them)
  int kslabs; long long c_slab;
  // A given as a_slabs partial slabs of a pre-activation: staged as
  // tanh(sum) (a_act) with the ones column at K - 1, and written once to a_out
  int a_slabs; long long a_slab; int a_act; float* a_out; int a_ldo;
  // A read straight from the caller's rows (no ones column): column a_ones (> 0)
  // reads 1, later ones 0 (0: off); a_bytes bounds the reads (0: unbounded);
  // workgroups of column tile 0 also store the staged rows (ones column
  // included) to a_copy for the later readers of A
  int a_ones; unsigned a_bytes; float* a_copy; int a_copy_ld;
};
hipError_t launch_smallm(hipStream_t st, const SmArgs& a);
hipError_t smallm_setup_attributes();

// grouped backward-weight GEMMs (64x64 tiles, split over K = rows)
constexpr int kMaxGroup = 16;
struct GemmGroup {
  GemmArgs g[kMaxGroup];
  int splits[kMaxGroup];
  int start[kMaxGroup + 1];
  int tiles_x[kMaxGroup], tiles_y[kMaxGroup];
  int n;
};
hipError_t launch_gemm_group_bwd_weight(hipStream_t st, GemmGroup& gg);

// ------------------------------------------------------------ Gaussians ----
struct GaussArgs {
  const float* P; int ldP; int prow_div;   // head output rows (mu | zs), row = r / prow_div
  int d;
  float* H; int ldH;                        // sampled / evaluated h
  const float* eps_a; const float* eps_b;   // injected noise (sample-major [k][Bg][d]) or null
  int kS, Bsplit, Bimg;                     // samples per image, images in group a, total images
  uint64_t seed; const uint64_t* rng_base; int layer;
  float* out; int accumulate;               // per-row log density (set or +=)
  float* eps_out; int ld_eps_out;           // mode 0: keep the noise for the backward pass
  int M;
  const float* mask;                        // mode 0: h *= mask[j] before log q (F:501-F:511), or null
};
// mode 0: sample h = eps*scale+mu and log N(h; mu, scale)   (Encoder.call F:58-F:70)
// mode 1: log N(h; mu, scale) of a given h                   (Decoder.get_log_ph F:139-F:140)
// mode 2: log N(h; 0, 1)                                      (F:135-F:136)
hipError_t launch_gauss_fwd(hipStream_t st, int mode, const GaussArgs& a);

// Which partials of log q(h | .) with h = eps*s + mu an encoder Gaussian
// backward puts into (dmu, dsc), per row with dht = dL/dh + dlq * (-z/s):
//   GM_TOTAL    dmu = dht + dlq z/s,  dsc = dht eps + dlq (z^2 - 1)/s   (GradientTape)
//   GM_PATH     dmu = dht,            dsc = dht eps    (through the sample only: STL / DReG)
//   GM_DENSITY  dmu = dlq z/s,        dsc = dlq (z^2 - 1)/s   (through (mu, s) only; no dL/dh
//               sources: the chain below it yields the density's dL/dh of the layer underneath)
//   GM_FIT      the density partials of the loss -a log q(h | .) at fixed h, a = the row's weight
//               read where the other modes read dL/dlw: dmu = -a z/s, dsc = -a (z^2 - 1)/s.  No
//               dL/dh sources, no eps, no dX below (the latent a layer reads is data); also on the
//               first encoder layer (reduced over an image's rows).  iwae_wake_sleep_step's mode.
enum GradMode { GM_TOTAL = 0, GM_PATH = 1, GM_DENSITY = 2, GM_FIT = 3 };

struct GaussBwdArgs {
  const float* P; int ldP; int prow_div; int d;
  const float* H; int ldH;
  const float* eps_rows; int ld_eps;        // noise stored by the forward pass, [M][ld_eps]
  const float* src[4]; int ldsrc[4]; int nsrc;   // dL/dh contributions (dX outputs)
  int std_normal;            // this h is h_L: add dL/dlogp * (-h)
  const float* dlw;          // dL/dlw per row (dL/dlogp = dlw, dL/dlogq = -dlw)
  float kl_coef; int kl_rows;  // VAE_V1: dL/dKLmean on this head (0 = none)
  float* dP; int lddP;       // (dmu | dzs) per P row
  float* dh_out; int ldh_out;  // prior mode: dL/dh of the target
  int M;                     // rows of H
  int grad_mode;             // encoder mode: GM_TOTAL (0), GM_PATH, GM_DENSITY or GM_FIT
  int nk_img;                // GM_FIT, prow_div > 1: P rows from nk_img on own ONE row of H each, behind the
                             // nk_img * prow_div rows of the first nk_img (the dream rows); 0: every P row owns prow_div
};
// P rows of an encoder Gaussian backward over M rows of H
__host__ __device__ inline int gauss_bwd_prows(const GaussBwdArgs& a) {
  if (a.nk_img > 0) return a.nk_img + (a.M - a.nk_img * a.prow_div);
  return (a.M + a.prow_div - 1) / a.prow_div;
}
// mode 0: backward of an encoder sampling layer -> dP (reduced over prow_div rows)
// mode 1: backward of a decoder prior head      -> dP (per row) and dh_out
hipError_t launch_gauss_bwd(hipStream_t st, int mode, const GaussBwdArgs& a);

// ------------------------------------------------------ wake-sleep step ----
// Dream rows into the workspace (iwae_wake_sleep_step): buffer q's n rows of
// width[q] floats from src[q] (row stride ld_src[q]) to dst[q] (row stride
// ld_dst[q]); the ones column and the padding of the destination rows stay.
struct WsStageArgs {
  const float* src[9]; float* dst[9];
  int width[9], ld_src[9], ld_dst[9];
  int n, nbuf;
};
hipError_t launch_ws_stage(hipStream_t st, const WsStageArgs& a);
// Row weights of the GM_FIT backward: w[r] = -c_wake dlw[r] on the wake rows
// r < M (c_wake softmax / B; not written, dlw not read, when c_wake == 0),
// w[M + j] = a_sleep on the n dream rows.
hipError_t launch_ws_weights(hipStream_t st, const float* dlw, float* w, int M, int n, float c_wake, float a_sleep);
// values[0] = sum_{r < M} dlw[r] logq[r]  (L_wake; 0 when !wake),
// values[1] = -(1/n) sum_j logq[M + j]    (L_sleep; 0 when n == 0):
// one workgroup, fixed summation order, no atomics.
hipError_t launch_ws_values(hipStream_t st, const float* dlw, const float* logq, int M, int n, int wake,
                            float* values);

// --------------------------------------------------------------- bounds ----
// BM_SM2: value as BM_IWAE, row weights the squared softmax (e/se)^2 (DReG's encoder weighting)
enum BoundMode { BM_VAE = 0, BM_IWAE = 1, BM_POWER = 2, BM_MEDIAN = 3, BM_MIWAE = 4, BM_NONE = 5, BM_SM2 = 6 };

struct BoundArgs {
  const float* part; const float* part2; int ldpart, npart;
  const float* logp; const float* logq;
  float* lw; float* contrib;
  float* dlw; float* dpx;               // may be null (no backward)
  float* dlw2; float* dpx2;             // PIWAE second weighting (encoder), may be null
  int kS, Bimg, Bsplit;
  int mode_a; float w_a; int mode_b; float w_b;
  int mode2;                            // weighting of dlw2 (PIWAE: MIWAE; DReG: BM_SM2)
  float p; int k1, k2;
  float bce_w;                          // objective += bce_w * mean_s(bce row) / Bg
  float dpx_const; int dpx_is_const;    // dpx = dpx_const instead of dlw
  float* loss; float loss_sign;         // last block: *loss = loss_sign * sum(contrib) + loss_add
  const float* loss_add;                // optional device scalar (VAE_V1 KL) ...
  float loss_add_coef;                  // ... added as loss_add_coef * (*loss_add)
  unsigned* ticket; uint64_t* rng_base; // last-block bookkeeping
  long long* adam_step;                 // train step with Adam: advance the step counter (or null)
};
hipError_t launch_bound(hipStream_t st, const BoundArgs& a);
int bound_grid(const BoundArgs& a);    // its workgroups

// ------------------------------------------ thermodynamic variational objective
// tvo_kernel (iwae_tvo.hip): per image, over its kS log
// weights and the partition beta[0 .. J] (beta[0] = 0 < ... < beta[J] = 1), with
// D_j = beta[j + 1] - beta[j], wn^(j) = softmax_s(beta[j] lw_s) and
// m_j = sum_s wn^(j)_s lw_s:
//   lower = sum_{j<J} D_j m_j,  upper = sum_{j<J} D_j m_{j+1},
//   iwae  = logsumexp_s lw_s - log kS,
//   a_theta_s = sum_{j<J} D_j wn^(j)_s [1 + beta[j] (lw_s - m_j)],
//   a_phi_s   = sum_{j<J} D_j wn^(j)_s [(1 - beta[j]) (lw_s - m_j) - 1].
// One wave per image, bound_kernel's discipline: fixed butterflies over lanes,
// a lane's samples in sample order, j ascending; no float atomics, one writer
// per element.  An image with a NaN or an infinity among its log weights gets
// NaN in every output of its own, and in the batch values it is summed into.
constexpr int kTvoMaxPart = 64;
struct TvoArgs {
  // the log weights: lw_in [Bimg][kS] when given, else composed per row as
  // bound_kernel does from logp / the Bernoulli partials / logq and stored to lw_out
  const float* lw_in;
  const float* part; int ldpart, npart; const float* logp; const float* logq;
  float* lw_out;
  int kS, Bimg, J;
  float beta[kTvoMaxPart + 1];
  float* a_theta; float* a_theta2; float s_theta;   // s_theta a_theta per row, to both (each may be null)
  float* a_phi; float s_phi;                        // s_phi a_phi per row (may be null)
  float* lower; float* upper; float* iwae;          // per image (each may be null; all three given with `values`)
  // step mode (values != null): values[0 .. 2] = -(1/Bimg) sum_b (lower, upper,
  // iwae), the advance of the noise position and Adam's tick, as bound_finalize
  float* values;
  unsigned* ticket; uint64_t* rng_base; long long* adam_step;
};
hipError_t launch_tvo(hipStream_t st, const TvoArgs& a);
int tvo_grid(const TvoArgs& a);        // its workgroups (bound_grid's rule)

// per-image LSE over this chunk's rows merged into running (m, s)
struct LseArgs {
  const float* part; int ldpart, npart; const float* logp; const float* logq;
  const float* lw;             // if set: log w per row directly (fused forward), part/logp/logq unused
  int kS, Bimg;
  float* run_m; float* run_s; int init;
  unsigned* ticket; uint64_t* rng_base;
};
hipError_t launch_lse(hipStream_t st, const LseArgs& a);
hipError_t launch_lse_final(hipStream_t st, const float* m, const float* s, int n, float logk,
                            float* out);

// VAE_V1 analytic KL: value (mean over rows of sum_d KL) into *out
hipError_t launch_kl_v1(hipStream_t st, const float* P, int ldP, int d, int rows, float* out);

// ----------------------------------------------------------------- Adam ----
struct AdamSeg {
  long long off, n;        // parameter range in the flat internal buffer
  long long slab_off;      // offset of this segment's slabs in the slab arena
  int splits;              // number of slabs (0 = read grad buffer)
  int fin, fout, ldw;      // the Dense layer (W_aug [fin+1][ldw])
  long long f_off, g_off;  // its split copies F / G (see WSplitSeg)
  int ldF, ldG;
};
struct AdamState {         // device resident (graph-replay safe)
  float lr, b1, b2, eps;
  float grad_scale; int pad0;
  long long t;             // Adam steps, advanced BEFORE the step's Adam launch reads it
};
constexpr int kMaxSegs = 64;
struct AdamArgs {
  float* param; float* m; float* v; float* grad; const float* slabs;
  __bf16* whi; __bf16* wlo;    // split weight copies refreshed with every update
  AdamSeg seg[kMaxSegs]; int nseg;
  int write_grad, do_adam, read_slabs;
  AdamState* state; unsigned* ticket;
  float grad_scale_override;   // >0: use this instead of state->grad_scale
  const float* scale_dev;      // data parallel: scale = 1 / *scale_dev (the all-reduced batch total), or null
  float* tail; float tail_val; // data parallel write pass: *tail = tail_val (this rank's batch size), or null
  int tick;                    // advance state->t in a tick kernel first (else the bound kernel did)
};
hipError_t launch_adam(hipStream_t st, const AdamArgs& a, long long max_seg_n);
hipError_t launch_grad_moments(hipStream_t st, const float* g, float* s, float* s2, long long n);

// ------------------------------------------------------ split weights ----
// bf16x3 products a.b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi (hi = bf16(x),
// lo = bf16(x - hi), f32 accumulate).  Every Dense layer keeps two split
// copies of W_aug, both k-contiguous so an MFMA B operand row is a straight
// copy into LDS (no transposition, no conversion):
//   F [fout][ldF]  F[j][i] = W_aug[i][j]   forward   (k = fin+1 incl. the bias row)
//   G [fin][ldG]   G[i][j] = W[i][j]       backward  (dX = dZ W^T, k = fout)
// ldF / ldG are multiples of 32; the padding stays zero.  The Adam kernel
// rewrites them with every update; wsplit_kernel after iwae_set_params.
struct WSplitSeg {
  long long off; int fin, fout, ldw;
  long long f_off, g_off; int ldF, ldG;
};
struct WSplitArgs {
  const float* param; __bf16* hi; __bf16* lo;
  WSplitSeg seg[kMaxSegs]; int nseg;
};
hipError_t launch_wsplit(hipStream_t st, const WSplitArgs& a, long long max_seg_elems);

// Fragment-major split copies (bf16 hi / lo planes) for the kernels that take
// the weights as the MFMA A operand of v_mfma_f32_16x16x32_bf16 (the row-chain
// train engine; iwae_train.hip): per Dense layer and direction, the 16-row x
// 32-k fragment of tile t, k step u is stored as 64 lanes x 8 bf16 contiguous
// (lane l holds row 16t + (l & 15), k = 32u + 8(l >> 4) .. +7), so one
// buffer_load_dwordx4 per plane reads 1 KiB of consecutive memory (the plain
// row-major copies touch 16 half-used lines per load).
//   FX (forward):  rows = output features (a head's rows permuted into groups
//                  of 8, [mu 4q..4q+3 | zs 4q..4q+3], when head_d > 0),
//                  k = fin + 1 (the bias row last);
//   GX (backward): rows = input features, k = fout.
struct FxSeg {
  long long off; int fin, fout, ldw;           // W_aug [fin+1][ldw] in the parameters
  long long fx_off; int fx_tiles, fx_steps, head_d;
  long long gx_off; int gx_tiles, gx_steps;
  long long start;                             // first 8-value chunk of this segment in the launch
};
struct FxArgs {
  const float* param; __bf16* hi; __bf16* lo;
  FxSeg seg[kMaxSegs]; int nseg;
  long long total;                             // chunks
};
hipError_t launch_fx_refresh(hipStream_t st, const FxArgs& a);

// Fused train-step update (iwae_update.hip): per Dense layer, dW_aug = X_aug^T
// dZ over all the step's rows in 64 x 64 tiles (bf16x3, no split-K slabs), the
// gradient buffer, Keras Adam and the FX / GX copies of the updated tile.
struct UpdJob {
  const float* A; const float* B; const float* ks;   // X_aug [rows][lda] (ones column at fin), dZ [rows][ldb], dZ row scale (>= rows floats)
  int lda, ldb, rows;
  long long off; int fin, fout, ldw;                  // W_aug [fin+1][ldw] at param + off
  long long fx_off; int fx_steps, head_d;             // FX copy (fx_off < 0: none, GX neither)
  long long gx_off; int gx_steps;
  int tiles_m, tiles_n, tile0;                        // tiles [tile0, tile0 + tiles_m * tiles_n), column-major
  int tn;                                             // tile columns: 64, or 32
  // split-K over rows (large batches, gradient pass only): nsplit row chunks of
  // `chunk` rows, split s writes its partial W_aug tile at off + s * slab_stride
  // (the Adam launch sums the slabs); the job's tiles are then split-major
  int nsplit, chunk; long long slab_stride;
  // (apply mode 2: B = the job's slab arena, chunk = its slab count, slab_stride between slabs)
};
constexpr int kUpdMaxJobs = 20, kUpdMaxTiles = 384;
struct UpdArgs {
  UpdJob job[kUpdMaxJobs]; int njobs;
  unsigned char tile_job[kUpdMaxTiles];               // job of each tile
  int ntiles, nheavy, per_xcd, per_xcd2;              // tiles [0, nheavy): per_xcd per XCD, the rest per_xcd2 per XCD
  int search;                                         // more than kUpdMaxTiles tiles: job of a tile by the jobs' tile0
  float* param; float* m; float* v; float* grad;
  __bf16* fx_hi; __bf16* fx_lo;
  const AdamState* state; int do_adam;
  float gscale;                                       // gradient written as gscale * dW (data parallel: B_local)
  float* tail; float tail_val;                        // data parallel: *tail = tail_val (B_local), or null
  // apply mode (data parallel, after the all-reduce): no reduction; the tile's
  // gradient is read from grad, scaled by 1 / *scale_dev (or gscale), written
  // back, then Adam and the FX / GX copies as usual
  int apply; const float* scale_dev;
  int waves;                                          // 4, or 8 (64-column tiles: two waves per SIMD)
  // store policy (iwae_set_store_policy; the fused / combined routes only), kUpdSt* bits:
  // the grad, m, v, param, FX and GX stores of the sample-row ("heavy": more than
  // one reduction iteration) or one-iteration ("light") tiles write-through (sc1);
  // a heavy tile's workgroup writes its XCD's L2 back as its last act
  int st_wt;
};
constexpr int kUpdStHeavy = 1, kUpdStLight = 2, kUpdStRelease = 4;
hipError_t launch_update(hipStream_t st, const UpdArgs& a);
constexpr int kUpdRowsPerIter = 128;     // rows per reduction iteration of the update kernel (UP_RI)
// in-launch wait of the update's first-encoder-layer tiles on the image-row
// backward workgroups of tcu_kernel (iwae_update_dev.h, upd_wait)
struct UpdWait {
  unsigned* ctr;              // [0] producers done, [1] workgroups through (producers and consumers), [2] give-ups
  unsigned* err;              // host-mapped error word: set to 1 by a wait that gave up (iwae_status reports it)
  unsigned wait_mask;         // jobs whose tiles wait
  int n_prod, n_cons;
  int n_expect;               // ctr[0] a wait waits for (n_prod; n_prod + 1 under the fault-injection knob)
  unsigned max_spins;         // spin bound of a wait (s_sleep 1 per spin)
  int wt;                     // write-through hand-off: the producers store every handed-off byte sc1 and add to
                              // the counter with no release fence; the waiting tiles load dZ sc1 with no acquire
                              // (MI355X_MICROARCH.md, valid forms, first table row); set by launch_tcu
};
hipError_t upd_setup_attributes();
size_t upd_lds_bytes();             // dynamic LDS of an update workgroup

// Large-batch weight gradients into split-K slabs (iwae_dwgrad.hip): per layer,
// workgroup blocks of 7 x 16 W_aug rows by 8 * nb x 16 columns over a row chunk.
struct DwJob {
  const float* A; const float* B; const float* ks;   // X_aug [rows][lda] (ones column at fin), dZ [rows][ldb], dZ row scale
  int lda, ldb, rows;
  float* out; int ldo; long long slab_stride;        // slab s at out + s * slab_stride: [M][ldo]
  int M, N, mt, nt;                                  // M = fin + 1, N = fout; 16-tiles along M / N
  int mtb, ntb, nib, njb;                            // tiles per block (<= 13 x 8, or wide: <= 8 x 16), blocks along M / N
  int wide;                                          // 1: wide blocks (waves 4 x 2)
  int scaled;                                        // dZ rows carry a scale (ks: the output layer's dpx)
  int nsplit, chunk;                                 // row chunks (chunk % 32 == 0)
  int item0;                                         // first work item of the job (chunk-major, then N, then M block)
};
constexpr int kDwMaxJobs = 20;
struct DwArgs {
  DwJob job[kDwMaxJobs]; int njobs, nitems, per_xcd;
};
hipError_t launch_dw(hipStream_t st, const DwArgs& a);
hipError_t dw_setup_attributes();

// ------------------------------------------------- fused row-block kernels ----
struct RbNoise {             // where a sampling layer's eps comes from (see eps_at)
  const float* eps_a; const float* eps_b;
  int kS, Bsplit, Bimg;
  uint64_t seed; int layer;
};
// Width the LDS operand of a row-block stage is zero-padded to (= the k range
// its register-resident weight fetch covers): 32/64/128/256, then 64-multiples.
__host__ __device__ inline int rb_k_pad(int K, bool bt) {
  if (!bt && K <= 32) return 32;
  if (K <= 64) return 64;
  if (K <= 128) return 128;
  if (K <= 256) return 256;
  return (K + 63) & ~63;
}

struct RbStage {             // one Dense layer of a chain
  const float* W; int ldw;   // W_aug [fin+1][ldw]
  unsigned W_bytes;          // readable bytes from W to the end of the (zero-slacked) allocation
  int K, N;                  // fwd: K = fin+1, N = fout; bwd: K = fout, N = fin
  int act;                   // 0 none, 1 tanh, 2 tanh-grad (times 1 - y^2)
  float* out_g; int ld_out;  // global copy of the stage output (rows of the job)
  const float* y; int ldy;   // act 2: forward tanh output on the input side
};
constexpr int kRbMaxJobs = 4;
struct RbFwdJob {
  int rows, rpb;
  const float* in; int ld_in;                  // input rows (with ones column) unless sampled
  int pro_sample;                              // input h = eps*scale + mu of ps_P[row / ps_div]
  const float* ps_P; int ps_ldP, ps_div, ps_d;
  float* ps_h; int ps_ldh; float* ps_eps; int ps_ldeps; RbNoise ps_noise;
  int pro_stdnormal;                           // log N(input h; 0, 1) into log p
  const float* pr_slabs; int pr_nslab, pr_ld, pr_H; long long pr_stride;  // input = tanh(sum of split-K slabs)
  float* pr_y; int pr_ldy;                     // ... also stored as the layer's y1
  int nst; RbStage st[3];
  int epi;                                     // 0 none, 1 encoder sample, 2 decoder prior
  int ep_d; RbNoise ep_noise;
  float* ep_h; int ep_ldh; float* ep_eps; int ep_ldeps;
  const float* ep_tgt; int ep_ldtgt;
  float* logq; int logq_acc; float* logp; int logp_acc;
};
struct RbFwdLaunch {
  RbFwdJob job[kRbMaxJobs];
  int block_start[kRbMaxJobs + 1];
  int njobs, ld_lds;
  const uint64_t* rng_base;
};
struct RbBwdJob {
  int rows, rpb;
  int pro;                   // 0 load dZ; 1 encoder sampling bwd; 2 decoder prior bwd; 3 encoder layer 0 (per image)
  const float* dz_in; int ld_dz_in;          // pro 0: dZ = sum of dz_nslab slabs dz_stride floats apart
  int dz_nslab; long long dz_stride;
  float* dz_out;                                 // slab mode: the summed dZ is also stored here (weight grads)
  const float* P; int ldP; int d;
  const float* H; int ldH; const float* eps; int ld_eps; const float* dlw;
  const float* src[4]; int ldsrc[4]; int nsrc;
  int std_normal; float kl_coef; int kl_rows; int kS;
  float* dP_out; int ld_dP; float* dh_out; int ld_dh;   // (pro 1: dP_out may be null -- a dX-only density job)
  int nst; RbStage st[3];
  int gmode;                 // pro 1 / 3: GradMode of the sampling layer's partials
  int nk_img;                // pro 3, GM_FIT: images from nk_img on own ONE row each, behind the nk_img * kS rows
                             // of the first nk_img (the dream rows); 0: every image owns kS rows
};
struct RbBwdLaunch {
  RbBwdJob job[kRbMaxJobs];
  int block_start[kRbMaxJobs + 1];
  int njobs, ld_lds;
};
hipError_t launch_rb_fwd(hipStream_t st, RbFwdLaunch& L);
hipError_t launch_rb_bwd(hipStream_t st, RbBwdLaunch& L);
hipError_t rb_setup_attributes();

// ------------------------------------------- fused k-sample forward (NLL) ----
// One workgroup owns MG_ROWS(RT) = 16*RT sample rows and runs the whole model
// after the first encoder layer on them, activations resident in LDS: sample
// h1 from the image's (mu, scale), every later stochastic layer, the decoder
// prior, the output MLP and the Bernoulli log-likelihood; it writes only the
// log weight of each row.  Matrix products: bf16x3 on v_mfma_f32_16x16x32_bf16
// with the layers' pre-split F copies streamed from L2 into registers.
constexpr int kMgMaxStages = 24;
constexpr int kMgMaxBufs = 12;
// Stage kinds.  A head stage (SAMPLE / PRIOR) computes the (mu | zs) outputs
// of a stochastic layer with its weight rows permuted into groups of 8 --
// [mu 4q..4q+3 | zs 4q..4q+3] -- so the lanes holding mu_j and zs_j are 16
// apart and the sampling / prior density runs in the MFMA epilogue.
enum MgAct { MG_NONE = 0, MG_TANH = 1, MG_BERN = 2, MG_SAMPLE = 3, MG_PRIOR = 4 };
struct MgStage {
  const __bf16* Whi; const __bf16* Wlo; unsigned W_bytes;
  int ldk, K, N;             // F [rows][ldk]; K = fin + 1 (input ones column at K - 1);
                             // N = output features (head stages: 8 * ceil(d / 4) permuted)
  int in_buf, out_buf;       // LDS buffer ids; out_buf: TANH output, SAMPLE destination h_i,
                             // PRIOR target h_t (read)
  int act;                   // MgAct
  int d, layer, stdnormal;   // head stages: latent width, Philox layer, add log N(h; 0, 1)
  int next_k;                // TANH / SAMPLE: padded K of the reader of out_buf (ones column + zero pad)
};
struct MgLaunch {
  MgStage st[kMgMaxStages]; int nst;
  int buf_off[kMgMaxBufs], buf_ld[kMgMaxBufs];   // float offsets / row strides in LDS
  int acc_off;                                    // LDS: logq, logp, logpx [rows] + reduction scratch
  int rows, kS;                                   // sample rows in this chunk, samples per image
  const float* P0; int ldP0; int d0; int h0_buf; int h0_next_k; int h0_stdnormal;   // prologue sampling
  const float* x; int ldx;                        // pixels [images][ldx]
  uint64_t seed; const uint64_t* rng_base;
  // injected noise (parity: iwae_nll_eps) instead of Philox: eps[i] is layer i's
  // [k][eps_N][d_i] buffer in the reference's sample-major layout (F:59, F:68);
  // chunk row r is sample eps_s0 + r % kS of image eps_i0 + r / kS.  Null: Philox.
  const float* eps[8]; int eps_N, eps_i0, eps_s0;
  float* lw;                                      // out: log w per row
};
hipError_t launch_mega_fwd(hipStream_t st, const MgLaunch& L, int rt, int waves, size_t lds_bytes);
// The pixel-masked variant (iwae_impute): L.x is the staged copy with -1 at the missing pixels
hipError_t launch_mega_fwd_masked(hipStream_t st, const MgLaunch& L, int rt, int waves, size_t lds_bytes);
hipError_t mega_setup_attributes();

// ------------------------ densities of caller-supplied latents (iwae_score) ----
// score_kernel (iwae_score.hip): mega_fwd_kernel's pipeline with every latent
// given.  The prologue loads the h_i tiles the stage list reads from the
// caller's [k][N][d_i] buffers into their LDS buffers (hi / lo planes, ones
// column, zero padding); every head is a density head -- encoder heads
// (MG_DENSQ) add log N(h_i; enc_{i-1}(h_{i-1})) to the row's log q, prior heads
// (MG_DENSP) add log N(h_t; dec_j(.)) to its log p(h) -- whose target is the
// caller's f32 value, read from memory (the split LDS copy feeds the matrix
// products only); the output stage (MG_BERNS) adds the Bernoulli terms to
// log p(x|h) and / or stores the probabilities from its accumulators.  The
// three sums are stored separately.  The 2 L chains are independent, so the
// stage list holds only the chains of the outputs asked for, the first prior
// chain ahead of the encoder's (it reads h_L from the scratch buffer the
// encoder chains write).  Stage fields: MgStage's, with layer = the target
// latent's index for the density heads.  The base's eps / eps_N / eps_i0 are
// the latents and their addressing (eps_s0 = 0), lw is unused.
enum ScAct { MG_DENSQ = 5, MG_DENSP = 6, MG_BERNS = 7 };
struct ScLaunch : MgLaunch {
  int n_lat;                         // stochastic layers
  int lat_d[8], lat_buf[8];          // latent widths; LDS buffer of h_i's tile, -1: no stage reads it
  int lat_next_k[8];                 // padded K of the tile's readers
  int want_q, want_ph;               // prologue: log N(h_1; P0) into log q / log N(h_L; 0, 1) into log p(h)
  float* log_q; float* log_ph; float* log_px;   // out: [rows] each, or null
  float* probs; int ld_probs;        // out: p(h_1) of the rows [rows][ld_probs], or null
};
hipError_t launch_score(hipStream_t st, const ScLaunch& L, int rt, int waves, size_t lds_bytes);
// The pixel-masked variant (iwae_score_masked): L.x is the staged copy with -1 at the missing pixels
hipError_t launch_score_masked(hipStream_t st, const ScLaunch& L, int rt, int waves, size_t lds_bytes);
hipError_t score_setup_attributes();

// Relayouts between the callers' sample-major [k][N][d] buffers and the
// workspace's image-major rows (iwae_score.hip).  Segment g, for b < n, s < k,
// j < d: gather: rows[(b k + s) ld + j] = ext[((s N) + i0 + b) d + j]; else
// ext[...] = f(rows[(b k + s) ld + col0 + j]), f the identity or (expo)
// exp(.) + 1e-6 (a head's scale).  img: the rows are image rows, ext is [N][d]:
// ext[(i0 + b) d + j] = f(rows[b ld + col0 + j]).
struct ScSeg { float* rows; int ld, col0, d; float* ext; int expo, img; };
struct ScRelayout {
  ScSeg seg[2 * 8 + 2]; int nseg;
  int n, k, N, i0, gather;
};
hipError_t launch_score_relayout(hipStream_t st, const ScRelayout& a);
// out[r] = the row's Bernoulli partial sums in column order (forward_core's row sum), r < rows
hipError_t launch_score_rowsum(hipStream_t st, const float* part, int ldpart, int npart, int rows, float* out);

// iwae_score_grad's layer-wise path (iwae_scoregrad.hip).  SgDens: a Gaussian
// head's gradients at the given target H (workspace rows), with z = (t - mu) / s
// and s = exp(zs) + 1e-6: tg[r][j] = -z / s (with respect to the target) and,
// when dP is set, dP[r] = (z / s | (z^2 - 1) (s - 1e-6) / s) (into the head's
// outputs); the head's row of P is r / prow_div.
struct SgDens {
  const float* P; int ldP, prow_div, d;
  const float* H; int ldH;
  float* tg; int ldtg;
  float* dP; int lddP;
  int M;
};
hipError_t launch_sg_dens(hipStream_t st, const SgDens& a);
// SgScatter: layer g's out[((s N) + i0 + b) d + j] = sum_q c[q] src[q][(b k + s) ld[q] + j]
// - c_top lat[...] (c_top: c_ph on the top layer, the gradient of log N(h_L; 0, 1)),
// the sources added in their listed order; b < n, s < k, j < d.
constexpr int kSgMaxSrc = 5;
struct SgLayer {
  const float* src[kSgMaxSrc]; int ld[kSgMaxSrc]; float c[kSgMaxSrc]; int nsrc;
  float c_top; const float* lat;
  float* out; int d;
};
struct SgScatter {
  SgLayer lay[8]; int nlay;
  int n, k, N, i0;
};
hipError_t launch_sg_scatter(hipStream_t st, const SgScatter& a);

// iwae_score_grad's fused path: sg_kernel (iwae_scoregrad.hip), score_kernel's
// rows, prologue and density heads with every chain run forward and straight
// back in LDS.  Buffers (bf16 hi / lo planes): one tile per latent a chain
// reads, A (a chain's y1, then dY1 in place), B (y2, then dY2 in place) and P
// (a head's dP in GX's k order, natural (dmu | dzs); the output chain's dlogit
// slab of 256 pixels).  f32 gradient tiles G_i [rows][g_ld] collect the terms
// in stage order.  Stage kinds:
//   SG_TANH   forward Dense + tanh into out_buf (FX copy)
//   SG_HEADQ / SG_HEADP  density head: the value into log q / log p(h); with
//             c != 0 the target gradient c (-z / s) into G[layer] and c dP into out_buf
//   SG_GTANH  backward-data Dense on the GX copy times (1 - y^2), y read from
//             and the result written to out_buf
//   SG_GX     backward-data Dense on the GX copy added into G[layer]
//   SG_OUT    the output Dense (FX) with the Bernoulli value and c dlogit,
//             fed slab by slab into dY2 = dlogit W3^T (GX, out_gx_*), then
//             times (1 - y2^2) in place in in_buf
enum SgKind { SG_TANH = 0, SG_HEADQ = 1, SG_HEADP = 2, SG_GTANH = 3, SG_GX = 4, SG_OUT = 5 };
constexpr int kSgMaxStages = 48;
constexpr int kSgOutTiles = 4;       // dY2 column tiles a wave may own in SG_OUT
constexpr int kSgWaves = 8;          // waves of an sg_kernel workgroup (MG_WAVES)
struct SgStage {
  unsigned woff;                     // element offset of the stage's FX / GX copy (hi and lo planes alike)
  short ldk, N;                      // padded K; output features (heads: 8 ceil(d / 4) permuted)
  signed char in_buf, out_buf, kind, layer;
  short d, next_k;                   // heads: latent width; padded K of out_buf's reader
  float c;                           // coefficient carried by this stage's gradient (0: value only)
};
struct SgLaunch {
  SgStage st[kSgMaxStages]; int nst;
  const __bf16* fx_hi; const __bf16* fx_lo; long long fx_elems;
  int buf_off[kMgMaxBufs], buf_ld[kMgMaxBufs];   // bf16 offset of the hi plane / row stride
  int g_off[8], g_ld[8];             // float offsets / row strides of the gradient tiles
  int acc_off;                       // floats: logq, logp [rows]
  int out_gx_woff, out_gx_ldk, out_gx_N;
  int rows, kS;
  const float* P0; int ldP0;
  const float* x; int ldx;
  const float* lat[8]; float* grad[8]; int lat_N, lat_i0;
  int n_lat, lat_d[8], lat_buf[8], lat_next_k[8];
  float cq, cph;                     // prologue: c_q T^q_1 (0: no gradient) and -c_ph h_L
  int want_q, want_ph;               // prologue values: log N(h_1; P0), log N(h_L; 0, 1)
  float* log_q; float* log_ph; float* log_px;
};
hipError_t launch_sgrad(hipStream_t st, const SgLaunch& L, int rt, size_t lds_bytes);
// The pixel-masked variant (iwae_score_grad_masked): L.x is the staged copy with -1 at the missing
// pixels; their terms of log p(x|h) and their dlogits are 0
hipError_t launch_sgrad_masked(hipStream_t st, const SgLaunch& L, int rt, size_t lds_bytes);
hipError_t sgrad_setup_attributes();

// ------------------------------- weight-ring k-sample forward (NLL) ----
// nring_kernel (iwae_nring.hip): the same per-row work as mega_fwd_kernel for
// 1- and 2-layer models, activations of 16 rows per wave in registers, the
// weights shared by the workgroup's 8 waves (128 rows) through an LDS ring of
// NR_D slots filled by LDS-DMA from FX, one (column tile, k <= 256) unit per
// slot.  Stage order in st[]: e1, e2, eh (SAMPLE h2), p1, p2, ph (PRIOR of
// h1), o1, o2, ob (Bernoulli); a 1-layer model uses st[6..8] only.
constexpr int NR_D = 8;
constexpr int kNrMaxUnits = 512;
struct NrUnit {
  unsigned off;              // FX byte offset of (column tile, k step 0), both planes
  int ns;                    // k steps of 32 (<= 8); nrb_kernel: pieces | piece stride KiB << 8
};
struct NrStage {
  int ntile, ns, N;          // column tiles, k steps of the input, output features (heads: 8 * ceil(d / 4))
  int d, layer, stdnormal;   // head stages
  int next_ns;               // tanh stages: k steps of the reader (ones column at N, zeros up to it)
  // train mode: the f32 stores (the train engine's TcOp fields of the same op)
  float* out; int ld_out;    // tanh y, head (mu | zs), Bernoulli g
  float* h; int ld_h;        // sampling head: h, eps
  float* eps; int ld_eps;
};
struct NrLaunch {
  const __bf16* fx_hi; const __bf16* fx_lo; unsigned fx_bytes;
  const NrUnit* units; int nunits;                // the units in consumption order (device memory)
  int L;
  NrStage st[9];
  int rows, kS;                                   // sample rows of the launch (kS >= 128), samples per image
  const float* P0; int ldP0; int d0;              // first encoder layer's (mu | zs) per image
  const float* x; int ldx; int xdim;              // pixels [images][ldx], xdim <= 800
  uint64_t seed; const uint64_t* rng_base;
  const float* eps[8]; int eps_N, eps_i0, eps_s0; // injected noise (MgLaunch's convention) or null
  float* lw;                                      // out: log w per row
  // train mode (the forward of a train step): h1 / eps1 stores, per-row log q,
  // log p and the Bernoulli sum (bern[row * ld_bern]), g's weight wa
  int train;
  float* h1; int ld_h1; float* e1; int ld_e1;
  float* logq; float* logp; float* bern; int ld_bern;
  float wa;
};
bool nring_shape_ok(const NrLaunch& L);   // L, stage ns filled: an instantiated shape
hipError_t launch_nring(hipStream_t st, const NrLaunch& L);
hipError_t nring_setup_attributes();
size_t nring_lds_bytes();

// nrb_kernel (iwae_nring.hip): the output MLP's backward of a large-batch train
// step (the train engine's job O': (dpx g) W3^T (1 - y2^2) -> W2^T (1 - y1^2)
// -> W1^T) on 128-row workgroups sharing the GX weights through an LDS-DMA ring;
// g is streamed by LDS-DMA beside the weights.  Units: NrUnit with
// ns = pieces | piece stride in KiB << 8 (output-layer units: 8 column tiles
// of one k step; the others: one column tile, its k steps).
constexpr int kNrbMaxUnits = 128;
struct NrbLaunch {
  const __bf16* fx_hi; const __bf16* fx_lo; unsigned fx_bytes;
  const NrUnit* units; int nunits;
  int rows;
  const float* g; int ld_g; int N;                // the Bernoulli layer's g (forward's store), width
  const float* dpx;                               // dL/dlog p(x|h) per row (the bound's)
  const float* y2; int ld_y2; const float* y1; int ld_y1;   // the output MLP's tanh outputs
  float* dY2; int ld_dY2; float* dY1; int ld_dY1;           // their dZ (weight gradients); may be null
  float* dh; int ld_dh;                           // dL/dh1 of the output MLP
  int H, d1;                                      // hidden width, h1 width
  int gx3_tiles, gx3_steps, gx2_tiles, gx2_steps, gx1_tiles, gx1_steps;   // shape check
};
bool nrb_shape_ok(const NrbLaunch& L);
hipError_t launch_nrb(hipStream_t st, const NrbLaunch& L);

// nre_kernel (iwae_nring.hip): the decoder prior's and the encoder's backward
// of a large-batch 2-layer train step (the train engine's job E': prior
// Gaussian backward -> ph^T (1 - y2^2) -> p2^T (1 - y1^2) -> p1^T = dL/dh2 of
// the prior; encoder Gaussian backward of h2 -> eh^T -> e2^T -> e1^T = dL/dh1
// of the encoder) on the weight ring, GX units of the six Dense layers (k steps
// of one column tile each, nring_kernel's unit format) in that order.
struct NreLaunch {
  const __bf16* fx_hi; const __bf16* fx_lo; unsigned fx_bytes;
  const NrUnit* units; int nunits;
  int rows;
  const float* dlw;                               // dL/dlog w per row (the bound's)
  // prior of h1 given h2 (decoder layer 0): head (mu | zs), target h1, tanh outputs
  const float* Pp; int ld_Pp; const float* h1; int ld_h1; int dp;
  const float* py2; int ld_py2; const float* py1; int ld_py1; int Hp;
  float* pdP; int ld_pdP; float* dh_prior; int ld_dh_prior;
  float* pdY2; int ld_pdY2; float* pdY1; int ld_pdY1;
  float* dh_dec; int ld_dh_dec;                   // dL/dh2 of the prior chain
  // encoder layer 1 (h1 -> h2): head (mu | zs), h2, eps2, tanh outputs
  const float* Pe; int ld_Pe; const float* h2; int ld_h2; const float* e2; int ld_e2; int de;
  const float* ey2; int ld_ey2; const float* ey1; int ld_ey1; int He;
  float* edP; int ld_edP; float* edY2; int ld_edY2; float* edY1; int ld_edY1;
  float* dh_enc; int ld_dh_enc;                   // dL/dh1 of the encoder chain
  int gx_tiles[6], gx_steps[6];                   // ph, p2, p1, eh, e2, e1 (shape check)
};
constexpr int kNreGap = 6;       // empty units in nre_kernel's table between its ring phases (NR_D - NR_G)
bool nre_shape_ok(const NreLaunch& L);
hipError_t launch_nre(hipStream_t st, const NreLaunch& L);

// ---------------------------------------- row-chain train engine (bf16x3) ----
// The small- and large-batch train step's per-sample-row work (everything
// after the first encoder layer, forward and backward) as chains of ops run by
// one workgroup on 16*RT sample rows whose activations stay in LDS as split
// bf16 planes (iwae_train.hip).  Dense ops take the layer's split copy F
// (forward, k = fin + 1) or G (backward, k = fout) as the MFMA A operand
// streamed from L2, the LDS activations as B, bf16x3 products on
// v_mfma_f32_16x16x32_bf16; epilogues write the f32 tensors the weight
// gradients and later ops read.  A launch runs up to kTcMaxJobs independent
// chains (workgroups [block_start[j], block_start[j+1]) run job j).
enum TcKind {
  // Dense ops (kind <= TC_LAST_DENSE): MFMA tile loop + epilogue
  TC_TANH = 0,       // out = tanh(acc)                                   Dense(tanh) F:26-F:27, F:92-F:93
  TC_SAMPLE = 1,     // encoder head: h = eps*scale + mu, log q (+ log N(h;0,1))   F:37, F:68-F:73
  TC_PRIOR = 2,      // decoder head: log N(h_t; mu, scale), h_t read (f32)       F:138-F:141
  TC_BERN = 3,       // output Dense(784): Bernoulli log-prob row sum + dLoss/dlogit factor g   F:123-F:128
  TC_TGRAD = 4,      // backward dX = dZ W^T (1 - y^2)  (tanh of the forward layer below)
  TC_LIN = 5,        // backward dX = dZ W^T (no activation): dL/dh contribution
  TC_HEADP = 6,      // first encoder layer's head on image rows: stores P = (mu | zs) only   F:37
  TC_LAST_DENSE = 6,
  // elementwise ops
  TC_SAMPLE0 = 7,    // sample h1 from the image's first-layer (mu | zs)         F:58-F:60
  TC_GBWD_PRIOR = 8, // dP of a decoder head (+ dL/dh of its target)
  TC_GBWD_ENC = 9,   // dP of an encoder sampling head from the dL/dh sources
  TC_LOADG = 10,     // B operand = dpx[row] * g[row][:] (output layer backward)
  TC_LOADSLAB = 11,  // image rows: y1 = tanh(sum of the input layer's split-K slabs)   F:26
  TC_GBWD0 = 12      // image rows: dP0 = sum over the image's k samples of the h1 Gaussian backward
};
constexpr int kTcMaxOps = 20, kTcMaxBufs = 16, kTcMaxJobs = 3;
struct TcOp {
  int kind;
  const __bf16* Whi; const __bf16* Wlo; unsigned W_bytes; int ldk, K, N;   // dense ops: split rows [.][ldk]
  int in_buf, out_buf;        // LDS buffers (-1: none)
  int next_k;                 // columns of out_buf its reader consumes (zero padded)
  int ones;                   // forward: ones column (bias row of W_aug) at the output width
  int d, layer, stdnormal;    // heads / Gaussian ops: latent width, Philox layer, add log N(h; 0, 1)
  int acc;                    // SAMPLE0 / heads: this job accumulates the row's log q / log p terms
  float* out; int ld_out;     // f32 copy of the output: y, dZ, dX, P (mu | zs), dP, g
  float* h; int ld_h;         // SAMPLE / SAMPLE0: h (write); PRIOR / GBWD_*: h (read)
  float* eps; int ld_eps;     // SAMPLE / SAMPLE0: eps (write); GBWD_ENC: eps (read)
  const float* y; int ld_y;   // TGRAD: forward tanh output; LOADG: g
  const float* P; int ld_P; int P_div;   // SAMPLE0: image P0 (row / P_div); GBWD_*: head P
  const float* src[4]; int ld_src[4]; int nsrc;   // GBWD_ENC: dL/dh sources summed
  float* dh; int ld_dh;       // GBWD_PRIOR: dL/dh of the target h
  int t0;                     // dense ops: first column tile (a job may run a column range [16 t0, N))
  int nslab; long long slab_stride;   // LOADSLAB: partial slabs at y + i * slab_stride ([rows][ld_y] each)
  int img;                    // runs on the images of the workgroup's sample rows (rows b = row / kS)
  int gsync;                  // reads global data an earlier op of this launch wrote: full barrier before it
};
// The op's "hot" record: what the op loop and a Dense op's prologue read,
// resolved on the host for the plan's row-tile count and packed into one
// 64-byte line, which the kernel reads whole (one s_load_dwordx16, one wait)
// -- for op s + 1 during op s, so the hand-over prefetch and the op itself use
// the same registers.  TcOp keeps everything (the epilogues and the
// elementwise ops read their fields from it where they use them).
constexpr unsigned kTcHotImg = 1u << 8;        // TcOp::img
constexpr unsigned kTcHotOnes = 1u << 9;       // TcOp::ones (ones column at pad_lo)
constexpr unsigned kTcHotFullSync = 1u << 10;  // a full barrier follows the op (the next op reads this launch's global stores, or none follows)
constexpr unsigned kTcHotNextDense = 1u << 11; // the next op is a Dense op whose first units this op may request
struct alignas(64) TcHot {
  uint32_t whi_lo, whi_hi, wlo_lo, wlo_hi;   // Dense: the two weight planes' buffer bases ...
  uint32_t W_bytes;                          // ... and their range
  uint32_t flags;                            // TcKind in bits 0-7 | kTcHot*
  uint32_t in_off, in_ld;                    // Dense: input hi plane, bf16 offset / row stride (lo plane: + 16 RT ld)
  uint32_t out_off, out_ld;                  // Dense: output hi plane (the input's when the op has no LDS output)
  uint32_t pad;                              // Dense: per-op zero padding, columns [pad & 0xFFFF, pad >> 16) of the output
  uint32_t kt;                               // Dense: ldk / 32 | k chunks of 128 (nch) << 16
  uint32_t ntile, t0;                        // Dense: column tiles of N, the first one the job runs
  uint32_t N;
  uint32_t rsvd;
};
static_assert(sizeof(TcHot) == 64, "one 64-byte line per op");
// A Dense output's padding written before the job's first barrier instead of
// by its op (plans in which every op's LDS output has a buffer of its own)
struct TcPad {
  uint32_t off, ld;           // output hi plane: bf16 offset / row stride
  uint32_t pad;               // columns [pad & 0xFFFF, pad >> 16)
  uint32_t ones;              // ones column at the first of them
};
struct TcJob {
  TcHot hot[kTcMaxOps];       // first: every record on a line of its own (TcPlan is 64-byte aligned)
  TcPad pre[kTcMaxOps]; int npre;   // the up-front padding (npre > 0: the ops' own TcHot::pad are 0)
  TcOp op[kTcMaxOps]; int nop;
  int buf_off[kTcMaxBufs], buf_ld[kTcMaxBufs];   // bf16 offset of the hi plane / row stride
  float* logq; float* logp; float* bern; int ld_bern, bern_col;   // per-row sums this job writes (null: none)
  int bern_ncol;              // jobs that split the Bernoulli columns (1: this job alone also zeroes column 1)
  float* bce;                 // L_alpha: per-row Keras-BCE sums (same layout as bern)
};
struct TcPlan {              // device resident (built once per shape)
  TcJob job[kTcMaxJobs]; int njobs;
  int acc_off;               // float offset of the per-row accumulators + reduction scratch
};
// op kinds an engine launch's plan uses (bit 1 << TcKind): the launch picks the
// kernel instantiation compiled for the smallest of these sets that covers them
// (fewer epilogue kinds inlined at the op loop's call sites: less code to fetch)
constexpr unsigned kTcKindsFwd = (1u << TC_TANH) | (1u << TC_SAMPLE) | (1u << TC_PRIOR) | (1u << TC_BERN) |
                                 (1u << TC_HEADP) | (1u << TC_SAMPLE0) | (1u << TC_LOADSLAB);
constexpr unsigned kTcKindsBwd = (1u << TC_TGRAD) | (1u << TC_LIN) | (1u << TC_GBWD_PRIOR) | (1u << TC_GBWD_ENC) |
                                 (1u << TC_LOADG) | (1u << TC_GBWD0);
constexpr unsigned kTcKindsAll = 0x1FFFu;
// (16-row backward launches also have narrower sets: the sample-row backward
// without job I' op, job I' alone)
constexpr unsigned kTcKindsBwdRows = (1u << TC_TGRAD) | (1u << TC_LIN) | (1u << TC_GBWD_PRIOR) | (1u << TC_GBWD_ENC) |
                                     (1u << TC_LOADG);
constexpr unsigned kTcKindsImgBwd = (1u << TC_TGRAD) | (1u << TC_LIN) | (1u << TC_GBWD0);
// job I alone (the first encoder layer's l2 / head on image rows above 32 images)
constexpr unsigned kTcKindsImgFwd = (1u << TC_LOADSLAB) | (1u << TC_TANH) | (1u << TC_HEADP);
// not an op kind: an engine instantiation whose activation / dZ stores are
// write-through (sc1) -- job I' inside tcu_kernel, the producer side of the
// write-through hand-off (UpdWait::wt) -- and, under the store policy
// (TcArgs::st_wt), every global store of a 16-row forward / backward launch
constexpr unsigned kTcWriteThrough = 1u << 31;
struct TcArgs {
  const TcPlan* plan;
  unsigned kinds;             // op kinds of the plan's jobs (host-computed; 0: all)
  int block_start[kTcMaxJobs + 1];
  int rows, kS;
  int row_step;                             // rows per workgroup (0: 16 * RT; image-row launches: 1)
  // XCD-aware placement (xcd_slots > 0): workgroup b runs on XCD b % 8 (round-robin dispatch);
  // XCD x serves job xcd_job[x] as its xcd_rank[x]-th of xcd_count[job] XCDs, so each XCD's
  // L2 fetches one job's weights.  Grid = 8 * xcd_slots; workgroups past a job's blocks exit.
  int xcd_slots; int xcd_job[8], xcd_rank[8], xcd_count[kTcMaxJobs];
  const float* x; int ldx;                  // pixels by image
  uint64_t seed; const uint64_t* rng_base;
  const float* eps_a[8]; const float* eps_b[8]; int Bsplit, Bimg;   // injected noise ([k][B][d]) or null
  const float* dlw; const float* dpx; float wa;
  float wb; int need_bce;                   // L_alpha: Keras-BCE term of the output epilogue (weight wb)
  // unit row weights (PIWAE): the backward chain runs with dL/dlw = dpx = 1 per
  // row (every output of the chain is linear in a row's weight), the weight
  // gradients scale each layer's dZ rows by its own weighting afterwards, and
  // the image-row Gaussian backward scales its dL/dh sources by dlw per sample
  int unit_w;
  // the bound inside the backward launch (bnd_rows): every workgroup computes
  // its rows' dL/dlw and dpx into LDS at float offset bnd_lds (dpx at + 16 RT)
  // from its images' log weights, staging an image per wave at float offset
  // bnd_stage + wave * bnd_ld (0: the op buffers' space, nothing in them yet;
  // plans padded up front: the final row reduction's scratch);
  // workgroup bnd_block (the grid's last) runs the whole bound: log weights,
  // loss, global dlw / dpx, the Philox base and the Adam step
  BoundArgs bnd; int bnd_rows, bnd_block, bnd_ld, bnd_lds, bnd_stage;
  // store policy (iwae_set_store_policy; 16-row plans only).  st_wt: launch_tc runs the
  // write-through instantiation of the plan's kind set (every global store sc1).
  // rel_jobs: the workgroups of these jobs (bit per job), which end well before
  // the launch does, write their XCD's L2 back themselves as their last act
  // (wg_release_l2), so the write-back at the launch's end finds less to do
  int st_wt; unsigned rel_jobs;
};
hipError_t launch_tc(hipStream_t st, const TcArgs& a, int rt, size_t lds_bytes);
// job I' (a one-job image-row plan, RT = 1) and the fused update (8 waves) in one launch
hipError_t launch_tcu(hipStream_t st, const TcArgs& a, const UpdArgs& u, const UpdWait& w, size_t lds_bytes);
hipError_t tc_setup_attributes();

hipError_t launch_fill_col(hipStream_t st, float* buf, int rows, int ld, int col, float v);
// Evaluation statistics (F:249-F:302).  out[b][j] (+)= scale * sum_s H[b*n+s][j]
// for b < N, j < d; block 0 advances the Philox base when rng_base is given.
hipError_t launch_group_mean(hipStream_t st, const float* H, int ldH, int n, int d, int N, float* out, int ldo,
                             float scale, int accumulate, uint64_t* rng_base);
// probs = sigmoid(logit) * (1 - 1e-6) + 1e-7 in place over [rows][ld] (F:102)
hipError_t launch_bern_probs(hipStream_t st, float* z, int rows, int cols, int ld);
hipError_t launch_transpose_lw(hipStream_t st, const float* lw_img, int Bimg, int kS, float* out);

// ------------------------------------- generation from the prior (fused) ----
// gen_kernel (iwae_generate.hip): Decoder.generate_x (F:107-F:119) on 16*RT
// generated rows per workgroup, activations resident in LDS as split bf16
// planes, on the chain machinery it shares with mega_fwd_kernel
// (iwae_mega_dev.h: storage, weight streaming, MFMA loop, tile loop): top
// latent h_L (given, injected or Philox) -> per prior layer tanh, tanh, head:
// sample h -> output MLP tanh, tanh, Dense(x_dim) -> probabilities (F:101-F:102)
// and / or Bernoulli pixel draws.  Stage fields: MgStage's (act: GnAct; head
// stages: layer = the Philox layer id; K and stdnormal unused), and:
enum GnAct { GN_TANH = MG_TANH, GN_OUT = 2, GN_HEAD = 3 };
struct GnStage : MgStage {
  const float* eps;          // HEAD: injected noise [n][d], or null (Philox)
  float* h_out;              // HEAD: f32 copy of the sampled latent [n][d], or null
};
struct GnLaunch {
  GnStage st[kMgMaxStages]; int nst;
  int buf_off[kMgMaxBufs], buf_ld[kMgMaxBufs];   // bf16 offset of the hi plane / row stride
  int n;                                          // generated rows
  // top latent: h_top [n][d_top], else eps_top [n][d_top] (h_L = eps * 1 + 0), else Philox normals
  const float* h_top; const float* eps_top; float* top_out;
  int d_top, top_buf, top_next_k, top_layer;
  // outputs (either may be null): probabilities / pixels [n][ld]; u: injected uniforms [n][xdim] or null
  float* probs; int ld_probs; float* pixels; int ld_pixels; const float* u; int pix_layer;
  uint64_t seed; uint64_t* rng_base; unsigned* ticket;   // the last workgroup advances the Philox base
};
hipError_t launch_gen(hipStream_t st, const GnLaunch& L, int rt, size_t lds_bytes);
hipError_t gen_setup_attributes();

// layer-wise generation (iwae_elem.hip), same Philox counters as gen_kernel:
// top latent H[r][j] = src[r][j] (h_top or injected eps) or a Philox normal
// (+ optional tight f32 copy), pixel draws out = (u < p), and the Philox base's
// advance as a one-thread launch
hipError_t launch_gen_top(hipStream_t st, const float* src, int n, int d, float* H, int ldH, float* copy,
                          uint64_t seed, const uint64_t* rng_base, int layer);
hipError_t launch_gen_pixels(hipStream_t st, const float* p, int ldp, const float* u, int n, int xdim, float* out,
                             int ldo, uint64_t seed, const uint64_t* rng_base, int layer);
hipError_t launch_rng_advance(hipStream_t st, uint64_t* rng_base);

// ------------------------- importance-weighted posterior (iwae_posterior.hip) ----
// Self-normalised weights of a chunk whose images hold all their k samples:
// from the per-row log weights (LseArgs' sources: lw, or part / logp / logq)
// and the image's (m, sum e) left by lse_kernel, w~ = exp(lw - m) / sum e per
// row, ess = (sum e)^2 / sum e^2 and the SIR index min{ j : sum_{s <= j} w~_s >
// u } (clamped to k - 1; the sum in sample order) per image.  One workgroup per
// image, fixed reduction order.
struct PostWArgs {
  LseArgs src;               // the rows' log weights, kS, Bimg, run_m / run_s (read)
  float* wt;                 // out: w~ per row [Bimg * kS] (image-major, as the rows)
  float* ess;                // out [Bimg], or null
  int* sir;                  // out [Bimg], or null
  const float* u;            // uniforms [Bimg], or null: Philox (row = image, layer u_layer, quad 0, first value)
  uint64_t seed; const uint64_t* rng_base; int u_layer;
};
hipError_t launch_post_weights(hipStream_t st, const PostWArgs& a);

// post_kernel: the weighted second pass over a chunk's rows, fused.  A
// workgroup owns up to 16*RT samples of ONE image (workgroup = image * tiles +
// tile) and runs the encoder chain after the first layer and the output MLP
// on them with the chain machinery shared with gen_kernel / mega_fwd_kernel
// (iwae_mega_dev.h: split bf16 planes in LDS, bf16x3 MFMA, FX weights as the A
// operand); the sampling and output epilogues multiply by the row's w~ (tail
// rows: 0), reduce over the rows and write one partial vector [h_1 | .. | h_L
// | probs] per workgroup; the row whose sample index is the image's SIR index
// stores its latents.  post_merge_kernel sums an image's partials in tile
// order.  Stage fields: MgStage's (act: PoAct;
// out_buf of a SAMPLE stage -1: the top latent, which no stage reads: summed
// and stored by the epilogue only; layer: Philox layer id = encoder layer; K
// and stdnormal unused), and:
enum PoAct { PO_TANH = MG_TANH, PO_OUT = 2, PO_SAMPLE = 3 };
struct PoStage : MgStage {
  int part_off;              // SAMPLE / OUT: float offset of this stage's sums in the partial vector
};
struct PoLaunch {
  PoStage st[kMgMaxStages]; int nst;
  int buf_off[kMgMaxBufs], buf_ld[kMgMaxBufs];   // bf16 offset of the hi plane / row stride
  int stage_buf;                                  // buffer that holds h_1 as f32 [rows][buf_ld] during the prologue
  int w_off;                                      // LDS float offset of the rows' weights [16 RT]
  int Bimg, kS, tiles;                            // images of the chunk, samples per image, workgroups per image
  const float* P0; int ldP0; int d0; int h0_buf; int h0_next_k;   // prologue: h_1 from the image's (mu | zs)
  uint64_t seed; const uint64_t* rng_base;        // the base pass 1 drew with
  const float* eps[8]; int eps_N, eps_i0;         // injected noise (MgLaunch's convention) or null
  const float* wt;                                // w~ per row
  const int* sir;                                 // SIR index per image, or null
  float* h_sir[8];                                // the chunk's rows of the callers' [N][d_i] buffers, or null
  int want_mean;                                  // the latents' sums are formed (probs: the plan has the output stages)
  float* part; int ld_part;                       // [Bimg * tiles][ld_part]
};
hipError_t launch_post(hipStream_t st, const PoLaunch& L, int rt, size_t lds_bytes);
hipError_t post_setup_attributes();
// Segment g of the partial vector, columns [off, off + width): out[g][b * ldo + j] = the sum over the
// image's tiles, in tile order, of part[(b * tiles + t) * ld_part + off + j]
struct PoMerge {
  const float* part; int ld_part, tiles, Bimg;
  int nseg; int off[9], width[9], ldo[9]; float* out[9];
};
hipError_t launch_post_merge(hipStream_t st, const PoMerge& a);
// Weighted sibling of group_mean_kernel: out[b][j] = sum_s wt[b*n + s] * H[b*n + s][j] (sample order);
// sir given: sel[b][j] = H[b*n + sir[b]][j] as well
hipError_t launch_group_wsum(hipStream_t st, const float* H, int ldH, int n, int d, int N, const float* wt, float* out,
                             int ldo, const int* sir, float* sel, int ldsel);


// ---------------------- imputation of missing pixels (iwae_impute.hip) ----
// mask [n][xdim]: non-zero = observed.  Every kernel selects by the mask, so a
// missing entry of x (NaN and Inf included) never reaches an output.
// Staging: x_in[r][j] = mask ? x : 0 (the encoder's input; columns past xdim,
// the ones column among them, are left alone) and, when xm is given, xm[r][j] =
// mask ? x : -1 for j < xdim, 0 for xdim <= j < ld_m (the masked
// mega_fwd_kernel's pixels).
hipError_t launch_impute_stage(hipStream_t st, const float* x, const float* mask, int n, int xdim, float* x_in,
                               int ld_in, float* xm, int ld_m);
// Layer-wise first pass: part[r] = (sum_j [mask] x log p + (1 - x) log(1 - p), 0, 0, 0) of the row's logits
// Z[r][0..xdim) (row r = image r / kS), p = sigmoid(z) (1 - 1e-6) + 1e-7 (F:126), one wave per row in a fixed
// order; to_probs: the logits are replaced by p (bern_probs_kernel's value) for the second pass.
hipError_t launch_impute_rowsum(hipStream_t st, float* Z, int ldz, int rows, int kS, const float* x_in, int ld_in,
                                const float* mask, int xdim, float* part, int to_probs);
// out[b][j] = mask ? x : out[b][j] (the weighted probabilities already there), j < xdim
hipError_t launch_impute_fill(hipStream_t st, const float* x, const float* mask, int n, int xdim, float* out, int ldo);
// out[b][j] = mask ? x : (u < p[b][j]) as 0.0 / 1.0; u: [n][xdim] or null: Philox uniforms (row b, `layer`,
// column quad j / 4, value j % 4: gen_kernel's layout)
hipError_t launch_impute_draw(hipStream_t st, const float* x, const float* mask, const float* p, int ldp,
                              const float* u, int n, int xdim, float* out, int ldo, uint64_t seed,
                              const uint64_t* rng_base, int layer);

// ------------------------------- dynamic binarisation (iwae_binarize.hip) ----
// out[i][j] = (u < v || v >= 1) as 0.0 / 1.0, v = x[perm[i]][j] (perm null: row i), j < xdim; x [n_src][xdim],
// a perm[i] outside [0, n_src) reads nothing and gives zeros; u: [n][xdim] or null: Philox uniforms (row i,
// `layer`, column quad j / 4, value j % 4: gen_kernel's layout).  out may be x when perm is null and ldo == xdim.
// Fewer than 2^32 - 255 (row, quad) threads, else hipErrorInvalidValue.
hipError_t launch_binarize(hipStream_t st, const float* x, long long n_src, const long long* perm, const float* u,
                           int n, int xdim, float* out, int ldo, uint64_t seed, const uint64_t* rng_base, int layer);

// ------------------------- annealed importance sampling (iwae_ais.hip) ----
// One transition's launches between the gradient passes.  Chain c = b k + s
// (image b, sample s); cur / r / q / g / mom: per layer [k][N][d_i], sample-major;
// every per-chain scalar [N][k].  lq / lph / lpx and g are what the last
// iwae_score_grad pass left for the state it was given; (cq, cph, cpx) its
// coefficients (a zero coefficient's term is left out of the energy).
struct AisArgs {
  int L, N, k, group;                   // group: lanes per chain, 16 or 64
  long long chains;                     // N k
  int d[8], vec[8];                     // vec: ais_step_kernel takes the layer in float4 (d % 4 == 0, aligned)
  float* cur[8]; float* r[8]; float* q[8]; const float* g[8];
  const float* mom[8];                  // begin: injected momenta, or null (Philox normals, layer id mom_layer + i)
  const float *lq, *lph, *lpx;
  float cq, cph, cpx;
  int init;                             // Delta: 0 log p(x|h), 1 log p(h) + log p(x|h) - log q(h|x)
  float dbeta;                          // begin: log_w += dbeta Delta
  int zero;                             // the call's first transition, not accumulating: log_w / accepts start at 0
  float step0;                          // > 0: every chain's step in this transition (step[] not yet written)
  float* step; float* H_old;
  float* log_w; float* accepts;         // either may be null
  const float* u;                       // end: this transition's uniforms [N][k], or null (Philox, layer u_layer)
  uint64_t seed; const uint64_t* rng_base; unsigned t_off;   // noise base = *rng_base + t_off
  int mom_layer, u_layer;
  float inc, dec, smin, smax;           // end: step = clamp(step (accept ? inc : dec), smin, smax)
};
hipError_t launch_ais_begin(hipStream_t st, const AisArgs& a);
hipError_t launch_ais_step(hipStream_t st, const AisArgs& a);
hipError_t launch_ais_end(hipStream_t st, const AisArgs& a);
// logpx[b] = logsumexp_s log_w[b][s] - log k, ess[b] = (sum e)^2 / sum e^2 (either may be null; nothing is
// reduced when log_w is); the noise position moves on by n_adv when rng_base is given
hipError_t launch_ais_finish(hipStream_t st, const float* log_w, int N, int k, float* logpx, float* ess,
                             uint64_t* rng_base, unsigned n_adv);

// -------------------- per-image variational refinement (iwae_refine.hip) ----
// One call's launches between the gradient passes.  mean / logstd and the Adam
// moments: per layer [N][d_i]; lat / epsw / g / eps_in / lat_out: per layer
// [k][N][d_i], sample-major (lat, epsw: the workspace's latents and their
// noise); every per-sample scalar [N][k].  lph / lpx and g are what the last
// iwae_score_grad pass left for lat.
struct RefineArgs {
  int L, N, k, group, D;                // group: lanes per sample in the log q* sums, 16 or 64; D = sum d_i
  int d[8], vec[8];                     // vec: the draw stores the layer in float4 (d % 4 == 0)
  float* mean[8]; float* logstd[8];
  float* m1m[8]; float* m2m[8]; float* m1s[8]; float* m2s[8];   // Adam moments of mean_i and of logstd_i
  float* lat[8]; float* epsw[8]; const float* g[8];
  const float* eps_in[8];               // draw: the pass's injected noise, or null (Philox normals, noise_layer + i)
  const float *lph, *lpx;
  float* lw;                            // log w_s, then a_s, of the current iteration
  float* bound;                         // this iteration's [N], or null
  int objective;                        // 0 ELBO, 1 IWAE_k
  int zero;                             // the moments are taken as 0 (first update of a run)
  int draw;                             // end: draw the evaluation pass
  float lr_n, omb1, omb2, eps_hat, ls_min, ls_max;
  uint64_t seed; const uint64_t* rng_base; unsigned pass;       // the draw's noise base = *rng_base + pass
  int noise_layer;
  // finish
  int eval;                             // there was an evaluation pass
  float* lat_out[8]; float* log_w; float* logpx; float* ess;   // each may be null (log_w: wherever logpx / ess need it)
  uint64_t* rng_adv; unsigned n_adv;    // the noise position moves on by n_adv
};
hipError_t launch_refine_begin(hipStream_t st, const RefineArgs& a);
hipError_t launch_refine_step(hipStream_t st, const RefineArgs& a);
hipError_t launch_refine_end(hipStream_t st, const RefineArgs& a);
hipError_t launch_refine_finish(hipStream_t st, const RefineArgs& a);

// ----------------------------------------------- aggregate posterior ----
// iwae_aggregate's kernels (iwae_aggregate.hip).  R query
// rows lat [R][d] against M reference components given as mu, rs = 1 / s and
// lc = -(log s + 1/2 log 2 pi), [M][d] each (launch_agg_prep forms the last two
// from the scales).  The references are walked in nseg segments of seg_len
// (the last one shorter); nseg == 1 writes out = logsumexp - log_m directly,
// else each segment writes its (max, sum) to part ([R][nseg][2] joint,
// [R][d][nseg][2] per unit) and launch_agg_merge combines them in segment
// order.  vec: d % 4 == 0 and lat, mu, rs, lc 16-byte aligned (float4 loads;
// the scalar path gives the same bits).
constexpr int kAggJointRows = 64;    // query rows per workgroup of agg_joint_kernel
constexpr int kAggJointRefs = 64;    // references per tile
constexpr int kAggJointCols = 32;    // most columns per LDS pass
constexpr int kAggDimTile = 4096;    // agg_dim_kernel: floats per LDS array (references per tile x units per chunk)
constexpr int kAggDimUnits = 256;    // ... most units per chunk
constexpr int kAggWgs = 1024;        // workgroups below which the references are split
constexpr int kAggMaxSeg = 1024;     // most segments
struct AggArgs {
  const float* lat; long long R;
  const float *mu, *rs, *lc;
  int M, d, vec;
  int seg_len, nseg;
  int uw, tm;                        // agg_dim_kernel: units per chunk, references per tile (uw tm <= kAggDimTile)
  float log_m;
  float* out;
  float* part;
};
// The split rule: wgs workgroups would walk all M references in tiles of
// `tile`.  At kAggWgs or more: one segment.  Below: ceil(kAggWgs / wgs)
// segments, at most kAggMaxSeg and at most one per tile, of equal length
// rounded up to whole tiles.  A function of (R, M, d) alone.  A split launch
// has wgs < kAggWgs workgroups of at most 64 rows (joint) or 1024 (row, unit)
// pairs (per unit) and fewer than kAggWgs / wgs + 1 segments, so its partials
// stay below 2 * 64 * 2 kAggWgs = 2^18 and 2 * 1024 * 2 kAggWgs = 2^22 floats.
inline void agg_split(long long wgs, int M, int tile, int& seg_len, int& nseg) {
  long long n = wgs >= kAggWgs ? 1 : (kAggWgs + wgs - 1) / wgs;
  const long long tiles = ((long long)M + tile - 1) / tile;
  if (n > tiles) n = tiles;
  if (n > kAggMaxSeg) n = kAggMaxSeg;
  const long long per = (tiles + n - 1) / n;
  seg_len = (int)(per * tile);
  nseg = (int)((tiles + per - 1) / per);
}
inline int agg_dim_units(int d) { return d < kAggDimUnits ? d : kAggDimUnits; }
inline int agg_dim_refs(int d) { const int t = kAggDimTile / agg_dim_units(d); return t < 128 ? t : 128; }
inline long long agg_joint_wgs(long long R) { return (R + kAggJointRows - 1) / kAggJointRows; }
inline long long agg_dim_wgs(long long R, int d) {
  const int uw = agg_dim_units(d);
  return (((R + 3) / 4) * uw + 255) / 256 * ((d + uw - 1) / uw);
}
hipError_t launch_agg_prep(hipStream_t st, const float* scale, long long n, float* rs, float* lc);
hipError_t launch_agg_joint(hipStream_t st, const AggArgs& a);
hipError_t launch_agg_dim(hipStream_t st, const AggArgs& a);
hipError_t launch_agg_merge(hipStream_t st, const float* part, long long n, int nseg, float log_m, float* out);
hipError_t launch_agg_own(hipStream_t st, const AggArgs& a, int period, float* own, float* own_dim);

}  // namespace iwae
