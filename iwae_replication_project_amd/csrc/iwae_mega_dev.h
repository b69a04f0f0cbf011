// Device code shared by every fused kernel that runs a chain of Dense stages
// in LDS: the fused k-sample forward (mega_fwd_kernel, iwae_mega.hip, whose
// head comment describes the pipeline), the scoring kernel built on its stages
// (score_kernel, iwae_score.hip), generation from the prior (gen_kernel,
// iwae_generate.hip) and the posterior's weighted second pass (post_kernel,
// iwae_posterior.hip); sg_kernel (iwae_scoregrad.hip) takes the basic pieces
// (MgBuf, the vector types, mg_pad, the barrier) and has its own tile code.
// Here: LDS buffers, weight-fragment fetch, the bf16x3 MFMA loop, the tanh
// epilogue, the barrier, and the loop over a wave's column tiles (mg_tiles),
// which gen_kernel and post_kernel call with epilogues of their own.
// mega_fwd_kernel and score_kernel keep their Dense stage (mg_tile / mg_dense,
// with their operand requests and epilogues) as a second, written-out copy of
// that loop (see the comment there).  Every kernel lives in its own
// translation unit, so no kernel's code depends on another's presence.
#pragma once
#include "iwae_kernels.h"

namespace iwae {

typedef float mg_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 mg_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mg_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 mg_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned mg_u32x4 __attribute__((ext_vector_type(4)));

constexpr int MG_WAVES = 8;         // waves of the 64-row workgroup (NW template argument: 8 or 4)
constexpr int MG_KS = 8;             // k steps of 32 per weight fetch (256 k)
#ifndef IWAE_MG_PF
#define IWAE_MG_PF 2
#endif
constexpr int MG_PF = IWAE_MG_PF;    // steps of the next column tile requested during the current one
#ifndef IWAE_MG_UNCOND     // unconditional fragment loads: measured 62.9 K vs 63.8 K images/s, off
#define IWAE_MG_UNCOND 0
#endif

extern __shared__ __attribute__((aligned(16))) float mgs[];

#ifdef IWAE_MG_TRACE
// Debug build only (-DIWAE_MG_TRACE): s_memtime stamps of every wave of a few
// workgroups at the phase boundaries: [blk][wave][slot], slot 0 = kernel
// entry, 1 = prologue done, 2 + 3 s .. = stage s entry, dense done, barrier done.
// (static: one copy per translation unit that includes this header; mega_fwd_kernel's is the one dumped)
static __device__ unsigned long long g_mg_trace[4 * 8 * 128];
#define MG_TRACE(slot)                                                                  \
  {                                                                                     \
    const int tb_ = blockIdx.x == 0 ? 0 : blockIdx.x == 2000 ? 1 : blockIdx.x == 9000 ? 2 : \
                    blockIdx.x == gridDim.x - 1 ? 3 : -1;                               \
    if (tb_ >= 0 && (threadIdx.x & 63) == 0 && (slot) < 128)                            \
      g_mg_trace[(tb_ * 8 + (threadIdx.x >> 6)) * 128 + (slot)] = __builtin_amdgcn_s_memtime(); \
  }
#else
#define MG_TRACE(slot)
#endif

__device__ __forceinline__ mg_bf16x8 mg_as_bf16x8(mg_u32x4 v) { return __builtin_bit_cast(mg_bf16x8, v); }

// LDS buffer b: hi plane at bf16 offset off, lo plane at off + R * ld
struct MgBuf {
  __bf16* hi; __bf16* lo; int ld;
};
template <int RT, class LT>
__device__ __forceinline__ MgBuf mg_buf(const LT& L, int b) {
  __bf16* base = reinterpret_cast<__bf16*>(mgs);
  MgBuf B;
  B.ld = L.buf_ld[b];
  B.hi = base + L.buf_off[b];
  B.lo = B.hi + 16 * RT * B.ld;
  return B;
}

// NLL-path tanh: 1 - 2 / (exp(2x) + 1), one exp and one reciprocal; absolute
// error ~1 ulp of 1 (6e-8), below the 2^-16 relative split of the next product
__device__ __forceinline__ float mg_tanh(float x) {
  return __builtin_fmaf(-2.f, frcp(fexp(2.f * x) + 1.f), 1.f);
}

// ones column (K - 1 of the next reader) and zero padding of columns [width, next_k)
template <int RT, int NW>
__device__ __forceinline__ void mg_pad(const MgBuf& B, int width, int next_k) {
  constexpr int TPR = (NW * 64) / (16 * RT);    // threads per row
  const int row = threadIdx.x / TPR;
  for (int col = width + threadIdx.x % TPR; col < next_k; col += TPR) {
    B.hi[row * B.ld + col] = (__bf16)(col == width ? 1.f : 0.f);
    B.lo[row * B.ld + col] = (__bf16)0.f;
  }
}

struct MgFrag {
  mg_bf16x8 h[MG_KS], l[MG_KS];
};

// Byte offset (hi and lo planes alike) of this lane's fragment of column tile
// t at k0 in the fragment-major copy (FX: [tile][k step][64 lanes][8], head
// rows already permuted, padding rows zero), or kOOB
__device__ __forceinline__ unsigned mg_frag_base(const MgStage& S, int t, int k0) {
  const int lane = threadIdx.x & 63;
  const int ntile = (S.N + 15) >> 4;
  return t < ntile ? (unsigned)(((t * (S.ldk >> 5) + (k0 >> 5)) * 64 + lane) * 16) : kOOB;
}
// k step u of the fragment: 1 KiB further (an invalid tile's kOOB + 1024 u
// stays beyond the buffer: it reads 0)
// (IWAE_MG_UNCOND: unconditional, a step past ns reading zeros out of range,
// so the compiler's wait counts stay static -- measured slower here: the
// extra fragment registers cost more than the waits)
__device__ __forceinline__ void mg_fetch_step(__amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl, unsigned vb,
                                              int u, int ns, MgFrag& f) {
#if IWAE_MG_UNCOND
  const unsigned v = u < ns ? vb : kOOB;
  f.h[u] = mg_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rh, v, 1024 * u, 0));
  f.l[u] = mg_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rl, v, 1024 * u, 0));
#else
  if (u >= ns) return;
  f.h[u] = mg_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rh, vb, 1024 * u, 0));
  f.l[u] = mg_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rl, vb, 1024 * u, 0));
#endif
}
// A fragments of column tile t over k in [k0, k0 + 256): 8 steps of 32, hi and lo
__device__ __forceinline__ void mg_fetch(const MgStage& S, __amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl,
                                         int t, int k0, MgFrag& f) {
  const unsigned vb = mg_frag_base(S, t, k0);
  const int ns = (S.ldk - k0) >> 5;
#pragma unroll
  for (int u = 0; u < MG_KS; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
}

// acc[rt] += F-tile . IN[rows of rt][k0 .. k0 + 32 ns) (bf16x3).  With
// pf (uniform) the fragments of the first MG_PF steps are re-requested for
// the next column tile (of this stage or the next one: rh / rl / pf_ns are
// that tile's) right after their last MFMA (one register set; those
// loads have the rest of this tile and its epilogue to arrive), the others at
// the start of the next tile, ahead of its first MG_PF steps of MFMAs.
template <int RT>
__device__ __forceinline__ void mg_mma(const MgBuf& IN, int k0, int ns, MgFrag& f, mg_f32x4 (&acc)[RT],
                                       __amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl, bool pf, unsigned pf_vb,
                                       int pf_ns) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  // chunks of (k step u, row-tile pair p); the activation fragments of the next
  // chunk are read from LDS while this chunk's MFMAs run (two register sets)
  constexpr int RH = RT < 2 ? RT : 2;
  constexpr int NP = RT / RH;
  constexpr int NC = MG_KS * NP;
  mg_bf16x8 ah[2][RH], al[2][RH];
  auto rd = [&](int c, int b) {
    const int u = c / NP, p = c % NP;
#pragma unroll
    for (int i = 0; i < RH; ++i) {
      const int ao = ((p * RH + i) * 16 + r) * IN.ld + k0 + 32 * u + 8 * g;
      ah[b][i] = *reinterpret_cast<const mg_bf16x8*>(IN.hi + ao);
      al[b][i] = *reinterpret_cast<const mg_bf16x8*>(IN.lo + ao);
    }
  };
  rd(0, 0);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int u = c / NP, p = c % NP, b = c & 1;
    if (u >= ns) break;
    if (c + 1 < NC && (c + 1) / NP < ns) rd(c + 1, b ^ 1);
#pragma unroll
    for (int i = 0; i < RH; ++i)
      acc[p * RH + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.l[u], ah[b][i], acc[p * RH + i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < RH; ++i)
      acc[p * RH + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.h[u], al[b][i], acc[p * RH + i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < RH; ++i)
      acc[p * RH + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.h[u], ah[b][i], acc[p * RH + i], 0, 0, 0);
#if IWAE_MG_UNCOND
    if (p == NP - 1 && u < MG_PF) mg_fetch_step(rh, rl, pf ? pf_vb : kOOB, u, pf_ns, f);
#else
    if (p == NP - 1 && u < MG_PF && pf) mg_fetch_step(rh, rl, pf_vb, u, pf_ns, f);
#endif
  }
}

// Per-lane state carried through the stages: log w partial sums of the lane's
// rows (rt * 16 + r) -- natural-log terms and log2 Bernoulli products -- and
// the pixel offsets of their images.
template <int RT>
struct MgRows {
  float lw[RT];
  float l2[RT];
  unsigned xoff[RT];
};

// TFP Bernoulli(probs = sigmoid(l)*(1-1e-6)+1e-7).log_prob(x) (F:126-F:128).
// Binarised pixels: the selected probability is sigmoid(+-l) * c + (x ? 1e-7 :
// 1 - c - 1e-7), (1 - p written without the f32 cancellation of 1 - p), and
// four of them are multiplied (>= 1e-28) before one log2.  Both forms sum
// log2 terms; the row total is scaled by ln 2 once.
constexpr float kBernOff0 = 9.1327896e-7f;   // 1 - 0.999999f - 1e-7f (f32 constants, F:126)
//
// MASK (iwae_impute): xv is the staged copy whose missing pixels hold -1
// (impute_stage_kernel).  A negative pixel is the factor 1 of the binarised
// product and the term 0 of the fractional sum: the pixel leaves log p(x|h).
template <int RT, bool MASK>
__device__ __forceinline__ void mg_bern(const MgLaunch& L, const MgStage& S, int t, const mg_f32x4 (&acc)[RT],
                                        const float4 (&xv)[RT], MgRows<RT>& R) {
  const int g = (threadIdx.x & 63) >> 4;
  const int f0 = t * 16 + 4 * g;
  bool bin = true;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    if (MASK)
      bin = bin && (xv[rt].x <= 0.f || xv[rt].x == 1.f) && (xv[rt].y <= 0.f || xv[rt].y == 1.f) &&
            (xv[rt].z <= 0.f || xv[rt].z == 1.f) && (xv[rt].w <= 0.f || xv[rt].w == 1.f);
    else
      bin = bin && (xv[rt].x == 0.f || xv[rt].x == 1.f) && (xv[rt].y == 0.f || xv[rt].y == 1.f) &&
            (xv[rt].z == 0.f || xv[rt].z == 1.f) && (xv[rt].w == 0.f || xv[rt].w == 1.f);
  if (__all(bin)) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float prod = 1.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = f4_at(xv[rt], i);
        const bool one = MASK ? x > 0.f : x != 0.f;
        const float z = one ? acc[rt][i] : -acc[rt][i];
        const float s = frcp(1.f + fexp(-z));
        const float p = __builtin_fmaf(s, kProbScale, one ? kProbShift : kBernOff0);
        prod *= (f0 + i < S.N && !(MASK && x < 0.f)) ? p : 1.f;
      }
      R.l2[rt] += __builtin_amdgcn_logf(prod);
    }
  } else {
    // fractional pixels: x log p + (1 - x) log(1 - p), both probabilities
    // formed without cancellation and without overflow: a = exp(-|l|) <= 1,
    // r = 1 / (1 + a); sigmoid(|l|) = r, sigmoid(-|l|) = a r (exp(-l) itself
    // is inf below l = -88.7, and inf * 0 a NaN)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = f4_at(xv[rt], i);
        const float l = acc[rt][i];
        const float a = fexp(-__builtin_fabsf(l));
        const float r = frcp(1.f + a), ar = a * r;
        const float p1 = __builtin_fmaf(l >= 0.f ? r : ar, kProbScale, kProbShift);
        const float p0 = __builtin_fmaf(l >= 0.f ? ar : r, kProbScale, kBernOff0);
        const float v = x * __builtin_amdgcn_logf(p1) + (1.f - x) * __builtin_amdgcn_logf(p0);
        R.l2[rt] += (f0 + i < S.N && !(MASK && x < 0.f)) ? v : 0.f;
      }
  }
}

// TFP Normal(mu, sc).log_prob(h) with the raw v_rcp / v_log (sc >= 1e-6 is
// normal: no denormal scaling needed)
__device__ __forceinline__ float mg_normal_logp(float h, float mu, float sc) {
  const float rs = frcp(sc);
  const float z = h * rs - mu * rs;
  return -0.5f * (z * z) - (kHalfLog2Pi + kLn2 * __builtin_amdgcn_logf(sc));
}

// Head stage epilogue.  Lane groups g hold, for quad q = 2t + (g >> 1), the mu
// quad (g even) or the zs quad (g odd).  v_permlane16_swap exchanges the odd
// 16-lane rows of its first operand with the even rows of its second, so
// after swap(acc.x, acc.z) and swap(acc.y, acc.w) every lane holds (mu, zs)
// of its own two latent columns j = 4q + 2(g & 1) + {0, 1} -- no selects.
template <int RT, int ACT>
__device__ __forceinline__ void mg_head(const MgLaunch& L, const MgStage& S, int t, uint64_t base,
                                        const mg_f32x4 (&acc)[RT], MgRows<RT>& R) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int q = 2 * t + (g >> 1);
  const int j0 = 4 * q + 2 * (g & 1);
  const int d = S.d;
  const MgBuf H = mg_buf<RT>(L, S.out_buf);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const auto p0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][0]), __float_as_uint(acc[rt][2]),
                                                     false, false);
    const auto p1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][1]), __float_as_uint(acc[rt][3]),
                                                     false, false);
    const float mu[2] = {__uint_as_float(p0[0]), __uint_as_float(p1[0])};
    const float zs[2] = {__uint_as_float(p0[1]), __uint_as_float(p1[1])};
    const int row = rt * 16 + r;
    // computed on every lane (branch-free); columns past d are masked
    if (ACT == MG_SAMPLE) {
      const int row0 = blockIdx.x * 16 * RT;
      const int grow = row0 + min(row, L.rows - 1 - row0);      // global row (clamped into the chunk)
      float2 e;
      if (L.eps[S.layer]) {
        // injected [k][N][d] noise; columns past d read 0 (masked below anyway)
        const size_t eo = ((size_t)(L.eps_s0 + grow % L.kS) * L.eps_N + (L.eps_i0 + grow / L.kS)) * d;
        const float* ep = L.eps[S.layer] + eo;
        e.x = j0 < d ? ep[j0] : 0.f;
        e.y = j0 + 1 < d ? ep[j0 + 1] : 0.f;
      } else {
        e = philox_normal2(L.seed, base, (unsigned)grow, (unsigned)S.layer, (unsigned)q, (g & 1) != 0);
      }
      float hv[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int j = j0 + c;
        const float sc = fexp(zs[c]) + kScaleEps;
        const float h = (c == 0 ? e.x : e.y) * sc + mu[c];
        float contrib = -mg_normal_logp(h, mu[c], sc);
        if (S.stdnormal) contrib += -0.5f * (h * h) - kHalfLog2Pi;
        R.lw[rt] += j < d ? contrib : 0.f;
        hv[c] = j < d ? h : (j == d ? 1.f : 0.f);
      }
      mg_bf16x2 vh, vl;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        vh[c] = (__bf16)hv[c];
        vl[c] = (__bf16)(hv[c] - (float)vh[c]);
      }
      *reinterpret_cast<mg_bf16x2*>(H.hi + row * H.ld + j0) = vh;
      *reinterpret_cast<mg_bf16x2*>(H.lo + row * H.ld + j0) = vl;
    } else {
      const mg_bf16x2 th = *reinterpret_cast<const mg_bf16x2*>(H.hi + row * H.ld + j0);
      const mg_bf16x2 tl = *reinterpret_cast<const mg_bf16x2*>(H.lo + row * H.ld + j0);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float sc = fexp(zs[c]) + kScaleEps;
        const float v = mg_normal_logp((float)th[c] + (float)tl[c], mu[c], sc);
        R.lw[rt] += j0 + c < d ? v : 0.f;
      }
    }
    __builtin_amdgcn_sched_barrier(0);     // one row tile at a time (register pressure)
  }
}

// TANH epilogue: features f0..f0+3 of row rt*16 + r
template <int RT>
__device__ __forceinline__ void mg_store_tanh(const MgBuf& OUT, const MgStage& S, int t, const mg_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int f0 = t * 16 + 4 * g;
  if (f0 >= S.N) return;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float v[4];
    mg_bf16x4 vh, vl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = mg_tanh(acc[rt][i]);
      vh[i] = (__bf16)v[i];
      vl[i] = (__bf16)(v[i] - (float)vh[i]);
    }
    const int o = (rt * 16 + r) * OUT.ld + f0;
    if (f0 + 3 < S.N) {
      *reinterpret_cast<mg_bf16x4*>(OUT.hi + o) = vh;
      *reinterpret_cast<mg_bf16x4*>(OUT.lo + o) = vl;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (f0 + i < S.N) {
          OUT.hi[o + i] = vh[i];
          OUT.lo[o + i] = vl[i];
        }
    }
  }
}

// Barrier between stages.  The stages exchange data through LDS only (global
// memory: read-only inputs, and the log weights stored after the last stage),
// so the release / acquire cover LDS alone: requested weight fragments and
// pixels stay in flight across it (a full __syncthreads would wait for them).
__device__ __forceinline__ void mg_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// One Dense stage of gen_kernel / post_kernel: the loop over the column tiles
// of a wave (wave w owns the tiles w, w + NW, ...) from buffer S.in_buf.  Per
// tile the MFMAs run over the whole K, then EPI::run(L, S, OUT, t, acc, a...)
// consumes the accumulators (EPI: a tag type, so the epilogue is a plain
// forceinline function taking its context by reference; OUT: buffer out_buf).
// When the whole K fits one fetch (ldk <= 256) the first MG_PF steps of the
// wave's next tile are requested during the current tile's MFMAs (mg_mma).
// Call it from the kernel's stage switch directly and keep the wide-K fetch
// written in place (not mg_fetch): the register allocation of the two
// kernels depends on both.
template <int RT, int NW, class EPI, class LT, class ST, class... A>
__device__ __forceinline__ void mg_tiles(const LT& L, const ST& S, int out_buf, A&&... a) {
  const int wave = threadIdx.x >> 6;
  const int ntile = (S.N + 15) >> 4;
  const MgBuf IN = mg_buf<RT>(L, S.in_buf);
  const MgBuf OUT = mg_buf<RT>(L, out_buf);
  const __amdgpu_buffer_rsrc_t rh = buf_rsrc(S.Whi, S.W_bytes), rl = buf_rsrc(S.Wlo, S.W_bytes);
  if (S.ldk <= 32 * MG_KS) {
    MgFrag f;
    const int ns = S.ldk >> 5;
    if (wave < ntile) {
      const unsigned vb = mg_frag_base(S, wave, 0);
#pragma unroll
      for (int u = 0; u < MG_PF; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
    }
    for (int t = wave; t < ntile; t += NW) {
      const int tn = t + NW;
      const unsigned vb = mg_frag_base(S, t, 0);
#pragma unroll
      for (int u = MG_PF; u < MG_KS; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
      mg_f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
      mg_mma<RT>(IN, 0, min(MG_KS, ns), f, acc, rh, rl, tn < ntile, mg_frag_base(S, tn, 0), ns);
      EPI::run(L, S, OUT, t, acc, a...);
    }
  } else {
    // wide K: 256-deep fetches, no prefetch across tiles
    for (int t = wave; t < ntile; t += NW) {
      mg_f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < S.ldk; k0 += 32 * MG_KS) {
        MgFrag f;
        const unsigned vb = mg_frag_base(S, t, k0);
        const int ns = (S.ldk - k0) >> 5;
#pragma unroll
        for (int u = 0; u < MG_KS; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
        mg_mma<RT>(IN, k0, min(MG_KS, ns), f, acc, rh, rl, false, kOOB, 0);
      }
      EPI::run(L, S, OUT, t, acc, a...);
    }
  }
}

// ---- score_kernel's stage kinds (ScAct): operand requests and epilogues
// defined in iwae_score.hip, compiled into its instantiations only (the
// branches below that name them are discarded for MgAct stage kinds).
// score_kernel's rows: lq the encoder density heads' sums (lw: the prior heads')
template <int RT>
struct ScRows : MgRows<RT> {
  float lq[RT];
};
// a tile's density targets (none for the stage kinds of mega_fwd_kernel)
template <int RT, bool HAVE>
struct ScTargets {};
template <int RT>
struct ScTargets<RT, true> {
  float2 v[RT];
};

template <int RT, int ACT>
__device__ __forceinline__ void sc_operands(const ScLaunch& L, const MgStage& S, int t, const ScRows<RT>& R,
                                            float4 (&xv)[RT], ScTargets<RT, true>& T);
template <int RT, int ACT, bool MASK>
__device__ __forceinline__ void sc_epilogue(const ScLaunch& L, const MgStage& S, int t, const mg_f32x4 (&acc)[RT],
                                            const float4 (&xv)[RT], const ScTargets<RT, true>& T, ScRows<RT>& R);

// ---- mega_fwd_kernel's and score_kernel's own tile loop.  mg_tile / mg_dense
// are mg_tiles' two branches written out with these kernels' operand requests
// (pixels, density targets) ahead of the MFMAs and their epilogues in place.
// They have not moved onto a shared loop: an attempt through one with an
// operand hook changed the device assembly of both kernels throughout, and
// the NLL kernel's tuned code is not traded for these 40 lines.  A change to
// the loop's structure is made here and in mg_tiles.
//
// One column tile: x operands (Bernoulli stage) requested first, MFMAs over
// the whole K, epilogue.
template <int RT, int ACT, bool MASK, class LT, class RW>
__device__ __forceinline__ void mg_tile(const LT& L, const MgStage& S, const MgBuf& IN, const MgBuf& OUT,
                                        int t, MgFrag& f, __amdgpu_buffer_rsrc_t ph, __amdgpu_buffer_rsrc_t pl,
                                        bool pf, unsigned pf_vb, int pf_ns, uint64_t base, RW& R) {
  const int g = (threadIdx.x & 63) >> 4;
  float4 xv[RT];
  if (ACT == MG_BERN) {
    const __amdgpu_buffer_rsrc_t rx = buf_rsrc(L.x);
    const int f0 = t * 16 + 4 * g;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) xv[rt] = bld4(rx, f0 < S.N ? R.xoff[rt] + (unsigned)f0 * 4u : kOOB);
  }
  ScTargets<RT, (ACT >= MG_DENSQ)> tg;
  if constexpr (ACT >= MG_DENSQ) sc_operands<RT, ACT>(L, S, t, R, xv, tg);
  mg_f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
  mg_mma<RT>(IN, 0, min(MG_KS, S.ldk >> 5), f, acc, ph, pl, pf, pf_vb, pf_ns);
  if constexpr (ACT >= MG_DENSQ) sc_epilogue<RT, ACT, MASK>(L, S, t, acc, xv, tg, R);
  else if (ACT == MG_TANH) mg_store_tanh<RT>(OUT, S, t, acc);
  else if (ACT == MG_BERN) mg_bern<RT, MASK>(L, S, t, acc, xv, R);
  else mg_head<RT, ACT>(L, S, t, base, acc, R);
}

// One Dense stage.  Wave w owns the column tiles w, w + 8, ...; when the whole
// K fits one fetch (ldk <= 256) the first MG_PF steps of the wave's next tile
// are requested during the current tile's MFMAs (mg_mma).
template <int RT, int ACT, int NW, bool MASK, class LT, class RW>
__device__ __forceinline__ void mg_dense(const LT& L, const MgStage& S, uint64_t base, RW& R) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntile = (S.N + 15) >> 4;
  const MgBuf IN = mg_buf<RT>(L, S.in_buf);
  const MgBuf OUT = mg_buf<RT>(L, ACT == MG_TANH ? S.out_buf : S.in_buf);
  const __amdgpu_buffer_rsrc_t rh = buf_rsrc(S.Whi, S.W_bytes), rl = buf_rsrc(S.Wlo, S.W_bytes);
  if (S.ldk <= 32 * MG_KS) {
    MgFrag f;
    const int ns = S.ldk >> 5;
    if (wave < ntile) {
      const unsigned vb = mg_frag_base(S, wave, 0);
#pragma unroll
      for (int u = 0; u < MG_PF; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
    }
    for (int t = wave; t < ntile; t += NW) {
      const int tn = t + NW;
      const unsigned vb = mg_frag_base(S, t, 0);
#pragma unroll
      for (int u = MG_PF; u < MG_KS; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
      mg_tile<RT, ACT, MASK>(L, S, IN, OUT, t, f, rh, rl, tn < ntile, mg_frag_base(S, tn, 0), ns, base, R);
    }
  } else {
    // wide K: 256-deep fetches, no prefetch across tiles
    const int g = lane >> 4;
    for (int t = wave; t < ntile; t += NW) {
      float4 xv[RT];
      if (ACT == MG_BERN) {
        const __amdgpu_buffer_rsrc_t rx = buf_rsrc(L.x);
        const int f0 = t * 16 + 4 * g;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) xv[rt] = bld4(rx, f0 < S.N ? R.xoff[rt] + (unsigned)f0 * 4u : kOOB);
      }
      ScTargets<RT, (ACT >= MG_DENSQ)> tg;
      if constexpr (ACT >= MG_DENSQ) sc_operands<RT, ACT>(L, S, t, R, xv, tg);
      mg_f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < S.ldk; k0 += 32 * MG_KS) {
        MgFrag f;
        mg_fetch(S, rh, rl, t, k0, f);
        mg_mma<RT>(IN, k0, min(MG_KS, (S.ldk - k0) >> 5), f, acc, rh, rl, false, kOOB, 0);
      }
      if constexpr (ACT >= MG_DENSQ) sc_epilogue<RT, ACT, MASK>(L, S, t, acc, xv, tg, R);
      else if (ACT == MG_TANH) mg_store_tanh<RT>(OUT, S, t, acc);
      else if (ACT == MG_BERN) mg_bern<RT, MASK>(L, S, t, acc, xv, R);
      else mg_head<RT, ACT>(L, S, t, base, acc, R);
    }
  }
}

}  // namespace iwae
