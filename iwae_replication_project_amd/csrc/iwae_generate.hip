// Fused generation from the prior (Decoder.generate_x, F:107-F:119, and
// ancestral sampling with h_L ~ N(0, I)), gfx950.
//
// One workgroup of 8 waves owns 16*RT generated rows and runs the whole
// decoder on them, activations resident in LDS:
//
//   h_L of each row: the caller's, injected eps * 1 + 0, or Philox normals
//   per prior layer j: l1 tanh, l2 tanh, head -> h_{L-2-j} = eps (exp(zs) + 1e-6) + mu   (F:113-F:114)
//   output MLP: tanh, tanh, Dense(x_dim) -> p = sigmoid(l) (1 - 1e-6) + 1e-7            (F:101-F:102)
//   p stored, and / or x = (u < p) drawn and stored
//
// The machinery is mega_fwd_kernel's (iwae_mega.hip), copied here so that
// kernel's code size and register budget stay as tuned: bf16x3 products on
// v_mfma_f32_16x16x32_bf16, the weights as the A operand streamed from the
// fragment-major FX copies, the activations as the B operand read from LDS
// where they are kept as two bf16 planes (hi, lo) with row strides of 8 mod 16
// dwords, the ones column of the next reader written by gn_pad, LDS-only
// barriers between stages, head rows permuted into [mu 4q..4q+3 | zs 4q..4q+3]
// groups and exchanged with v_permlane16_swap.  No log densities are
// evaluated.  Noise: the shared Philox function with (row = generated row,
// layer id, column quad), so the layer-wise path draws the identical stream.
// Deterministic: no float atomics, each output written by exactly one lane.
#include "iwae_kernels.h"

namespace iwae {

typedef float gn_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 gn_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gn_bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 gn_bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned gn_u32x4 __attribute__((ext_vector_type(4)));

constexpr int GN_WAVES = 8;          // waves per workgroup
constexpr int GN_KS = 8;             // k steps of 32 per weight fetch (256 k)
constexpr int GN_PF = 2;             // steps of the next column tile requested during the current one

extern __shared__ __attribute__((aligned(16))) float gns[];

__device__ __forceinline__ gn_bf16x8 gn_as_bf16x8(gn_u32x4 v) { return __builtin_bit_cast(gn_bf16x8, v); }

// LDS buffer b: hi plane at bf16 offset off, lo plane at off + R * ld
struct GnBuf {
  __bf16* hi; __bf16* lo; int ld;
};
template <int RT>
__device__ __forceinline__ GnBuf gn_buf(const GnLaunch& L, int b) {
  __bf16* base = reinterpret_cast<__bf16*>(gns);
  GnBuf B;
  B.ld = L.buf_ld[b];
  B.hi = base + L.buf_off[b];
  B.lo = B.hi + 16 * RT * B.ld;
  return B;
}

// 1 - 2 / (exp(2x) + 1): absolute error ~1 ulp of 1 (mega_fwd_kernel's tanh)
__device__ __forceinline__ float gn_tanh(float x) {
  return __builtin_fmaf(-2.f, frcp(fexp(2.f * x) + 1.f), 1.f);
}

// ones column (K - 1 of the next reader) and zero padding of columns [width, next_k)
template <int RT>
__device__ __forceinline__ void gn_pad(const GnBuf& B, int width, int next_k) {
  constexpr int TPR = (GN_WAVES * 64) / (16 * RT);    // threads per row
  const int row = threadIdx.x / TPR;
  for (int col = width + threadIdx.x % TPR; col < next_k; col += TPR) {
    B.hi[row * B.ld + col] = (__bf16)(col == width ? 1.f : 0.f);
    B.lo[row * B.ld + col] = (__bf16)0.f;
  }
}

struct GnFrag {
  gn_bf16x8 h[GN_KS], l[GN_KS];
};

// Byte offset (hi and lo planes alike) of this lane's fragment of column tile
// t at k0 in the fragment-major copy (FX: [tile][k step][64 lanes][8], head
// rows already permuted, padding rows zero), or kOOB
__device__ __forceinline__ unsigned gn_frag_base(const GnStage& S, int t, int k0) {
  const int lane = threadIdx.x & 63;
  const int ntile = (S.N + 15) >> 4;
  return t < ntile ? (unsigned)(((t * (S.ldk >> 5) + (k0 >> 5)) * 64 + lane) * 16) : kOOB;
}
// k step u of the fragment: 1 KiB further
__device__ __forceinline__ void gn_fetch_step(__amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl, unsigned vb,
                                              int u, int ns, GnFrag& f) {
  if (u >= ns) return;
  f.h[u] = gn_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rh, vb, 1024 * u, 0));
  f.l[u] = gn_as_bf16x8(__builtin_amdgcn_raw_buffer_load_b128(rl, vb, 1024 * u, 0));
}

// acc[rt] += F-tile . IN[rows of rt][k0 .. k0 + 32 ns) (bf16x3).  With pf
// (uniform) the fragments of the first GN_PF steps are re-requested for the
// wave's next column tile right after their last MFMA (one register set).
template <int RT>
__device__ __forceinline__ void gn_mma(const GnBuf& IN, int k0, int ns, GnFrag& f, gn_f32x4 (&acc)[RT],
                                       __amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl, bool pf, unsigned pf_vb,
                                       int pf_ns) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  // chunks of (k step u, row-tile pair p); the activation fragments of the next
  // chunk are read from LDS while this chunk's MFMAs run (two register sets)
  constexpr int RH = RT < 2 ? RT : 2;
  constexpr int NP = RT / RH;
  constexpr int NC = GN_KS * NP;
  gn_bf16x8 ah[2][RH], al[2][RH];
  auto rd = [&](int c, int b) {
    const int u = c / NP, p = c % NP;
#pragma unroll
    for (int i = 0; i < RH; ++i) {
      const int ao = ((p * RH + i) * 16 + r) * IN.ld + k0 + 32 * u + 8 * g;
      ah[b][i] = *reinterpret_cast<const gn_bf16x8*>(IN.hi + ao);
      al[b][i] = *reinterpret_cast<const gn_bf16x8*>(IN.lo + ao);
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
    if (p == NP - 1 && u < GN_PF && pf) gn_fetch_step(rh, rl, pf_vb, u, pf_ns, f);
  }
}

// TANH epilogue: features f0..f0+3 of row rt*16 + r
template <int RT>
__device__ __forceinline__ void gn_store_tanh(const GnBuf& OUT, const GnStage& S, int t, const gn_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int f0 = t * 16 + 4 * g;
  if (f0 >= S.N) return;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float v[4];
    gn_bf16x4 vh, vl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = gn_tanh(acc[rt][i]);
      vh[i] = (__bf16)v[i];
      vl[i] = (__bf16)(v[i] - (float)vh[i]);
    }
    const int o = (rt * 16 + r) * OUT.ld + f0;
    if (f0 + 3 < S.N) {
      *reinterpret_cast<gn_bf16x4*>(OUT.hi + o) = vh;
      *reinterpret_cast<gn_bf16x4*>(OUT.lo + o) = vl;
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

// Head epilogue (F:113-F:114).  Lane groups g hold, for quad q = 2t + (g >> 1),
// the mu quad (g even) or the zs quad (g odd); after swap(acc.x, acc.z) and
// swap(acc.y, acc.w) every lane holds (mu, zs) of its own two latent columns
// j = 4q + 2(g & 1) + {0, 1}.  h goes to LDS (split, with the ones column at d)
// and, when asked for, as f32 to the caller's buffer (rows below n only).
template <int RT>
__device__ __forceinline__ void gn_head(const GnLaunch& L, const GnStage& S, int t, uint64_t base,
                                        const gn_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int q = 2 * t + (g >> 1);
  const int j0 = 4 * q + 2 * (g & 1);
  const int d = S.d;
  const int row0 = blockIdx.x * 16 * RT;
  const int nrows = min(16 * RT, L.n - row0);
  const GnBuf H = gn_buf<RT>(L, S.out_buf);
  // the workgroup's rows of the injected noise / the caller's latent buffer
  // through buffer resources (32-bit offsets; a masked lane gets kOOB: its
  // load reads 0, its store is dropped)
  const unsigned wg_bytes = (unsigned)(nrows * d) * 4u;
  const __amdgpu_buffer_rsrc_t re = buf_rsrc(S.eps ? S.eps + (size_t)row0 * d : nullptr, S.eps ? wg_bytes : 0u);
  const __amdgpu_buffer_rsrc_t ro = buf_rsrc(S.h_out ? S.h_out + (size_t)row0 * d : nullptr, S.h_out ? wg_bytes : 0u);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const auto p0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][0]), __float_as_uint(acc[rt][2]),
                                                     false, false);
    const auto p1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][1]), __float_as_uint(acc[rt][3]),
                                                     false, false);
    const float mu[2] = {__uint_as_float(p0[0]), __uint_as_float(p1[0])};
    const float zs[2] = {__uint_as_float(p0[1]), __uint_as_float(p1[1])};
    const int row = rt * 16 + r;
    const bool live = row < nrows;
    const int rowc = min(row, nrows - 1);                  // clamped for loads
    float2 e;
    if (S.eps) {
      e.x = bld1(re, j0 < d ? (unsigned)(rowc * d + j0) * 4u : kOOB);
      e.y = bld1(re, j0 + 1 < d ? (unsigned)(rowc * d + j0 + 1) * 4u : kOOB);
    } else {
      e = philox_normal2(L.seed, base, (unsigned)(row0 + rowc), (unsigned)S.layer, (unsigned)q, (g & 1) != 0);
    }
    float hv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = j0 + c;
      const float sc = fexp(zs[c]) + kScaleEps;
      const float h = (c == 0 ? e.x : e.y) * sc + mu[c];
      hv[c] = j < d ? h : (j == d ? 1.f : 0.f);
      if (S.h_out)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h), ro,
                                              live && j < d ? (unsigned)(row * d + j) * 4u : kOOB, 0, 0);
    }
    gn_bf16x2 vh, vl;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      vh[c] = (__bf16)hv[c];
      vl[c] = (__bf16)(hv[c] - (float)vh[c]);
    }
    *reinterpret_cast<gn_bf16x2*>(H.hi + row * H.ld + j0) = vh;
    *reinterpret_cast<gn_bf16x2*>(H.lo + row * H.ld + j0) = vl;
    __builtin_amdgcn_sched_barrier(0);     // one row tile at a time (register pressure)
  }
}

// Output epilogue: p = sigmoid(acc) (1 - 1e-6) + 1e-7 (F:101-F:102) of features
// f0..f0+3 of one row per lane: one 16-byte store into probs, and / or the
// Bernoulli draw x = (u < p) into pixels.  The workgroup's rows of probs,
// pixels and u are addressed through buffer resources (32-bit offsets, one
// descriptor per array): rows past n and columns past x_dim get kOOB, so they
// are never stored.
__device__ __forceinline__ void gn_store4(__amdgpu_buffer_rsrc_t rs, unsigned off, bool full, int f0, int xdim,
                                          const float (&v)[4]) {
  if (full) {
    const gn_u32x4 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, off, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), rs, f0 + i < xdim ? off + 4u * i : kOOB, 0, 0);
  }
}
template <int RT>
__device__ __forceinline__ void gn_out(const GnLaunch& L, const GnStage& S, int t, uint64_t base,
                                       const gn_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int f0 = t * 16 + 4 * g;
  const int xdim = S.N;
  const int row0 = blockIdx.x * 16 * RT;
  const int nrows = min(16 * RT, L.n - row0);
  if (f0 >= xdim) return;
  const bool full = f0 + 3 < xdim;
  const __amdgpu_buffer_rsrc_t rp = buf_rsrc(L.probs ? L.probs + (size_t)row0 * L.ld_probs : nullptr,
                                             L.probs ? (unsigned)(nrows * L.ld_probs) * 4u : 0u);
  const __amdgpu_buffer_rsrc_t rx = buf_rsrc(L.pixels ? L.pixels + (size_t)row0 * L.ld_pixels : nullptr,
                                             L.pixels ? (unsigned)(nrows * L.ld_pixels) * 4u : 0u);
  const __amdgpu_buffer_rsrc_t ru = buf_rsrc(L.u ? L.u + (size_t)row0 * xdim : nullptr,
                                             L.u ? (unsigned)(nrows * xdim) * 4u : 0u);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = rt * 16 + r;
    const bool live = row < nrows;
    float p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = __builtin_fmaf(frcp(1.f + fexp(-acc[rt][i])), kProbScale, kProbShift);
    if (L.probs) gn_store4(rp, live ? (unsigned)(row * L.ld_probs + f0) * 4u : kOOB, full, f0, xdim, p);
    if (L.pixels) {
      float4 u4;
      if (L.u) {
        // columns past x_dim read the next row's values or 0: never stored
        const unsigned uo = live ? (unsigned)(row * xdim + f0) * 4u : kOOB;
        u4 = make_float4(bld1(ru, uo), bld1(ru, uo + 4u), bld1(ru, uo + 8u), bld1(ru, uo + 12u));
      } else {
        u4 = philox_uniform4(L.seed, base, (unsigned)(row0 + row), (unsigned)L.pix_layer, (unsigned)(f0 >> 2));
      }
      float x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = f4_at(u4, i) < p[i] ? 1.f : 0.f;
      gn_store4(rx, live ? (unsigned)(row * L.ld_pixels + f0) * 4u : kOOB, full, f0, xdim, x);
    }
    __builtin_amdgcn_sched_barrier(0);     // one row tile at a time (register pressure)
  }
}

// Barrier between stages: the stages exchange data through LDS only, so the
// release / acquire cover LDS alone and requested weight fragments stay in
// flight across it.
__device__ __forceinline__ void gn_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int RT, int ACT>
__device__ __forceinline__ void gn_epilogue(const GnLaunch& L, const GnStage& S, const GnBuf& OUT, int t,
                                            uint64_t base, const gn_f32x4 (&acc)[RT]) {
  if (ACT == GN_TANH) gn_store_tanh<RT>(OUT, S, t, acc);
  else if (ACT == GN_OUT) gn_out<RT>(L, S, t, base, acc);
  else gn_head<RT>(L, S, t, base, acc);
}

// One Dense stage.  Wave w owns the column tiles w, w + 8, ...; when the whole
// K fits one fetch (ldk <= 256) the first GN_PF steps of the wave's next tile
// are requested during the current tile's MFMAs (gn_mma).
template <int RT, int ACT>
__device__ __forceinline__ void gn_dense(const GnLaunch& L, const GnStage& S, uint64_t base) {
  const int wave = threadIdx.x >> 6;
  const int ntile = (S.N + 15) >> 4;
  const GnBuf IN = gn_buf<RT>(L, S.in_buf);
  const GnBuf OUT = gn_buf<RT>(L, ACT == GN_OUT ? S.in_buf : S.out_buf);
  const __amdgpu_buffer_rsrc_t rh = buf_rsrc(S.Whi, S.W_bytes), rl = buf_rsrc(S.Wlo, S.W_bytes);
  if (S.ldk <= 32 * GN_KS) {
    GnFrag f;
    const int ns = S.ldk >> 5;
    if (wave < ntile) {
      const unsigned vb = gn_frag_base(S, wave, 0);
#pragma unroll
      for (int u = 0; u < GN_PF; ++u) gn_fetch_step(rh, rl, vb, u, ns, f);
    }
    for (int t = wave; t < ntile; t += GN_WAVES) {
      const int tn = t + GN_WAVES;
      const unsigned vb = gn_frag_base(S, t, 0);
#pragma unroll
      for (int u = GN_PF; u < GN_KS; ++u) gn_fetch_step(rh, rl, vb, u, ns, f);
      gn_f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
      gn_mma<RT>(IN, 0, min(GN_KS, ns), f, acc, rh, rl, tn < ntile, gn_frag_base(S, tn, 0), ns);
      gn_epilogue<RT, ACT>(L, S, OUT, t, base, acc);
    }
  } else {
    // wide K: 256-deep fetches, no prefetch across tiles
    for (int t = wave; t < ntile; t += GN_WAVES) {
      gn_f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (gn_f32x4){0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < S.ldk; k0 += 32 * GN_KS) {
        GnFrag f;
        const unsigned vb = gn_frag_base(S, t, k0);
        const int ns = (S.ldk - k0) >> 5;
#pragma unroll
        for (int u = 0; u < GN_KS; ++u) gn_fetch_step(rh, rl, vb, u, ns, f);
        gn_mma<RT>(IN, k0, min(GN_KS, ns), f, acc, rh, rl, false, kOOB, 0);
      }
      gn_epilogue<RT, ACT>(L, S, OUT, t, base, acc);
    }
  }
}

template <int RT>
__global__ __launch_bounds__(GN_WAVES * 64) void gen_kernel(GnLaunch L) {
  constexpr int R = 16 * RT;
  constexpr int TPR = (GN_WAVES * 64) / R;       // threads per row in the prologue
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, L.n - row0);
  const uint64_t base = *L.rng_base;
  // ---- prologue: the top latent h_L of each row, split, with its ones column
  {
    const int d = L.d_top;
    const GnBuf H = gn_buf<RT>(L, L.top_buf);
    const int rr = t / TPR, sub = t - rr * TPR;
    const bool live = rr < nrows;
    const int rg = row0 + min(rr, nrows - 1);
    const float* src = L.h_top ? L.h_top : L.eps_top;      // eps * 1 + 0 is eps
    if (src) src += (size_t)rg * d;
    for (int gq = sub; 4 * gq < L.top_next_k; gq += TPR) {
      float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * gq < d) {
        if (src) {
          const int j = 4 * gq;
          e4 = make_float4(src[j], src[min(j + 1, d - 1)], src[min(j + 2, d - 1)], src[min(j + 3, d - 1)]);
        } else {
          e4 = philox_normal4(L.seed, base, (unsigned)rg, (unsigned)L.top_layer, (unsigned)gq);
        }
      }
      gn_bf16x4 vh, vl;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * gq + q;
        const float hv = j < d ? f4_at(e4, q) : (j == d ? 1.f : 0.f);
        if (L.top_out && live && j < d) L.top_out[(size_t)rg * d + j] = hv;
        vh[q] = (__bf16)hv;
        vl[q] = (__bf16)(hv - (float)vh[q]);
      }
      *reinterpret_cast<gn_bf16x4*>(H.hi + rr * H.ld + 4 * gq) = vh;
      *reinterpret_cast<gn_bf16x4*>(H.lo + rr * H.ld + 4 * gq) = vl;
    }
  }
  gn_lds_barrier();

  for (int s = 0; s < L.nst; ++s) {
    const GnStage& S = L.st[s];
    if (S.act == GN_TANH) gn_pad<RT>(gn_buf<RT>(L, S.out_buf), S.N, S.next_k);
    else if (S.act == GN_HEAD) gn_pad<RT>(gn_buf<RT>(L, S.out_buf), S.d, S.next_k);
    switch (S.act) {     // one instantiation per stage kind: one epilogue per tile loop
      case GN_TANH: gn_dense<RT, GN_TANH>(L, S, base); break;
      case GN_HEAD: gn_dense<RT, GN_HEAD>(L, S, base); break;
      default: gn_dense<RT, GN_OUT>(L, S, base); break;
    }
    gn_lds_barrier();
  }

  // ---- every workgroup has read the Philox base: the last one to arrive
  // advances it (integer ticket, agent-scope release / acquire)
  __syncthreads();
  if (t == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const unsigned tk = __hip_atomic_fetch_add(L.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      L.rng_base[1] = base;
      L.rng_base[0] = base + 1;
      *L.ticket = 0u;
    }
  }
}

hipError_t launch_gen(hipStream_t st, const GnLaunch& L, int rt, size_t lds_bytes) {
  if (L.n <= 0) return hipSuccess;
  const int R = 16 * rt;
  const dim3 grid((L.n + R - 1) / R), block(GN_WAVES * 64);
  switch (rt) {
    case 1: hipLaunchKernelGGL(gen_kernel<1>, grid, block, lds_bytes, st, L); break;
    case 2: hipLaunchKernelGGL(gen_kernel<2>, grid, block, lds_bytes, st, L); break;
    case 4: hipLaunchKernelGGL(gen_kernel<4>, grid, block, lds_bytes, st, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t gen_setup_attributes() {
  const void* fns[] = {(const void*)gen_kernel<1>, (const void*)gen_kernel<2>, (const void*)gen_kernel<4>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace iwae
