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
// The chain machinery is the one shared with mega_fwd_kernel, score_kernel and
// post_kernel (iwae_mega_dev.h): bf16x3 products on the bf16 16x16x32 MFMA, the
// weights as the A operand streamed from the fragment-major FX copies, the
// activations as the B operand read from LDS where they are kept as two bf16
// planes (hi, lo) with row strides of 8 mod 16 dwords, the ones column of the
// next reader written by mg_pad, LDS-only barriers between stages, the loop
// over a wave's column tiles (mg_tiles).  This file holds what is generation's
// own: the prologue, the head and output epilogues and the kernel body.  Head
// rows are permuted into [mu 4q..4q+3 | zs 4q..4q+3] groups and exchanged with
// v_permlane16_swap.  No log densities are evaluated.  Noise: the shared
// Philox function with (row = generated row, layer id, column quad), so the
// layer-wise path draws the identical stream.  Deterministic: no float
// atomics, each output written by exactly one lane.
#include "iwae_mega_dev.h"

namespace iwae {

// Head epilogue (F:113-F:114).  Lane groups g hold, for quad q = 2t + (g >> 1),
// the mu quad (g even) or the zs quad (g odd); after swap(acc.x, acc.z) and
// swap(acc.y, acc.w) every lane holds (mu, zs) of its own two latent columns
// j = 4q + 2(g & 1) + {0, 1}.  h goes to LDS (split, with the ones column at d)
// and, when asked for, as f32 to the caller's buffer (rows below n only).
template <int RT>
__device__ __forceinline__ void gn_head(const GnLaunch& L, const GnStage& S, int t, uint64_t base,
                                        const mg_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int q = 2 * t + (g >> 1);
  const int j0 = 4 * q + 2 * (g & 1);
  const int d = S.d;
  const int row0 = blockIdx.x * 16 * RT;
  const int nrows = min(16 * RT, L.n - row0);
  const MgBuf H = mg_buf<RT>(L, S.out_buf);
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
    mg_bf16x2 vh, vl;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      vh[c] = (__bf16)hv[c];
      vl[c] = (__bf16)(hv[c] - (float)vh[c]);
    }
    *reinterpret_cast<mg_bf16x2*>(H.hi + row * H.ld + j0) = vh;
    *reinterpret_cast<mg_bf16x2*>(H.lo + row * H.ld + j0) = vl;
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
    const mg_u32x4 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, off, 0, 0);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), rs, f0 + i < xdim ? off + 4u * i : kOOB, 0, 0);
  }
}
template <int RT>
__device__ __forceinline__ void gn_out(const GnLaunch& L, const GnStage& S, int t, uint64_t base,
                                       const mg_f32x4 (&acc)[RT]) {
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

// The stage kind's epilogue, for the shared tile loop (mg_tiles)
template <int RT, int ACT>
struct GnEpi {
  static __device__ __forceinline__ void run(const GnLaunch& L, const GnStage& S, const MgBuf& OUT, int t,
                                             const mg_f32x4 (&acc)[RT], uint64_t base) {
    if (ACT == GN_TANH) mg_store_tanh<RT>(OUT, S, t, acc);
    else if (ACT == GN_OUT) gn_out<RT>(L, S, t, base, acc);
    else gn_head<RT>(L, S, t, base, acc);
  }
};

template <int RT>
__global__ __launch_bounds__(MG_WAVES * 64) void gen_kernel(GnLaunch L) {
  constexpr int R = 16 * RT;
  constexpr int TPR = (MG_WAVES * 64) / R;       // threads per row in the prologue
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, L.n - row0);
  const uint64_t base = *L.rng_base;
  // ---- prologue: the top latent h_L of each row, split, with its ones column
  {
    const int d = L.d_top;
    const MgBuf H = mg_buf<RT>(L, L.top_buf);
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
      mg_bf16x4 vh, vl;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * gq + q;
        const float hv = j < d ? f4_at(e4, q) : (j == d ? 1.f : 0.f);
        if (L.top_out && live && j < d) L.top_out[(size_t)rg * d + j] = hv;
        vh[q] = (__bf16)hv;
        vl[q] = (__bf16)(hv - (float)vh[q]);
      }
      *reinterpret_cast<mg_bf16x4*>(H.hi + rr * H.ld + 4 * gq) = vh;
      *reinterpret_cast<mg_bf16x4*>(H.lo + rr * H.ld + 4 * gq) = vl;
    }
  }
  mg_lds_barrier();

  for (int s = 0; s < L.nst; ++s) {
    const GnStage& S = L.st[s];
    if (S.act == GN_TANH) mg_pad<RT, MG_WAVES>(mg_buf<RT>(L, S.out_buf), S.N, S.next_k);
    else if (S.act == GN_HEAD) mg_pad<RT, MG_WAVES>(mg_buf<RT>(L, S.out_buf), S.d, S.next_k);
    switch (S.act) {     // one instantiation per stage kind: one epilogue per tile loop
      case GN_TANH: mg_tiles<RT, MG_WAVES, GnEpi<RT, GN_TANH>>(L, S, S.out_buf, base); break;
      case GN_HEAD: mg_tiles<RT, MG_WAVES, GnEpi<RT, GN_HEAD>>(L, S, S.out_buf, base); break;
      default: mg_tiles<RT, MG_WAVES, GnEpi<RT, GN_OUT>>(L, S, S.in_buf, base); break;
    }
    mg_lds_barrier();
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
  const dim3 grid((L.n + R - 1) / R), block(MG_WAVES * 64);
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
