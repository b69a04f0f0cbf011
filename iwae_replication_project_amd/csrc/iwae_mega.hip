// Fused k-sample forward for the NLL estimator (get_NLL, F:463-F:464, through
// get_log_weights F:327-F:351), gfx950.
//
// The layer-wise path streams every [rows x width] activation of a 2^20-row
// chunk through HBM (~0.85 GB per tensor).  Here one workgroup owns 16*RT
// sample rows and keeps them in LDS from the first sampled latent to the
// Bernoulli log-likelihood:
//
//   h1 ~ N(mu0, s0) of the row's image (Encoder.call F:58-F:60)
//   for each later encoder layer: l1 tanh, l2 tanh, head -> sample h_i, log q (F:66-F:73)
//   log N(h_L; 0, 1) (F:135-F:136)
//   decoder prior layers: l1 tanh, l2 tanh, head -> log p(h_t | h_src) (F:138-F:141)
//   output MLP: tanh, tanh, Dense(784) -> sigmoid, clamp, Bernoulli log-prob, sum (F:92-F:129)
//   log w = log p(h) + log p(x|h) - log q(h|x) (F:345-F:349)
//
// and writes one float per row.
//
// Products: bf16x3 on v_mfma_f32_16x16x32_bf16 (w_lo a_hi + w_hi a_lo + w_hi
// a_hi, f32 accumulate).  The weights are the MFMA A operand: each lane
// streams one output feature's pre-split F row (16-byte buffer loads, k
// contiguous) from L2, and the fragments of the wave's next column tile are
// requested step by step during the current tile's MFMAs (one register set).
// The activations are the B operand, read from LDS, so each lane's four
// accumulators are four consecutive output features of one sample row: the
// epilogue writes them as one 8-byte store per plane.
//
// Storage: every LDS activation is kept already split, as two bf16 planes
// (hi = bf16(v), lo = bf16(v - hi)) of the same [rows][ld] shape -- 4 bytes
// per value like f32, but an MFMA fragment is then two ds_read_b128 with no
// conversion, and each value is split once by the epilogue that produces it.
// Row strides are chosen by the host plan so the fragment reads are free of
// LDS bank conflicts (stride = 8 mod 16 dwords).
//
// Head stages (MG_SAMPLE / MG_PRIOR) have their weight rows permuted into
// groups of 8 features [mu 4q..4q+3 | zs 4q..4q+3]: the lanes holding mu_j
// and zs_j are 16 apart, exchange two values each, and sample h_j (or
// evaluate the prior density at h_j) in the epilogue -- no (mu | zs) buffer,
// no separate pass.  Noise is the same Philox4x32-10 stream (row, layer,
// column quad) as every other path.
#include "iwae_mega_dev.h"

namespace iwae {

// NW = 8: one 64-row workgroup per CU (LDS-bound).  NW = 4 with RT = 2: two
// independent 32-row workgroups per CU, whose weight waits, MFMA loops and
// epilogues interleave instead of running in lock step behind one barrier.
// MASK: the pixel-masked likelihood of iwae_impute; L.x is then the staged copy
// with -1 at the missing pixels (the first layer, run ahead of this kernel,
// read the copy with 0 there).  A compile-time variant: the unmasked
// instantiations are what they were.
template <int RT, int NW, bool MASK>
__global__ __launch_bounds__(NW * 64) void mega_fwd_kernel(MgLaunch L) {
  constexpr int R = 16 * RT;
  constexpr int TPR = (NW * 64) / R;            // threads per row in the prologue
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, L.rows - row0);
  float* logq = mgs + L.acc_off;
  float* logp = logq + R;
  float* red = logp + R;                        // [NW][R]
  const uint64_t base = L.rng_base ? *L.rng_base : 0ull;
  const int rr = t / TPR, sub = t - rr * TPR;   // prologue: row rr, lane group sub
  MG_TRACE(0)
  // ---- prologue: h1 = eps * s0 + mu0 of the row's image; log q(h1 | x)
  {
    const int d = L.d0;
    const MgBuf H = mg_buf<RT>(L, L.h0_buf);
    float aq = 0.f, ap = 0.f;
    const int rg = row0 + min(rr, nrows - 1);
    const float* Pp = L.P0 + (size_t)(rg / L.kS) * L.ldP0;
    // batches of 4 column quads per thread: every load of a batch (the image's
    // mu / zs, injected eps) is issued before the first is used -- one memory
    // round trip per batch instead of one per quad
    const float* ep = L.eps[0] ? L.eps[0] + ((size_t)(L.eps_s0 + rg % L.kS) * L.eps_N + (L.eps_i0 + rg / L.kS)) * d
                               : nullptr;
    for (int gq0 = sub; 4 * gq0 < L.h0_next_k; gq0 += 4 * TPR) {
      float mu[4][4], zs[4][4], ev[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jc = min(4 * (gq0 + i * TPR) + q, d - 1);      // clamped: always a valid address
          mu[i][q] = Pp[jc];
          zs[i][q] = Pp[d + jc];
          ev[i][q] = 0.f;
        }
      if (L.eps[0]) {                 // uniform: injected noise (parity runs)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int q = 0; q < 4; ++q) ev[i][q] = ep[min(4 * (gq0 + i * TPR) + q, d - 1)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gq = gq0 + i * TPR;
        if (4 * gq >= L.h0_next_k) break;
        float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (L.eps[0]) {
          const int j = 4 * gq;
          e4 = make_float4(j < d ? ev[i][0] : 0.f, j + 1 < d ? ev[i][1] : 0.f, j + 2 < d ? ev[i][2] : 0.f,
                           j + 3 < d ? ev[i][3] : 0.f);
        } else if (4 * gq < d) {
          e4 = philox_normal4(L.seed, base, (unsigned)rg, 0u, (unsigned)gq);
        }
        mg_bf16x4 vh, vl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = 4 * gq + q;
          float hv = 0.f;
          if (j < d) {
            const float sc = fexp(zs[i][q]) + kScaleEps;
            hv = f4_at(e4, q) * sc + mu[i][q];
            aq += mg_normal_logp(hv, mu[i][q], sc);
            ap += -0.5f * (hv * hv) - kHalfLog2Pi;
          } else if (j == d) {
            hv = 1.f;
          }
          vh[q] = (__bf16)hv;
          vl[q] = (__bf16)(hv - (float)vh[q]);
        }
        *reinterpret_cast<mg_bf16x4*>(H.hi + rr * H.ld + 4 * gq) = vh;
        *reinterpret_cast<mg_bf16x4*>(H.lo + rr * H.ld + 4 * gq) = vl;
      }
    }
    for (int o = TPR >> 1; o > 0; o >>= 1) {
      aq += __shfl_xor(aq, o);
      ap += __shfl_xor(ap, o);
    }
    if (sub == 0) {
      logq[rr] = aq;
      logp[rr] = L.h0_stdnormal ? ap : 0.f;
    }
  }
  MgRows<RT> Rw;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = min(rt * 16 + (lane & 15), nrows - 1);
    Rw.lw[rt] = 0.f;
    Rw.l2[rt] = 0.f;
    Rw.xoff[rt] = (unsigned)((row0 + row) / L.kS) * (unsigned)L.ldx * 4u;
  }
  mg_lds_barrier();
  MG_TRACE(1)

  for (int s = 0; s < L.nst; ++s) {
    const MgStage& S = L.st[s];
    MG_TRACE(2 + 3 * s)
    if (S.act == MG_TANH) mg_pad<RT, NW>(mg_buf<RT>(L, S.out_buf), S.N, S.next_k);
    else if (S.act == MG_SAMPLE) mg_pad<RT, NW>(mg_buf<RT>(L, S.out_buf), S.d, S.next_k);
    switch (S.act) {     // one instantiation per stage kind: one epilogue per tile loop
      case MG_TANH: mg_dense<RT, MG_TANH, NW, MASK>(L, S, base, Rw); break;
      case MG_SAMPLE: mg_dense<RT, MG_SAMPLE, NW, MASK>(L, S, base, Rw); break;
      case MG_PRIOR: mg_dense<RT, MG_PRIOR, NW, MASK>(L, S, base, Rw); break;
      default: mg_dense<RT, MG_BERN, NW, MASK>(L, S, base, Rw); break;
    }
    MG_TRACE(3 + 3 * s)
    mg_lds_barrier();
    MG_TRACE(4 + 3 * s)
  }

  // ---- per-row sums: over the 4 lane groups, then over waves
  {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float v = Rw.lw[rt] + kLn2 * Rw.l2[rt];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (g == 0) red[wave * R + rt * 16 + r] = v;
    }
  }
  __syncthreads();
  if (t < nrows) {
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) acc += red[w * R + t];
    // F:345-F:349: log w = (log p(h) + log p(x|h)) - log q(h|x)
    L.lw[row0 + t] = (logp[t] + acc) - logq[t];
  }
  MG_TRACE(127)
}

template <bool MASK>
static hipError_t launch_mega_fwd_t(hipStream_t st, const MgLaunch& L, int rt, int waves, size_t lds_bytes) {
  if (L.rows <= 0) return hipSuccess;
  const int R = 16 * rt;
  const dim3 grid((L.rows + R - 1) / R), block(waves * 64);
  if (waves == 4) {
    if (rt != 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL((mega_fwd_kernel<2, 4, MASK>), grid, block, lds_bytes, st, L);
    return hipGetLastError();
  }
  if (waves != MG_WAVES) return hipErrorInvalidValue;
  switch (rt) {
    case 1: hipLaunchKernelGGL((mega_fwd_kernel<1, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    case 2: hipLaunchKernelGGL((mega_fwd_kernel<2, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    case 4: hipLaunchKernelGGL((mega_fwd_kernel<4, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_mega_fwd(hipStream_t st, const MgLaunch& L, int rt, int waves, size_t lds_bytes) {
  return launch_mega_fwd_t<false>(st, L, rt, waves, lds_bytes);
}
hipError_t launch_mega_fwd_masked(hipStream_t st, const MgLaunch& L, int rt, int waves, size_t lds_bytes) {
  return launch_mega_fwd_t<true>(st, L, rt, waves, lds_bytes);
}

hipError_t mega_setup_attributes() {
  const void* fns[] = {(const void*)mega_fwd_kernel<1, MG_WAVES, false>, (const void*)mega_fwd_kernel<2, MG_WAVES, false>,
                       (const void*)mega_fwd_kernel<4, MG_WAVES, false>, (const void*)mega_fwd_kernel<2, 4, false>,
                       (const void*)mega_fwd_kernel<1, MG_WAVES, true>, (const void*)mega_fwd_kernel<2, MG_WAVES, true>,
                       (const void*)mega_fwd_kernel<4, MG_WAVES, true>, (const void*)mega_fwd_kernel<2, 4, true>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace iwae

#ifdef IWAE_MG_TRACE
extern "C" int iwae_mg_trace_dump(unsigned long long* out, int cap) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  const int n = 4 * 8 * 128 < cap ? 4 * 8 * 128 : cap;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(iwae::g_mg_trace), n * sizeof(unsigned long long)) != hipSuccess) return -1;
  return n;
}
#endif
