// Device code of iwae_score / iwae_encode (gfx950): score_kernel, the fused
// scoring kernel on mega_fwd_kernel's stages (iwae_mega_dev.h; ScLaunch in
// iwae_kernels.h describes it), and the small launches of the layer-wise path:
// the relayouts between the callers' sample-major [k][N][d] latent buffers (the
// reference's layout of h_i, F:59 / F:68) and the workspace's image-major rows,
// and the row sums of the Bernoulli partials.
#include "iwae_mega_dev.h"
#include "iwae_bound.h"

namespace iwae {

// Operands requested ahead of the tile's MFMAs: the density heads' f32 targets
// h_t[j0], h_t[j0 + 1] of the lane's rows, from the caller's [k][N][d] buffer
// (columns past d: 0, masked in the epilogue); the output stage's pixels when
// log p(x|h) is asked for.
template <int RT, int ACT>
__device__ __forceinline__ void sc_operands(const ScLaunch& L, const MgStage& S, int t, const ScRows<RT>& R,
                                            float4 (&xv)[RT], ScTargets<RT, true>& T) {
  float2 (&tg)[RT] = T.v;
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  if (ACT == MG_BERNS) {
    if (!L.log_px) return;
    const __amdgpu_buffer_rsrc_t rx = buf_rsrc(L.x);
    const int f0 = t * 16 + 4 * g;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) xv[rt] = bld4(rx, f0 < S.N ? R.xoff[rt] + (unsigned)f0 * 4u : kOOB);
  } else {
    const int j0 = 4 * (2 * t + (g >> 1)) + 2 * (g & 1);
    const int d = S.d;
    const int row0 = blockIdx.x * 16 * RT;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int grow = row0 + min(rt * 16 + r, L.rows - 1 - row0);      // global row (clamped into the chunk)
      const float* tp = L.eps[S.layer] + ((size_t)(grow % L.kS) * L.eps_N + (L.eps_i0 + grow / L.kS)) * d;
      tg[rt].x = j0 < d ? tp[j0] : 0.f;
      tg[rt].y = j0 + 1 < d ? tp[j0 + 1] : 0.f;
    }
  }
}

// Epilogues.  Density heads: mg_head's lane exchange, then log N(target; mu,
// s) of the lane's two columns into the row's log q (MG_DENSQ) or log p(h)
// (MG_DENSP).  Output stage: mg_bern into log p(x|h), and / or p = sigmoid(l)
// (1 - 1e-6) + 1e-7 of the lane's four features stored (rows of the chunk only;
// 16-byte stores: ld_probs is a multiple of 4 and probs 16-byte aligned).
// MASK: the pixel-masked likelihood (mg_bern<., true>: xv holds -1 at a missing
// pixel); the probabilities stored are every pixel's, observed or not.
template <int RT, int ACT, bool MASK>
__device__ __forceinline__ void sc_epilogue(const ScLaunch& L, const MgStage& S, int t, const mg_f32x4 (&acc)[RT],
                                            const float4 (&xv)[RT], const ScTargets<RT, true>& T, ScRows<RT>& R) {
  const float2 (&tg)[RT] = T.v;
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  if (ACT == MG_BERNS) {
    if (L.log_px) mg_bern<RT, MASK>(L, S, t, acc, xv, R);
    if (L.probs) {
      const int f0 = t * 16 + 4 * g;
      const int row0 = blockIdx.x * 16 * RT;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int row = row0 + rt * 16 + r;
        if (row >= L.rows || f0 >= S.N) continue;
        float p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = __builtin_fmaf(frcp(1.f + fexp(-acc[rt][i])), kProbScale, kProbShift);
        float* o = L.probs + (size_t)row * L.ld_probs + f0;
        if (f0 + 3 < S.N) {
          *reinterpret_cast<float4*>(o) = make_float4(p[0], p[1], p[2], p[3]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (f0 + i < S.N) o[i] = p[i];
        }
      }
    }
  } else {
    const int j0 = 4 * (2 * t + (g >> 1)) + 2 * (g & 1);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const auto p0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][0]), __float_as_uint(acc[rt][2]),
                                                       false, false);
      const auto p1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][1]), __float_as_uint(acc[rt][3]),
                                                       false, false);
      const float mu[2] = {__uint_as_float(p0[0]), __uint_as_float(p1[0])};
      const float zs[2] = {__uint_as_float(p0[1]), __uint_as_float(p1[1])};
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float sc = fexp(zs[c]) + kScaleEps;
        const float v = mg_normal_logp(c == 0 ? tg[rt].x : tg[rt].y, mu[c], sc);
        if (ACT == MG_DENSQ) R.lq[rt] += j0 + c < S.d ? v : 0.f;
        else R.lw[rt] += j0 + c < S.d ? v : 0.f;
      }
      __builtin_amdgcn_sched_barrier(0);     // one row tile at a time (register pressure)
    }
  }
}

// iwae_score's fused path (ScLaunch, iwae_kernels.h): the latents are the
// caller's, so the prologue fills the LDS tiles the stage list reads and the
// stages only evaluate densities.  Same row tiles, waves and LDS plan as
// mega_fwd_kernel; nothing is drawn.  MASK: the pixel-masked likelihood of
// iwae_score_masked; L.x is then the staged copy with -1 at the missing pixels.
template <int RT, int NW, bool MASK>
__global__ __launch_bounds__(NW * 64) void score_kernel(ScLaunch L) {
  constexpr int R = 16 * RT;
  constexpr int TPR = (NW * 64) / R;            // threads per row in the prologue
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, L.rows - row0);
  float* logq = mgs + L.acc_off;
  float* logp = logq + R;
  const int rr = t / TPR, sub = t - rr * TPR;   // prologue: row rr, lane group sub
  // ---- prologue: the rows' h_i tiles (row-contiguous reads of the caller's
  // sample-major buffers); log N(h_1; mu0, s0) of the row's image; log N(h_L; 0, 1)
  {
    const int rg = row0 + min(rr, nrows - 1);
    const size_t srow = (size_t)(rg % L.kS) * L.eps_N + (L.eps_i0 + rg / L.kS);
    float aq = 0.f, ap = 0.f;
    for (int i = 0; i < L.n_lat; ++i) {
      const int d = L.lat_d[i];
      const float* hp = L.eps[i] + srow * d;
      const bool q0 = i == 0 && L.want_q, pL = i == L.n_lat - 1 && L.want_ph;
      if (L.lat_buf[i] >= 0) {
        const MgBuf H = mg_buf<RT>(L, L.lat_buf[i]);
        for (int j = sub; j < L.lat_next_k[i]; j += TPR) {
          const float hv = j < d ? hp[j] : (j == d ? 1.f : 0.f);
          const __bf16 vh = (__bf16)hv;
          H.hi[rr * H.ld + j] = vh;
          H.lo[rr * H.ld + j] = (__bf16)(hv - (float)vh);
        }
      }
      if (q0) {
        const float* Pp = L.P0 + (size_t)(rg / L.kS) * L.ldP0;
        for (int j = sub; j < d; j += TPR) aq += mg_normal_logp(hp[j], Pp[j], fexp(Pp[d + j]) + kScaleEps);
      }
      if (pL)
        for (int j = sub; j < d; j += TPR) {
          const float hv = hp[j];
          ap += -0.5f * (hv * hv) - kHalfLog2Pi;
        }
    }
    for (int o = TPR >> 1; o > 0; o >>= 1) {
      aq += __shfl_xor(aq, o);
      ap += __shfl_xor(ap, o);
    }
    if (sub == 0) {
      logq[rr] = aq;
      logp[rr] = ap;
    }
  }
  ScRows<RT> Rw;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = min(rt * 16 + (lane & 15), nrows - 1);
    Rw.lw[rt] = 0.f;
    Rw.l2[rt] = 0.f;
    Rw.lq[rt] = 0.f;
    Rw.xoff[rt] = (unsigned)((row0 + row) / L.kS) * (unsigned)L.ldx * 4u;
  }
  mg_lds_barrier();

  for (int s = 0; s < L.nst; ++s) {
    const MgStage& S = L.st[s];
    if (S.act == MG_TANH) mg_pad<RT, NW>(mg_buf<RT>(L, S.out_buf), S.N, S.next_k);
    switch (S.act) {
      case MG_TANH: mg_dense<RT, MG_TANH, NW, MASK>(L, S, 0ull, Rw); break;
      case MG_DENSQ: mg_dense<RT, MG_DENSQ, NW, MASK>(L, S, 0ull, Rw); break;
      case MG_DENSP: mg_dense<RT, MG_DENSP, NW, MASK>(L, S, 0ull, Rw); break;
      default: mg_dense<RT, MG_BERNS, NW, MASK>(L, S, 0ull, Rw); break;
    }
    mg_lds_barrier();
  }

  // ---- per-row sums of the three terms: over the 4 lane groups, then over
  // waves (the activation buffers are dead: their LDS is the scratch, [3][NW][R])
  float* red = mgs;
  {
    const int r = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float v[3] = {Rw.lq[rt], Rw.lw[rt], kLn2 * Rw.l2[rt]};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        v[q] += __shfl_xor(v[q], 16);
        v[q] += __shfl_xor(v[q], 32);
        if (g == 0) red[(q * NW + wave) * R + rt * 16 + r] = v[q];
      }
    }
  }
  __syncthreads();
  if (t < nrows) {
    float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int w = 0; w < NW; ++w) a[q] += red[(q * NW + w) * R + t];
    if (L.log_q) L.log_q[row0 + t] = logq[t] + a[0];
    if (L.log_ph) L.log_ph[row0 + t] = logp[t] + a[1];
    if (L.log_px) L.log_px[row0 + t] = a[2];
  }
}

template <bool MASK>
static hipError_t launch_score_t(hipStream_t st, const ScLaunch& L, int rt, int waves, size_t lds_bytes) {
  if (L.rows <= 0) return hipSuccess;
  const int R = 16 * rt;
  const dim3 grid((L.rows + R - 1) / R), block(waves * 64);
  if (waves == 4) {
    if (rt != 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL((score_kernel<2, 4, MASK>), grid, block, lds_bytes, st, L);
    return hipGetLastError();
  }
  if (waves != MG_WAVES) return hipErrorInvalidValue;
  switch (rt) {
    case 1: hipLaunchKernelGGL((score_kernel<1, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    case 2: hipLaunchKernelGGL((score_kernel<2, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    case 4: hipLaunchKernelGGL((score_kernel<4, MG_WAVES, MASK>), grid, block, lds_bytes, st, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_score(hipStream_t st, const ScLaunch& L, int rt, int waves, size_t lds_bytes) {
  return launch_score_t<false>(st, L, rt, waves, lds_bytes);
}
hipError_t launch_score_masked(hipStream_t st, const ScLaunch& L, int rt, int waves, size_t lds_bytes) {
  return launch_score_t<true>(st, L, rt, waves, lds_bytes);
}

hipError_t score_setup_attributes() {
  const void* fns[] = {(const void*)score_kernel<1, MG_WAVES, false>, (const void*)score_kernel<2, MG_WAVES, false>,
                       (const void*)score_kernel<4, MG_WAVES, false>, (const void*)score_kernel<2, 4, false>,
                       (const void*)score_kernel<1, MG_WAVES, true>, (const void*)score_kernel<2, MG_WAVES, true>,
                       (const void*)score_kernel<4, MG_WAVES, true>, (const void*)score_kernel<2, 4, true>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// One thread per element, indexed sample-major (s, b, j) so the accesses of the
// caller's buffer are contiguous; blockIdx.y is the segment.
__global__ __launch_bounds__(256) void score_relayout_kernel(ScRelayout a) {
  const ScSeg& g = a.seg[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)a.n * g.d;
  if (g.img) {
    if (i >= per) return;
    const int b = (int)(i / g.d), j = (int)(i - (long long)b * g.d);
    const float v = g.rows[(size_t)b * g.ld + g.col0 + j];
    g.ext[(size_t)(a.i0 + b) * g.d + j] = g.expo ? fexp(v) + kScaleEps : v;
    return;
  }
  if (i >= per * a.k) return;
  const int s = (int)(i / per);
  const long long rem = i - (long long)s * per;
  const int b = (int)(rem / g.d), j = (int)(rem - (long long)b * g.d);
  float* row = g.rows + ((size_t)b * a.k + s) * g.ld + g.col0 + j;
  float* ext = g.ext + ((size_t)s * a.N + a.i0 + b) * g.d + j;
  if (a.gather) {
    *row = *ext;
  } else {
    const float v = *row;
    *ext = g.expo ? fexp(v) + kScaleEps : v;
  }
}

hipError_t launch_score_relayout(hipStream_t st, const ScRelayout& a) {
  if (a.nseg <= 0 || a.n <= 0 || a.k <= 0) return hipSuccess;
  long long most = 0;
  for (int g = 0; g < a.nseg; ++g) {
    const long long e = (long long)a.n * a.seg[g].d * (a.seg[g].img ? 1 : a.k);
    most = e > most ? e : most;
  }
  if (most <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_relayout_kernel, dim3((unsigned)((most + 255) / 256), a.nseg), dim3(256), 0, st, a);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void score_rowsum_kernel(const float* part, int ldpart, int npart, int rows,
                                                           float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) out[r] = row_sum_parts(part, ldpart, npart, r);
}

hipError_t launch_score_rowsum(hipStream_t st, const float* part, int ldpart, int npart, int rows, float* out) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_rowsum_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, part, ldpart, npart, rows, out);
  return hipGetLastError();
}

}  // namespace iwae
