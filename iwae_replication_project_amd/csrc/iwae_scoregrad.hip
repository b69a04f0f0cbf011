// Device code of iwae_score_grad (gfx950).  Layer-wise path: the Gaussian
// heads' gradient kernel and the scatter that sums the terms into the caller's
// sample-major buffers (SgDens, SgScatter in iwae_kernels.h); its matrix
// products are the tiled GEMM's (iwae_gemm.hip), its values iwae_score's own
// launches.  Fused path: sg_kernel (SgLaunch), on the device functions of
// iwae_mega_dev.h.
#include <algorithm>

#include "iwae_mega_dev.h"

namespace iwae {

// One wave per row r, lanes over the head's columns.  With z = (t - mu) / s,
// s = exp(zs) + 1e-6: tg = -z / s; dP = (z / s | (z^2 - 1) (s - 1e-6) / s).
// The head's row is r / prow_div (the first encoder layer: one row per image).
__global__ __launch_bounds__(256) void sg_dens_kernel(SgDens a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.M) return;
  const float* __restrict__ P = a.P + (size_t)(r / a.prow_div) * a.ldP;
  const float* __restrict__ H = a.H + (size_t)r * a.ldH;
  float* __restrict__ tg = a.tg + (size_t)r * a.ldtg;
  float* __restrict__ dP = a.dP ? a.dP + (size_t)r * a.lddP : nullptr;
  for (int j = lane; j < a.d; j += 64) {
    const float mu = P[j];
    const float e = fexp(P[a.d + j]);
    const float rs = frcp(e + kScaleEps);
    const float z = H[j] * rs - mu * rs;
    tg[j] = -z * rs;
    if (dP) {
      dP[j] = z * rs;
      dP[a.d + j] = ((z * z - 1.f) * rs) * e;
    }
  }
}

hipError_t launch_sg_dens(hipStream_t st, const SgDens& a) {
  if (a.M <= 0 || a.d <= 0) return hipSuccess;
  hipLaunchKernelGGL(sg_dens_kernel, dim3((a.M + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

// One thread per element of a layer's gradient, indexed sample-major (s, b, j)
// as score_relayout_kernel (contiguous stores); blockIdx.y is the layer.  The
// sum runs over the layer's sources in their listed order, each times its
// coefficient, then the top layer's -c h_L: one fixed order, no atomics.
__global__ __launch_bounds__(256) void sg_scatter_kernel(SgScatter a) {
  const SgLayer& g = a.lay[blockIdx.y];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = (long long)a.n * g.d;
  if (i >= per * a.k) return;
  const int s = (int)(i / per);
  const long long rem = i - (long long)s * per;
  const int b = (int)(rem / g.d), j = (int)(rem - (long long)b * g.d);
  const size_t row = (size_t)b * a.k + s;
  const size_t e = ((size_t)s * a.N + a.i0 + b) * g.d + j;
  float acc = 0.f;
#pragma unroll
  for (int q = 0; q < kSgMaxSrc; ++q)
    if (q < g.nsrc) acc += g.c[q] * g.src[q][row * g.ld[q] + j];
  if (g.c_top != 0.f) acc += g.c_top * -g.lat[e];
  g.out[e] = acc;
}

hipError_t launch_sg_scatter(hipStream_t st, const SgScatter& a) {
  if (a.nlay <= 0 || a.n <= 0 || a.k <= 0) return hipSuccess;
  long long most = 0;
  for (int g = 0; g < a.nlay; ++g) most = std::max(most, (long long)a.n * a.k * a.lay[g].d);
  if (most <= 0) return hipSuccess;
  hipLaunchKernelGGL(sg_scatter_kernel, dim3((unsigned)((most + 255) / 256), a.nlay), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------- fused path
// A fragments of column tile t (of ntile) over k in [k0, k0 + 256) of a copy with ldk padded K
__device__ __forceinline__ void sg_fetch(__amdgpu_buffer_rsrc_t rh, __amdgpu_buffer_rsrc_t rl, int ntile, int ldk,
                                         int t, int k0, MgFrag& f) {
  const int lane = threadIdx.x & 63;
  const unsigned vb = t < ntile ? (unsigned)(((t * (ldk >> 5) + (k0 >> 5)) * 64 + lane) * 16) : kOOB;
  const int ns = (ldk - k0) >> 5;
#pragma unroll
  for (int u = 0; u < MG_KS; ++u) mg_fetch_step(rh, rl, vb, u, ns, f);
}

// acc = tile t of (copy at woff: N features, ldk padded K) . IN, the whole K
template <int RT>
__device__ __forceinline__ void sg_tile(const SgLaunch& L, unsigned woff, int N, int ldk, const MgBuf& IN, int t,
                                        mg_f32x4 (&acc)[RT]) {
  const unsigned bytes = (unsigned)((L.fx_elems - (long long)woff) * (long long)sizeof(__bf16));
  const __amdgpu_buffer_rsrc_t rh = buf_rsrc(L.fx_hi + woff, bytes), rl = buf_rsrc(L.fx_lo + woff, bytes);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < ldk; k0 += 32 * MG_KS) {
    MgFrag f;
    sg_fetch(rh, rl, (N + 15) >> 4, ldk, t, k0, f);
    mg_mma<RT>(IN, k0, min(MG_KS, (ldk - k0) >> 5), f, acc, rh, rl, false, kOOB, 0);
  }
}

// v -> hi / lo planes of B at (row, f0 .. f0 + 3), columns below N only
__device__ __forceinline__ void sg_store4(const MgBuf& B, int row, int f0, int N, const float (&v)[4]) {
  mg_bf16x4 vh, vl;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    vh[i] = (__bf16)v[i];
    vl[i] = (__bf16)(v[i] - (float)vh[i]);
  }
  const int o = row * B.ld + f0;
  if (f0 + 3 < N) {
    *reinterpret_cast<mg_bf16x4*>(B.hi + o) = vh;
    *reinterpret_cast<mg_bf16x4*>(B.lo + o) = vl;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (f0 + i < N) {
        B.hi[o + i] = vh[i];
        B.lo[o + i] = vl[i];
      }
  }
}

// acc (1 - y^2) in place of y in Y: the lane's four features of its rows
template <int RT>
__device__ __forceinline__ void sg_gtanh(const MgBuf& Y, int t, int N, const mg_f32x4 (&acc)[RT]) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int f0 = t * 16 + 4 * g;
  if (f0 >= N) return;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = rt * 16 + r;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = row * Y.ld + min(f0 + i, N - 1);
      const float y = (float)Y.hi[o] + (float)Y.lo[o];
      v[i] = acc[rt][i] * (1.f - y * y);
    }
    sg_store4(Y, row, f0, N, v);
  }
}

// One workgroup: 16 RT rows of the chunk, 8 waves; wave w owns column tiles w, w + 8, ...
// MASK (iwae_score_grad_masked): L.x is the staged copy with -1 at the missing pixels; such a
// pixel's term of log p(x|h) and its dlogit are selected to 0 (both are computed for every
// pixel: a -1 keeps each expression finite).
template <int RT, bool MASK>
__global__ __launch_bounds__(MG_WAVES * 64) void sg_kernel(SgLaunch L) {
  constexpr int NW = MG_WAVES;
  static_assert(kSgWaves == MG_WAVES, "sgrad_plan sizes the workgroup by kSgWaves");
  constexpr int R = 16 * RT;
  constexpr int TPR = (NW * 64) / R;            // threads per row in the prologue and the final store
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * R;
  const int nrows = min(R, L.rows - row0);
  float* logq = mgs + L.acc_off;
  float* logp = logq + R;
  const int rr = tid / TPR, sub = tid - rr * TPR;
  const int rg = row0 + min(rr, nrows - 1);
  const size_t srow = (size_t)(rg % L.kS) * L.lat_N + (L.lat_i0 + rg / L.kS);
  // ---- prologue: the rows' h_i tiles, the gradient tiles' first addends (c_q T^q_1, -c_ph h_L),
  // log N(h_1; mu0, s0) and log N(h_L; 0, 1)
  {
    float aq = 0.f, ap = 0.f;
    for (int i = 0; i < L.n_lat; ++i) {
      const int d = L.lat_d[i];
      const float* hp = L.lat[i] + srow * d;
      float* G = mgs + L.g_off[i] + rr * L.g_ld[i];
      const bool q0 = i == 0, pL = i == L.n_lat - 1;
      for (int j = sub; j < max(d, L.lat_buf[i] >= 0 ? L.lat_next_k[i] : 0); j += TPR) {
        const float hv = j < d ? hp[j] : (j == d ? 1.f : 0.f);
        if (L.lat_buf[i] >= 0 && j < L.lat_next_k[i]) {
          __bf16* base = reinterpret_cast<__bf16*>(mgs) + L.buf_off[L.lat_buf[i]];
          const int ld = L.buf_ld[L.lat_buf[i]];
          const __bf16 vh = (__bf16)hv;
          base[rr * ld + j] = vh;
          base[R * ld + rr * ld + j] = (__bf16)(hv - (float)vh);
        }
        if (j >= d) continue;
        float gv = 0.f;
        if (q0 && (L.want_q || L.cq != 0.f)) {
          const float* Pp = L.P0 + (size_t)(rg / L.kS) * L.ldP0;
          const float sc = fexp(Pp[d + j]) + kScaleEps;
          if (L.want_q) aq += mg_normal_logp(hv, Pp[j], sc);
          if (L.cq != 0.f) {
            const float rs = frcp(sc);
            gv += L.cq * (-(hv * rs - Pp[j] * rs) * rs);
          }
        }
        if (pL) {
          if (L.want_ph) ap += -0.5f * (hv * hv) - kHalfLog2Pi;
          if (L.cph != 0.f) gv += L.cph * -hv;
        }
        G[j] = gv;
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
  float lq[RT], lp[RT], l2[RT];
  unsigned xoff[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    lq[rt] = lp[rt] = l2[rt] = 0.f;
    const int row = min(rt * 16 + r, nrows - 1);
    xoff[rt] = (unsigned)((row0 + row) / L.kS) * (unsigned)L.ldx * 4u;
  }
  mg_lds_barrier();

  auto buf = [&](int b) {
    MgBuf B;
    B.ld = L.buf_ld[b];
    B.hi = reinterpret_cast<__bf16*>(mgs) + L.buf_off[b];
    B.lo = B.hi + R * B.ld;
    return B;
  };

  for (int s = 0; s < L.nst; ++s) {
    const SgStage& S = L.st[s];
    const int ntile = (S.N + 15) >> 4;
    const MgBuf IN = buf(S.in_buf);
    if (S.kind == SG_TANH) {
      const MgBuf OUT = buf(S.out_buf);
      mg_pad<RT, NW>(OUT, S.N, S.next_k);
      for (int t = wave; t < ntile; t += NW) {
        mg_f32x4 acc[RT];
        sg_tile<RT>(L, S.woff, S.N, S.ldk, IN, t, acc);
        const int f0 = t * 16 + 4 * g;
        if (f0 < S.N) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = mg_tanh(acc[rt][i]);
            sg_store4(OUT, rt * 16 + r, f0, S.N, v);
          }
        }
      }
    } else if (S.kind == SG_HEADQ || S.kind == SG_HEADP) {
      const int d = S.d;
      const bool grad = S.c != 0.f;
      const MgBuf DP = buf(S.out_buf);
      if (grad) {                                // dP's padding: columns [2 d, next_k)
        for (int col = 2 * d + sub; col < S.next_k; col += TPR) {
          DP.hi[rr * DP.ld + col] = (__bf16)0.f;
          DP.lo[rr * DP.ld + col] = (__bf16)0.f;
        }
      }
      float* G = mgs + L.g_off[S.layer];
      const int gld = L.g_ld[S.layer];
      for (int t = wave; t < ntile; t += NW) {
        const int j0 = 4 * (2 * t + (g >> 1)) + 2 * (g & 1);
        float2 tg[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const int grow = row0 + min(rt * 16 + r, L.rows - 1 - row0);
          const float* tp = L.lat[S.layer] + ((size_t)(grow % L.kS) * L.lat_N + (L.lat_i0 + grow / L.kS)) * d;
          tg[rt].x = j0 < d ? tp[j0] : 0.f;
          tg[rt].y = j0 + 1 < d ? tp[j0 + 1] : 0.f;
        }
        mg_f32x4 acc[RT];
        sg_tile<RT>(L, S.woff, S.N, S.ldk, IN, t, acc);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const auto p0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][0]), __float_as_uint(acc[rt][2]),
                                                           false, false);
          const auto p1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][1]), __float_as_uint(acc[rt][3]),
                                                           false, false);
          const float mu[2] = {__uint_as_float(p0[0]), __uint_as_float(p1[0])};
          const float zs[2] = {__uint_as_float(p0[1]), __uint_as_float(p1[1])};
          const int row = rt * 16 + r;
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int j = j0 + c;
            const float e = fexp(zs[c]);
            const float sc = e + kScaleEps;
            const float tv = c == 0 ? tg[rt].x : tg[rt].y;
            const float v = mg_normal_logp(tv, mu[c], sc);
            if (S.kind == SG_HEADQ) lq[rt] += j < d ? v : 0.f;
            else lp[rt] += j < d ? v : 0.f;
            if (grad && j < d) {
              const float rs = frcp(sc);
              const float z = tv * rs - mu[c] * rs;
              G[row * gld + j] += S.c * (-z * rs);
              const float dmu = S.c * (z * rs), dzs = S.c * (((z * z - 1.f) * rs) * e);
              const __bf16 mh = (__bf16)dmu, sh = (__bf16)dzs;
              DP.hi[row * DP.ld + j] = mh;
              DP.lo[row * DP.ld + j] = (__bf16)(dmu - (float)mh);
              DP.hi[row * DP.ld + d + j] = sh;
              DP.lo[row * DP.ld + d + j] = (__bf16)(dzs - (float)sh);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else if (S.kind == SG_GTANH) {
      const MgBuf Y = buf(S.out_buf);
      for (int t = wave; t < ntile; t += NW) {
        mg_f32x4 acc[RT];
        sg_tile<RT>(L, S.woff, S.N, S.ldk, IN, t, acc);
        sg_gtanh<RT>(Y, t, S.N, acc);
      }
    } else if (S.kind == SG_GX) {
      float* G = mgs + L.g_off[S.layer];
      const int gld = L.g_ld[S.layer];
      for (int t = wave; t < ntile; t += NW) {
        mg_f32x4 acc[RT];
        sg_tile<RT>(L, S.woff, S.N, S.ldk, IN, t, acc);
        const int f0 = t * 16 + 4 * g;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (f0 + i < S.N) G[(rt * 16 + r) * gld + f0 + i] += acc[rt][i];
      }
    } else {                                     // SG_OUT
      const bool grad = S.c != 0.f;
      const MgBuf D = buf(S.out_buf);
      const int nt2 = (L.out_gx_N + 15) >> 4;
      const unsigned gbytes = (unsigned)((L.fx_elems - (long long)L.out_gx_woff) * (long long)sizeof(__bf16));
      const __amdgpu_buffer_rsrc_t gh = buf_rsrc(L.fx_hi + L.out_gx_woff, gbytes);
      const __amdgpu_buffer_rsrc_t gl = buf_rsrc(L.fx_lo + L.out_gx_woff, gbytes);
      const __amdgpu_buffer_rsrc_t rx = buf_rsrc(L.x);
      mg_f32x4 acc2[kSgOutTiles][RT];
#pragma unroll
      for (int q = 0; q < kSgOutTiles; ++q)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc2[q][rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
      const int nchunk = (ntile + 15) >> 4;      // slabs of 256 pixels
      for (int c = 0; c < nchunk; ++c) {
        for (int t = 16 * c + wave; t < 16 * c + 16; t += NW) {
          const int f0 = t * 16 + 4 * g;
          float4 xv[RT];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) xv[rt] = bld4(rx, (t < ntile && f0 < S.N) ? xoff[rt] + (unsigned)f0 * 4u : kOOB);
          mg_f32x4 acc[RT];
          if (t < ntile) {
            sg_tile<RT>(L, S.woff, S.N, S.ldk, IN, t, acc);
          } else {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = (mg_f32x4){0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            float dl[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float x = f4_at(xv[rt], i);
              const float l = acc[rt][i];
              const float a = fexp(-__builtin_fabsf(l));
              const float rc = frcp(1.f + a), ar = a * rc;
              const float p1 = __builtin_fmaf(l >= 0.f ? rc : ar, kProbScale, kProbShift);
              const float p0 = __builtin_fmaf(l >= 0.f ? ar : rc, kProbScale, kBernOff0);
              const bool ok = t < ntile && f0 + i < S.N && !(MASK && x < 0.f);
              const float v = x * __builtin_amdgcn_logf(p1) + (1.f - x) * __builtin_amdgcn_logf(p0);
              l2[rt] += ok ? v : 0.f;
              const float gl1 = x * frcp(p1) - (1.f - x) * frcp(p0);
              dl[i] = ok ? S.c * gl1 * (kProbScale * (ar * rc)) : 0.f;
            }
            if (grad) sg_store4(D, rt * 16 + r, f0 - 256 * c, 256, dl);
          }
        }
        if (!grad) continue;
        mg_lds_barrier();
        const int ns = min(MG_KS, (L.out_gx_ldk - 256 * c) >> 5);
#pragma unroll
        for (int q = 0; q < kSgOutTiles; ++q) {
          const int t2 = wave + q * NW;
          if (t2 < nt2 && ns > 0) {
            MgFrag f;
            sg_fetch(gh, gl, nt2, L.out_gx_ldk, t2, 256 * c, f);
            mg_mma<RT>(D, 0, ns, f, acc2[q], gh, gl, false, kOOB, 0);
          }
        }
        mg_lds_barrier();
      }
      if (grad) {
#pragma unroll
        for (int q = 0; q < kSgOutTiles; ++q) {
          const int t2 = wave + q * NW;
          if (t2 < nt2) sg_gtanh<RT>(IN, t2, L.out_gx_N, acc2[q]);
        }
      }
    }
    mg_lds_barrier();
  }

  // ---- the gradient tiles into the caller's sample-major buffers (the prologue's addressing)
  if (rr < nrows) {
    for (int i = 0; i < L.n_lat; ++i) {
      if (!L.grad[i]) continue;
      const int d = L.lat_d[i];
      const float* G = mgs + L.g_off[i] + rr * L.g_ld[i];
      float* gp = L.grad[i] + srow * d;
      for (int j = sub; j < d; j += TPR) gp[j] = G[j];
    }
  }
  __syncthreads();
  // ---- per-row sums of the three values: over the 4 lane groups, then over waves
  float* red = mgs;
  {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      float v[3] = {lq[rt], lp[rt], kLn2 * l2[rt]};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        v[q] += __shfl_xor(v[q], 16);
        v[q] += __shfl_xor(v[q], 32);
        if (g == 0) red[(q * NW + wave) * R + rt * 16 + r] = v[q];
      }
    }
  }
  __syncthreads();
  if (tid < nrows) {
    float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int w = 0; w < NW; ++w) a[q] += red[(q * NW + w) * R + tid];
    if (L.log_q) L.log_q[row0 + tid] = logq[tid] + a[0];
    if (L.log_ph) L.log_ph[row0 + tid] = logp[tid] + a[1];
    if (L.log_px) L.log_px[row0 + tid] = a[2];
  }
}

template <bool MASK>
static hipError_t launch_sgrad_t(hipStream_t st, const SgLaunch& L, int rt, size_t lds_bytes) {
  if (L.rows <= 0) return hipSuccess;
  const int R = 16 * rt;
  const dim3 grid((L.rows + R - 1) / R), block(MG_WAVES * 64);
  switch (rt) {
    case 1: hipLaunchKernelGGL((sg_kernel<1, MASK>), grid, block, lds_bytes, st, L); break;
    case 2: hipLaunchKernelGGL((sg_kernel<2, MASK>), grid, block, lds_bytes, st, L); break;
    case 4: hipLaunchKernelGGL((sg_kernel<4, MASK>), grid, block, lds_bytes, st, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_sgrad(hipStream_t st, const SgLaunch& L, int rt, size_t lds_bytes) {
  return launch_sgrad_t<false>(st, L, rt, lds_bytes);
}
hipError_t launch_sgrad_masked(hipStream_t st, const SgLaunch& L, int rt, size_t lds_bytes) {
  return launch_sgrad_t<true>(st, L, rt, lds_bytes);
}

hipError_t sgrad_setup_attributes() {
  const void* fns[] = {(const void*)sg_kernel<1, false>, (const void*)sg_kernel<2, false>, (const void*)sg_kernel<4, false>,
                       (const void*)sg_kernel<1, true>, (const void*)sg_kernel<2, true>, (const void*)sg_kernel<4, true>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace iwae
