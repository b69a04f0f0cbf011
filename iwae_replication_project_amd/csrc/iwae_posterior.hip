// Importance-weighted posterior q_IW (Cremer, Morningstar & Duvenaud 2017):
// the self-normalised weights w~_s = softmax_s(log w) of an image's k samples
// and what is formed under them -- posterior-mean latents sum_s w~_s h_{i,s},
// the reconstruction sum_s w~_s p(x | h_{1,s}) and one sampling-importance-
// resampling draw per image (iwae_posterior), gfx950.
//
// A chunk of images runs in two passes.  Pass 1 is the NLL's: the log weight of
// every row and lse_kernel's (m, sum e) per image.  Then, here:
//
//   post_weights_kernel   w~ per row, ess and the SIR index per image
//   post_kernel           pass 2, fused: the rows recomputed from the same noise,
//                         every sum formed in the epilogues (weights known)
//   post_merge_kernel     an image's per-workgroup partial sums added in tile order
//   group_wsum_kernel     pass 2 of the layer-wise path: weighted sums over rows in HBM
//
// post_kernel runs on the chain machinery shared with mega_fwd_kernel,
// score_kernel and gen_kernel (iwae_mega_dev.h): bf16x3 products on the bf16
// 16x16x32 MFMA, the weights as the A operand streamed from the fragment-major
// FX copies, the activations as the B operand read from LDS where they are
// kept as two bf16 planes (hi, lo) with row strides of 8 mod 16 dwords, the
// ones column of the next reader written by mg_pad, LDS-only barriers between
// stages, the loop over a wave's column tiles (mg_tiles).  Its own, here: the
// prologue, the weighted sampling and output epilogues and the kernel body.
// Head rows are permuted into [mu 4q..4q+3 | zs 4q..4q+3] groups and exchanged
// with v_permlane16_swap.  It has no prior stages and no density sums: they
// only feed log w.  The rows of one workgroup belong to one image, so the
// weighted sum over rows is a reduction over the 16 lanes that hold one
// feature (and the RT row tiles of a lane) -- no segmented reduction.
// Deterministic: no float atomics, fixed reduction order, each output written
// by one lane.
#include "iwae_bound.h"
#include "iwae_mega_dev.h"

namespace iwae {

// ------------------------------------------------------------------ weights
constexpr int kPwThreads = 256, kPwBatch = 8;

// log w of a row, as lse_kernel assembles it
__device__ __forceinline__ float pw_row(const LseArgs& a, int r) {
  return a.lw ? a.lw[r] : __fsub_rn(__fadd_rn(a.logp[r], row_sum_parts(a.part, a.ldpart, a.npart, r)), a.logq[r]);
}

__global__ __launch_bounds__(kPwThreads) void post_weights_kernel(PostWArgs a) {
  __shared__ float sq[kPwThreads / 64];
  __shared__ float sc[kPwThreads * kPwBatch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x, kS = a.src.kS;
  const int row0 = b * kS;
  const float m = a.src.run_m[b], S = a.src.run_s[b];
  float q = 0.f;
  for (int q0 = threadIdx.x; q0 < kS; q0 += kPwBatch * kPwThreads) {
    float v[kPwBatch];
#pragma unroll
    for (int i = 0; i < kPwBatch; ++i) v[i] = pw_row(a.src, row0 + min(q0 + i * kPwThreads, kS - 1));
#pragma unroll
    for (int i = 0; i < kPwBatch; ++i) {
      if (q0 + i * kPwThreads >= kS) break;
      const float e = fexp(v[i] - m);            // lse_kernel's exponential: sum e is its run_s
      a.wt[row0 + q0 + i * kPwThreads] = __fdiv_rn(e, S);
      q += e * e;
    }
  }
  q = wave_sum(q);
  if (lane == 0) sq[wave] = q;
  __syncthreads();
  if (threadIdx.x == 0 && a.ess) {
    float Q = 0.f;
    for (int w = 0; w < kPwThreads / 64; ++w) Q += sq[w];
    a.ess[b] = __fdiv_rn(S * S, Q);
  }
  if (!a.sir) return;
  // SIR: thread 0 adds the stored weights in sample order, 2048 of them staged
  // through LDS at a time (8 independent reads ahead of their 8 dependent adds)
  const float u = a.u ? a.u[b] : philox_uniform4(a.seed, *a.rng_base, (unsigned)b, (unsigned)a.u_layer, 0u).x;
  float c = 0.f;
  int j = -1;
  for (int base = 0; base < kS; base += kPwThreads * kPwBatch) {
    __syncthreads();                              // the weights stored above; the previous batch scanned
#pragma unroll
    for (int i = 0; i < kPwBatch; ++i) {
      const int s = base + threadIdx.x + i * kPwThreads;
      sc[threadIdx.x + i * kPwThreads] = s < kS ? a.wt[row0 + s] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0 && j < 0) {
      const int n = min(kPwThreads * kPwBatch, kS - base);
      for (int s0 = 0; s0 < n; s0 += kPwBatch) {
        float w[kPwBatch];
#pragma unroll
        for (int i = 0; i < kPwBatch; ++i) w[i] = sc[s0 + i];
#pragma unroll
        for (int i = 0; i < kPwBatch; ++i) {
          c += w[i];
          if (j < 0 && s0 + i < n && c > u) j = base + s0 + i;
        }
      }
    }
  }
  if (threadIdx.x == 0) a.sir[b] = j < 0 ? kS - 1 : j;
}

hipError_t launch_post_weights(hipStream_t st, const PostWArgs& a) {
  if (a.src.Bimg <= 0) return hipSuccess;
  hipLaunchKernelGGL(post_weights_kernel, dim3(a.src.Bimg), dim3(kPwThreads), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------- pass 2, layer-wise
// One thread per (image, column), the image's n rows in sample order.
__global__ __launch_bounds__(256) void group_wsum_kernel(const float* __restrict__ H, int ldH, int n, int d, int N,
                                                         const float* __restrict__ wt, float* out, int ldo,
                                                         const int* sir, float* sel, int ldsel) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)N * d) return;
  const int b = (int)(i / d), j = (int)(i - (long long)b * d);
  const float* p = H + (size_t)b * n * ldH + j;
  const float* w = wt + (size_t)b * n;
  if (out) {
    float acc = 0.f;
    int s = 0;
    for (; s + 4 <= n; s += 4) {
      const float v0 = p[(size_t)s * ldH], v1 = p[(size_t)(s + 1) * ldH];
      const float v2 = p[(size_t)(s + 2) * ldH], v3 = p[(size_t)(s + 3) * ldH];
      acc = __builtin_fmaf(w[s], v0, acc);
      acc = __builtin_fmaf(w[s + 1], v1, acc);
      acc = __builtin_fmaf(w[s + 2], v2, acc);
      acc = __builtin_fmaf(w[s + 3], v3, acc);
    }
    for (; s < n; ++s) acc = __builtin_fmaf(w[s], p[(size_t)s * ldH], acc);
    out[(size_t)b * ldo + j] = acc;
  }
  if (sel) sel[(size_t)b * ldsel + j] = p[(size_t)sir[b] * ldH];
}
hipError_t launch_group_wsum(hipStream_t st, const float* H, int ldH, int n, int d, int N, const float* wt, float* out,
                             int ldo, const int* sir, float* sel, int ldsel) {
  const long long t = (long long)N * d;
  if (t <= 0 || (!out && !sel)) return hipSuccess;
  hipLaunchKernelGGL(group_wsum_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, st, H, ldH, n, d, N, wt, out,
                     ldo, sir, sel, ldsel);
  return hipGetLastError();
}

// ----------------------------------------------------------- pass 2, fused
// What a workgroup's lanes carry through the stages: the image, the chunk row
// of the workgroup's first sample, its live rows, the row (of the workgroup)
// that holds the image's resampled sample (or -1), the weights of the lane's
// rows rt * 16 + r, and the workgroup's partial vector.
template <int RT>
struct PoRows {
  int img, s0, row0, nrows, sir_row;
  float w[RT];
  float* part;
};

// sum over the 16 lanes that hold the same feature (lanes r = 0..15 of a lane group)
__device__ __forceinline__ float po_sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// Sampling epilogue (F:66-F:70).  Lane groups g hold, for quad q = 2t + (g >> 1),
// the mu quad (g even) or the zs quad (g odd); after swap(acc.x, acc.z) and
// swap(acc.y, acc.w) every lane holds (mu, zs) of its own two latent columns
// j = 4q + 2(g & 1) + {0, 1}.  h goes to LDS (split, with the ones column at d)
// when a later stage reads it, w~ h into the lane's sums, and the resampled
// row's h to the caller's buffer.
template <int RT>
__device__ __forceinline__ void po_head(const PoLaunch& L, const PoStage& S, int t, uint64_t base,
                                        const mg_f32x4 (&acc)[RT], const PoRows<RT>& R) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int q = 2 * t + (g >> 1);
  const int j0 = 4 * q + 2 * (g & 1);
  const int d = S.d;
  const MgBuf H = mg_buf<RT>(L, max(S.out_buf, 0));
  float* sel = L.h_sir[S.layer];
  float sum[2] = {0.f, 0.f};
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const auto p0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][0]), __float_as_uint(acc[rt][2]),
                                                     false, false);
    const auto p1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[rt][1]), __float_as_uint(acc[rt][3]),
                                                     false, false);
    const float mu[2] = {__uint_as_float(p0[0]), __uint_as_float(p1[0])};
    const float zs[2] = {__uint_as_float(p0[1]), __uint_as_float(p1[1])};
    const int row = rt * 16 + r;
    const int rowc = min(row, R.nrows - 1);                // clamped: a tail row repeats the last sample (weight 0)
    float2 e;
    if (L.eps[S.layer]) {
      // injected [k][N][d] noise; columns past d read 0 (masked below anyway)
      const float* ep = L.eps[S.layer] + ((size_t)(R.s0 + rowc) * L.eps_N + (L.eps_i0 + R.img)) * d;
      e.x = j0 < d ? ep[j0] : 0.f;
      e.y = j0 + 1 < d ? ep[j0 + 1] : 0.f;
    } else {
      e = philox_normal2(L.seed, base, (unsigned)(R.row0 + rowc), (unsigned)S.layer, (unsigned)q, (g & 1) != 0);
    }
    float hv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int j = j0 + c;
      const float sc = fexp(zs[c]) + kScaleEps;
      const float h = (c == 0 ? e.x : e.y) * sc + mu[c];
      hv[c] = j < d ? h : (j == d ? 1.f : 0.f);
      sum[c] = __builtin_fmaf(R.w[rt], h, sum[c]);
      if (sel && row == R.sir_row && j < d) sel[(size_t)R.img * d + j] = h;
    }
    if (S.out_buf >= 0) {                  // (uniform) a later stage reads this latent
      mg_bf16x2 vh, vl;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        vh[c] = (__bf16)hv[c];
        vl[c] = (__bf16)(hv[c] - (float)vh[c]);
      }
      *reinterpret_cast<mg_bf16x2*>(H.hi + row * H.ld + j0) = vh;
      *reinterpret_cast<mg_bf16x2*>(H.lo + row * H.ld + j0) = vl;
    }
    __builtin_amdgcn_sched_barrier(0);     // one row tile at a time (register pressure)
  }
  if (L.want_mean) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float v = po_sum16(sum[c]);
      if (r == 0 && j0 + c < d) R.part[S.part_off + j0 + c] = v;
    }
  }
}

// Output epilogue: p = sigmoid(acc) (1 - 1e-6) + 1e-7 (F:101-F:102, F:126) of
// features f0..f0+3 of the lane's rows, times their weights, summed over the
// workgroup's rows: one value per feature into the partial vector.
template <int RT>
__device__ __forceinline__ void po_out(const PoStage& S, int t, const mg_f32x4 (&acc)[RT], const PoRows<RT>& R) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int f0 = t * 16 + 4 * g;
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = __builtin_fmaf(frcp(1.f + fexp(-acc[rt][i])), kProbScale, kProbShift);
      sum[i] = __builtin_fmaf(R.w[rt], p, sum[i]);
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float v = po_sum16(sum[i]);
    if (r == 0 && f0 + i < S.N) R.part[S.part_off + f0 + i] = v;
  }
}

// The stage kind's epilogue, for the shared tile loop (mg_tiles)
template <int RT, int ACT>
struct PoEpi {
  static __device__ __forceinline__ void run(const PoLaunch& L, const PoStage& S, const MgBuf& OUT, int t,
                                             const mg_f32x4 (&acc)[RT], uint64_t base, const PoRows<RT>& R) {
    if (ACT == PO_TANH) mg_store_tanh<RT>(OUT, S, t, acc);
    else if (ACT == PO_OUT) po_out<RT>(S, t, acc, R);
    else po_head<RT>(L, S, t, base, acc, R);
  }
};

template <int RT>
__global__ __launch_bounds__(MG_WAVES * 64) void post_kernel(PoLaunch L) {
  constexpr int R = 16 * RT;
  constexpr int TPR = (MG_WAVES * 64) / R;       // threads per row in the prologue
  const int t = threadIdx.x;
  const uint64_t base = *L.rng_base;
  PoRows<RT> Rw;
  Rw.img = blockIdx.x / L.tiles;
  Rw.s0 = (blockIdx.x - Rw.img * L.tiles) * R;
  Rw.row0 = Rw.img * L.kS + Rw.s0;
  Rw.nrows = min(R, L.kS - Rw.s0);               // >= 1: tiles = ceil(kS / R)
  Rw.sir_row = L.sir ? L.sir[Rw.img] - Rw.s0 : -1;
  Rw.part = L.part + (size_t)blockIdx.x * L.ld_part;
  float* wl = mgs + L.w_off;
  if (t < R) wl[t] = t < Rw.nrows ? L.wt[Rw.row0 + t] : 0.f;
  // ---- prologue: h_1 = eps * s0 + mu0 of the image (F:58-F:60): split into
  // its LDS buffer with the ones column, and as f32 into the staging buffer
  // (a TANH buffer no stage has written yet) for the weighted sum over rows
  const int d0 = L.d0;
  float* stage = reinterpret_cast<float*>(reinterpret_cast<__bf16*>(mgs) + L.buf_off[L.stage_buf]);
  const int ld_stage = L.buf_ld[L.stage_buf];    // two bf16 planes of ld = ld floats per row
  {
    const MgBuf H = mg_buf<RT>(L, L.h0_buf);
    const int rr = t / TPR, sub = t - rr * TPR;
    const int rc = min(rr, Rw.nrows - 1);
    const float* Pp = L.P0 + (size_t)Rw.img * L.ldP0;
    const float* ep = L.eps[0] ? L.eps[0] + ((size_t)(Rw.s0 + rc) * L.eps_N + (L.eps_i0 + Rw.img)) * d0 : nullptr;
    float* sel = L.h_sir[0];
    for (int gq = sub; 4 * gq < L.h0_next_k; gq += TPR) {
      float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * gq < d0) {
        if (ep) {
          const int j = 4 * gq;
          e4 = make_float4(ep[j], ep[min(j + 1, d0 - 1)], ep[min(j + 2, d0 - 1)], ep[min(j + 3, d0 - 1)]);
        } else {
          e4 = philox_normal4(L.seed, base, (unsigned)(Rw.row0 + rc), 0u, (unsigned)gq);
        }
      }
      mg_bf16x4 vh, vl;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = 4 * gq + q;
        float hv = 0.f;
        if (j < d0) {
          const float sc = fexp(Pp[d0 + j]) + kScaleEps;
          hv = f4_at(e4, q) * sc + Pp[j];
          stage[rr * ld_stage + j] = hv;
          if (sel && rr == Rw.sir_row) sel[(size_t)Rw.img * d0 + j] = hv;
        } else if (j == d0) {
          hv = 1.f;
        }
        vh[q] = (__bf16)hv;
        vl[q] = (__bf16)(hv - (float)vh[q]);
      }
      *reinterpret_cast<mg_bf16x4*>(H.hi + rr * H.ld + 4 * gq) = vh;
      *reinterpret_cast<mg_bf16x4*>(H.lo + rr * H.ld + 4 * gq) = vl;
    }
  }
  mg_lds_barrier();
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) Rw.w[rt] = wl[rt * 16 + (t & 15)];
  // sum_s w~_s h_1: one column per thread, the rows in sample order (the first
  // stage does not write the staging buffer, and a barrier follows it)
  if (L.want_mean)
    for (int j = t; j < d0; j += MG_WAVES * 64) {
      float acc = 0.f;
      for (int rr = 0; rr < Rw.nrows; ++rr) acc = __builtin_fmaf(wl[rr], stage[rr * ld_stage + j], acc);
      Rw.part[j] = acc;
    }

  for (int s = 0; s < L.nst; ++s) {
    const PoStage& S = L.st[s];
    if (S.act == PO_TANH) mg_pad<RT, MG_WAVES>(mg_buf<RT>(L, S.out_buf), S.N, S.next_k);
    else if (S.act == PO_SAMPLE && S.out_buf >= 0) mg_pad<RT, MG_WAVES>(mg_buf<RT>(L, S.out_buf), S.d, S.next_k);
    switch (S.act) {     // one instantiation per stage kind: one epilogue per tile loop
      case PO_TANH: mg_tiles<RT, MG_WAVES, PoEpi<RT, PO_TANH>>(L, S, S.out_buf, base, Rw); break;
      case PO_SAMPLE: mg_tiles<RT, MG_WAVES, PoEpi<RT, PO_SAMPLE>>(L, S, S.in_buf, base, Rw); break;
      default: mg_tiles<RT, MG_WAVES, PoEpi<RT, PO_OUT>>(L, S, S.in_buf, base, Rw); break;
    }
    mg_lds_barrier();
  }
}

hipError_t launch_post(hipStream_t st, const PoLaunch& L, int rt, size_t lds_bytes) {
  if (L.Bimg <= 0 || L.kS <= 0) return hipSuccess;
  const dim3 grid((unsigned)(L.Bimg * L.tiles)), block(MG_WAVES * 64);
  switch (rt) {
    case 1: hipLaunchKernelGGL(post_kernel<1>, grid, block, lds_bytes, st, L); break;
    case 2: hipLaunchKernelGGL(post_kernel<2>, grid, block, lds_bytes, st, L); break;
    case 4: hipLaunchKernelGGL(post_kernel<4>, grid, block, lds_bytes, st, L); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t post_setup_attributes() {
  const void* fns[] = {(const void*)post_kernel<1>, (const void*)post_kernel<2>, (const void*)post_kernel<4>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// An image's partial vectors added in tile order: one thread per (image, column)
__global__ __launch_bounds__(256) void post_merge_kernel(PoMerge a) {
  const int c = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
  int g = 0;
  while (g < a.nseg && (c < a.off[g] || c >= a.off[g] + a.width[g])) ++g;
  if (g == a.nseg) return;
  const float* p = a.part + (size_t)b * a.tiles * a.ld_part + c;
  float acc = 0.f;
  for (int t = 0; t < a.tiles; ++t) acc += p[(size_t)t * a.ld_part];
  a.out[g][(size_t)b * a.ldo[g] + (c - a.off[g])] = acc;
}
hipError_t launch_post_merge(hipStream_t st, const PoMerge& a) {
  if (a.Bimg <= 0 || a.nseg <= 0) return hipSuccess;
  hipLaunchKernelGGL(post_merge_kernel, dim3((unsigned)a.Bimg, (unsigned)((a.ld_part + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace iwae
