// Aggregate posterior q(h_1) = 1/M sum_m q(h_1 | x_m) at R query latents
// (iwae_aggregate): the pairwise log-densities of R rows
// under M diagonal Gaussians over d units, reduced by log-sum-exp over M.
//
//   t(r,m,j) = -1/2 z^2 - log s_mj - 1/2 log 2 pi,  z = (h_rj - mu_mj) (1 / s_mj)
//   J(r,m)   = sum_j t(r,m,j)                        (column order)
//   joint    logsumexp_m J(r,m) - log M              agg_joint_kernel
//   per unit logsumexp_m t(r,m,j) - log M            agg_dim_kernel
//
// Float32 in difference form: 1 / s and -(log s + 1/2 log 2 pi) come from one
// prep launch per call (agg_prep_kernel, [M][d] each), a term is a subtract, a
// multiply and a fused multiply-add.  Plain VALU: the square of a difference is
// not a product of a row factor and a reference factor, so the matrix cores
// could only serve the expanded form h^2 a - 2 h b + c, which cancels at small
// scales.  Every reduction has a fixed order, every output element has one
// writer, there are no atomics.
#include "iwae_kernels.h"

namespace iwae {
namespace {

constexpr int kAjLd = kAggJointCols + 4;      // LDS row stride of the joint kernel's tiles (floats): 16 lanes of a
                                              // ds_read_b128 group start 36 l mod 64 = 16 distinct 4-bank slots

__device__ __forceinline__ float agg_term(float hv, float mu, float rs, float lc) {
  const float z = (hv - mu) * rs;
  return __builtin_fmaf(-0.5f * z, z, lc);
}

// Running (max, sum) of a log-sum-exp, one exp per value.  v == -inf adds
// nothing (also to a max that is still -inf: no inf - inf); a NaN v makes the
// sum NaN.
__device__ __forceinline__ void lse_push(float& m, float& s, float v) {
  const float d = (v == -INFINITY) ? -INFINITY : v - m;
  const float e = fexp(-fabsf(d));
  if (d > 0.f) {
    s = __builtin_fmaf(s, e, 1.f);
    m = v;
  } else {
    s += e;
  }
}

// (m, s) <- (m, s) + (m2, s2): M* = max, S = s exp(m - M*) + s2 exp(m2 - M*)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  const float b = (mm == -INFINITY) ? 0.f : mm;
  const float a1 = s * fexp(m - b), a2 = s2 * fexp(m2 - b);
  s = a1 + a2;
  m = mm;
}

__global__ __launch_bounds__(256) void agg_prep_kernel(const float* __restrict__ scale, long long n,
                                                       float* __restrict__ rs, float* __restrict__ lc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float s = scale[i];
  rs[i] = 1.f / s;
  lc[i] = -(logf(s) + kHalfLog2Pi);
}

// Rows [row0, row0 + 64) x columns [j0, j0 + w) of src [nrows][d] into dst
// [64][kAjLd], zero outside the matrix (w a multiple of 4).
__device__ __forceinline__ void aj_load_tile(float* dst, const float* __restrict__ src, long long row0, long long nrows,
                                             int d, int j0, int w, int vec) {
  const int q4 = w >> 2;
  for (int i = threadIdx.x; i < kAggJointRows * q4; i += 256) {
    const int r = i / q4, jl = (i - r * q4) << 2, j = j0 + jl;
    const long long gr = row0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gr < nrows && j < d) {
      const float* p = src + (size_t)gr * d + j;
      if (vec) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v.x = p[0];
        if (j + 1 < d) v.y = p[1];
        if (j + 2 < d) v.z = p[2];
        if (j + 3 < d) v.w = p[3];
      }
    }
    *reinterpret_cast<float4*>(dst + r * kAjLd + jl) = v;
  }
}

// A workgroup owns 64 query rows and one segment of the references; thread
// (rg, lane) = (tid / 16, tid % 16) owns rows 4 rg .. 4 rg + 3 and references
// lane + 16 q of each 64-reference tile.  The rows' h and the tile's (mu, 1/s,
// lc) go through LDS in column chunks of at most 32, read back as float4; J is
// accumulated in column order in registers, then pushed into the row's running
// (max, sum).  The 16 lanes of a row are merged by a fixed xor butterfly.
__global__ __launch_bounds__(256) void agg_joint_kernel(AggArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[4][kAggJointRows * kAjLd];
  const int tid = threadIdx.x, lane = tid & 15, rg = tid >> 4;
  const long long row0 = (long long)blockIdx.x * kAggJointRows;
  const int m_begin = blockIdx.y * a.seg_len;
  const int m_end = min(a.M, m_begin + a.seg_len);
  const int nch = (a.d + kAggJointCols - 1) / kAggJointCols;
  const int w = ((a.d + nch - 1) / nch + 3) & ~3;
  float mx[4], sm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { mx[i] = -INFINITY; sm[i] = 0.f; }
  for (int m0 = m_begin; m0 < m_end; m0 += kAggJointRefs) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
    for (int c = 0; c < nch; ++c) {
      const int j0 = c * w;
      __syncthreads();
      if (nch > 1 || m0 == m_begin) aj_load_tile(sh[0], a.lat, row0, a.R, a.d, j0, w, a.vec);
      aj_load_tile(sh[1], a.mu, m0, m_end, a.d, j0, w, a.vec);
      aj_load_tile(sh[2], a.rs, m0, m_end, a.d, j0, w, a.vec);
      aj_load_tile(sh[3], a.lc, m0, m_end, a.d, j0, w, a.vec);
      __syncthreads();
      for (int j = 0; j < w; j += 4) {
        float4 hv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) hv[i] = *reinterpret_cast<const float4*>(&sh[0][(rg * 4 + i) * kAjLd + j]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int o = (lane + 16 * q) * kAjLd + j;
          const float4 mu = *reinterpret_cast<const float4*>(&sh[1][o]);
          const float4 rs = *reinterpret_cast<const float4*>(&sh[2][o]);
          const float4 lc = *reinterpret_cast<const float4*>(&sh[3][o]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = acc[i][q];
            v += agg_term(hv[i].x, mu.x, rs.x, lc.x);
            v += agg_term(hv[i].y, mu.y, rs.y, lc.y);
            v += agg_term(hv[i].z, mu.z, rs.z, lc.z);
            v += agg_term(hv[i].w, mu.w, rs.w, lc.w);
            acc[i][q] = v;
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (m0 + lane + 16 * q < m_end) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lse_push(mx[i], sm[i], acc[i][q]);
      }
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float m2 = __shfl_xor(mx[i], off, 16), s2 = __shfl_xor(sm[i], off, 16);
      float ma = up ? m2 : mx[i], sa = up ? s2 : sm[i];          // the lower lane's pair first, on both lanes
      lse_merge(ma, sa, up ? mx[i] : m2, up ? sm[i] : s2);
      mx[i] = ma; sm[i] = sa;
    }
  }
  if (lane != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long r = row0 + rg * 4 + i;
    if (r >= a.R) continue;
    if (a.nseg == 1) {
      a.out[r] = mx[i] + flog(sm[i]) - a.log_m;
    } else {
      float* p = a.part + ((size_t)r * a.nseg + blockIdx.y) * 2;
      p[0] = mx[i]; p[1] = sm[i];
    }
  }
}

// A thread owns one unit of four consecutive rows: the (row group, unit) pairs
// of a unit chunk (blockIdx.y, a.uw units wide; one chunk when d <= 256) are
// laid flat over the threads, so no lane idles at any d.  The references'
// (mu, 1/s, lc) of the chunk's units go through LDS a.tm at a time; the thread
// walks them in order, one exp per term, no cross-lane traffic.
__global__ __launch_bounds__(256) void agg_dim_kernel(AggArgs a) {
  __shared__ __attribute__((aligned(16))) float sh[3][kAggDimTile];
  const int tid = threadIdx.x;
  const int u0 = blockIdx.y * a.uw, wc = min(a.uw, a.d - u0);
  const long long nrg = (a.R + 3) >> 2;
  if ((long long)blockIdx.x * 256 / wc >= nrg) return;           // (the narrower last chunk needs fewer workgroups)
  const long long p = (long long)blockIdx.x * 256 + tid;
  const long long rg = p / wc;
  const int uu = (int)(p - rg * wc);
  const bool live = rg < nrg;
  const int m_begin = blockIdx.z * a.seg_len;
  const int m_end = min(a.M, m_begin + a.seg_len);
  float hv[4], mx[4], sm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long r = rg * 4 + i;
    hv[i] = (live && r < a.R) ? a.lat[(size_t)r * a.d + u0 + uu] : 0.f;
    mx[i] = -INFINITY; sm[i] = 0.f;
  }
  const float* src[3] = {a.mu, a.rs, a.lc};
  for (int m0 = m_begin; m0 < m_end; m0 += a.tm) {
    const int n = min(a.tm, m_end - m0);
    __syncthreads();
    if (wc == a.d) {                         // one chunk: the tile's rows are contiguous
      const size_t base = (size_t)m0 * a.d;
      const int cnt = n * a.d;
      if (a.vec) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          for (int i = tid * 4; i < cnt; i += 1024)
            *reinterpret_cast<float4*>(&sh[k][i]) = *reinterpret_cast<const float4*>(src[k] + base + i);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          for (int i = tid; i < cnt; i += 256) sh[k][i] = src[k][base + i];
      }
    } else {
      for (int i = tid; i < n * wc; i += 256) {
        const int ref = i / wc, u = i - ref * wc;
        const size_t g = (size_t)(m0 + ref) * a.d + u0 + u;
#pragma unroll
        for (int k = 0; k < 3; ++k) sh[k][i] = src[k][g];
      }
    }
    __syncthreads();
    if (live) {
      for (int ref = 0; ref < n; ++ref) {
        const int o = ref * wc + uu;
        const float mu = sh[0][o], rs = sh[1][o], lc = sh[2][o];
#pragma unroll
        for (int i = 0; i < 4; ++i) lse_push(mx[i], sm[i], agg_term(hv[i], mu, rs, lc));
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long r = rg * 4 + i;
    if (r >= a.R) continue;
    const size_t e = (size_t)r * a.d + u0 + uu;
    if (a.nseg == 1) {
      a.out[e] = mx[i] + flog(sm[i]) - a.log_m;
    } else {
      float* q = a.part + (e * a.nseg + blockIdx.z) * 2;
      q[0] = mx[i]; q[1] = sm[i];
    }
  }
}

// out[e] = the segments' (max, sum) partials [e][nseg][2] combined in segment
// order (iwae_nll_partials' rule): M* = max m, S = sum s exp(m - M*).
__global__ __launch_bounds__(256) void agg_merge_kernel(const float* __restrict__ part, long long n, int nseg, float log_m,
                                                        float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float* p = part + (size_t)e * nseg * 2;
  float mm = -INFINITY;
  for (int g = 0; g < nseg; ++g) mm = fmaxf(mm, p[2 * g]);
  const float b = (mm == -INFINITY) ? 0.f : mm;
  float s = 0.f;
  for (int g = 0; g < nseg; ++g) s += p[2 * g + 1] * fexp(p[2 * g] - b);
  out[e] = mm + flog(s) - log_m;
}

// Row r's own component o = (r_base + r) mod P: J(r, o) and t(r, o, j), one thread per row
__global__ __launch_bounds__(256) void agg_own_kernel(AggArgs a, int period, float* __restrict__ own,
                                                      float* __restrict__ own_dim) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const size_t o = (size_t)(r % period) * a.d, hr = (size_t)r * a.d;
  float acc = 0.f;
  for (int j = 0; j < a.d; ++j) {
    const float t = agg_term(a.lat[hr + j], a.mu[o + j], a.rs[o + j], a.lc[o + j]);
    acc += t;
    if (own_dim) own_dim[hr + j] = t;
  }
  if (own) own[r] = acc;
}

}  // namespace

hipError_t launch_agg_prep(hipStream_t st, const float* scale, long long n, float* rs, float* lc) {
  hipLaunchKernelGGL(agg_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scale, n, rs, lc);
  return hipGetLastError();
}

hipError_t launch_agg_joint(hipStream_t st, const AggArgs& a) {
  hipLaunchKernelGGL(agg_joint_kernel, dim3((unsigned)((a.R + kAggJointRows - 1) / kAggJointRows), a.nseg), dim3(256), 0,
                     st, a);
  return hipGetLastError();
}

hipError_t launch_agg_dim(hipStream_t st, const AggArgs& a) {
  const long long nrg = (a.R + 3) / 4;
  const int nuc = (a.d + a.uw - 1) / a.uw;
  hipLaunchKernelGGL(agg_dim_kernel, dim3((unsigned)((nrg * a.uw + 255) / 256), nuc, a.nseg), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_agg_merge(hipStream_t st, const float* part, long long n, int nseg, float log_m, float* out) {
  hipLaunchKernelGGL(agg_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, nseg, log_m, out);
  return hipGetLastError();
}

hipError_t launch_agg_own(hipStream_t st, const AggArgs& a, int period, float* own, float* own_dim) {
  hipLaunchKernelGGL(agg_own_kernel, dim3((unsigned)((a.R + 255) / 256)), dim3(256), 0, st, a, period, own, own_dim);
  return hipGetLastError();
}

}  // namespace iwae
