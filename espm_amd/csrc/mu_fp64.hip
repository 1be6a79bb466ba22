// fp64 mode of the multiplicative updates (include/espm_mu.h, "fp64 mode"): the log_surrogate H and W steps of
// espm/estimators/updates.py:6-156 in double precision, with the reference's simplex bisection (dicotomy.py:4-55, :111-173).
//
//   H pass      one workgroup per 256 pixels of X (channel-major), G W staged through LDS in chunks of ESPM_F64_CHUNK channels,
//               the k numerators of a pixel in registers; the loss pieces of the state ride in the same pass
//   bisection   two launches: every column bisects to maxit and ANDs the bitmask of its converged steps into a global mask;
//               then every column recomputes its midpoint to the lowest common step (no grid-wide barrier)
//   W pass      workgroups of (4 channels, ESPM_F64_WCHUNK pixels) write partial sums of R H^T, one launch adds them in order
//   W finish    one workgroup: G^T (R H^T), the denominators, the bisection over the rows, the clamp
//
// Every reduction is a fixed tree (wave shuffles in a fixed order, then the waves of a workgroup in order, then the workgroups
// in order): no float atomics, a fit is bit-identical from run to run.  Only the narrow build (ESPM_KP == 8) instantiates the
// kernels; the wide builds export the same entry points as stubs.
#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
namespace f64k {

constexpr int B = ESPM_F64_BLOCK;
constexpr int NW = B / WAVE;
constexpr int CPB = 4;   // channels per W-pass workgroup: H is read once for four channels

template <typename XT>
__device__ __forceinline__ double xval(const XT* x, size_t i);
template <>
__device__ __forceinline__ double xval<uint8_t>(const uint8_t* x, size_t i) { return (double)x[i]; }
template <>
__device__ __forceinline__ double xval<bf16_t>(const bf16_t* x, size_t i) { return (double)__uint_as_float((uint32_t)x[i] << 16); }
template <>
__device__ __forceinline__ double xval<float>(const float* x, size_t i) { return (double)x[i]; }
template <>
__device__ __forceinline__ double xval<double>(const double* x, size_t i) { return x[i]; }

// np.maximum(v, eps): a NaN stays NaN (fmax would drop it), as in the reference's residual (dicotomy.py:51-53)
__device__ __forceinline__ double nan_max(double v, double eps) { return v != v ? v : fmax(v, eps); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
  return v;   // lane 0
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, WAVE));
  return v;
}

// NV values per thread -> their workgroup totals (sum for i < nsum, max above), valid in every thread on return.
// sh: NW * NV doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_reduce(double (&v)[NV], int nsum, double* sh) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double r = i < nsum ? wave_sum(v[i]) : wave_max(v[i]);
    if (lane == 0) sh[wv * NV + i] = r;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double t = sh[i];
    for (int w = 1; w < NW; ++w) t = i < nsum ? t + sh[w * NV + i] : fmax(t, sh[w * NV + i]);
    v[i] = t;
  }
  __syncthreads();
}

// out[i] = the sum (i < nsum) or the maximum of part[b * nv + i] over b < nblk, in a fixed order.  One workgroup.
__global__ __launch_bounds__(B) void parts_kernel(const double* __restrict__ part, int nblk, int nv, int nsum, double* __restrict__ out) {
  __shared__ double sh[NW];
  for (int i = 0; i < nv; ++i) {
    const bool sum = i < nsum;
    double t = sum ? 0.0 : -INFINITY;
    for (int b = threadIdx.x; b < nblk; b += B) t = sum ? t + part[(size_t)b * nv + i] : fmax(t, part[(size_t)b * nv + i]);
    double v[1] = {t};
    block_reduce<1>(v, sum ? 1 : 0, sh);
    if (threadIdx.x == 0) out[i] = v[0];
  }
}

// ---- G W -----------------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(B) void gw_kernel(const double* __restrict__ g, const double* __restrict__ w, int n, int m, double eps,
                                               double* __restrict__ gw, int32_t* __restrict__ small) {
  const int c = blockIdx.x * B + threadIdx.x;
  int lo = 0;
  if (c < n) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double t;
      if (g) {
        t = 0;
        for (int i = 0; i < m; ++i) t = fma(g[(size_t)c * m + i], w[(size_t)i * K + j], t);
      } else {
        t = w[(size_t)c * K + j];
      }
      gw[(size_t)c * K + j] = t;
      lo |= t < eps;
    }
  }
  if (__syncthreads_or(lo) && threadIdx.x == 0) atomicOr(small, 1);   // (an integer flag: the order does not matter)
}

template <int K>
__global__ __launch_bounds__(B) void colsum_kernel(const double* __restrict__ a, int rows, double* __restrict__ out) {
  __shared__ double sh[NW * K];
  double v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = 0;
  for (int r = threadIdx.x; r < rows; r += B)
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] += a[(size_t)r * K + j];
  block_reduce<K>(v, K, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < K; ++j) out[j] = v[j];
}

// ---- statistics of H -----------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(B) void hstat_kernel(const double* __restrict__ h, int p, double eps, double* __restrict__ part) {
  __shared__ double sh[NW * 2 * K];
  const int q = blockIdx.x * B + threadIdx.x;
  double v[2 * K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double hc = q < p ? fmax(h[(size_t)j * p + q], eps) : 0.0;
    v[j] = hc;
    v[K + j] = hc;
  }
  block_reduce<2 * K>(v, K, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 2 * K; ++i) part[(size_t)blockIdx.x * 2 * K + i] = v[i];
}

// ---- the H pass ----------------------------------------------------------------------------------------------------------------
template <int K, typename XT>
__global__ __launch_bounds__(B) void h_pass_kernel(const XT* __restrict__ x, int n, int p, double xscale, const double* __restrict__ gw,
                                                   const double* __restrict__ colsum_gw, const int32_t* __restrict__ gw_small,
                                                   const double* __restrict__ h, const double* __restrict__ hstat,
                                                   const double* __restrict__ mu, double eps_reg, double lambda_L, double sigma, int nx,
                                                   int ny, double eps, int mode, const double* __restrict__ fixed_h,
                                                   double* __restrict__ h_out, double* __restrict__ num_out, double* __restrict__ den_out,
                                                   double* __restrict__ part) {
  extern __shared__ double gws[];   // (min(n, CHUNK), K)
  __shared__ double sh[NW * 3];
  const int q = blockIdx.x * B + threadIdx.x;
  const bool valid = q < p;
  const bool small = *gw_small != 0;
  double hr[K], hc[K], acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    hr[j] = valid ? h[(size_t)j * p + q] : 1.0;
    hc[j] = fmax(hr[j], eps);
    acc[j] = 0;
  }
  double kl = 0;
  for (int c0 = 0; c0 < n; c0 += ESPM_F64_CHUNK) {
    const int cn = min(ESPM_F64_CHUNK, n - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < cn * K; i += B) gws[i] = gw[(size_t)c0 * K + i];
    __syncthreads();
    if (valid) {
      const XT* xp = x + (size_t)c0 * p + q;
      for (int c = 0; c < cn; ++c) {
        const double xv = xval<XT>(xp, (size_t)c * p) * xscale;
        const double* g = gws + c * K;
        double y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) y = fma(g[j], hc[j], y);
        if (mode) {
          // R = X / Y; a Y of 0 (a zero row of G W) is the reference's X / max(Y, eps) (updates.py:129-131): its G W entries are 0
          const double r = xv / (y != 0 ? y : eps);
#pragma unroll
          for (int j = 0; j < K; ++j) acc[j] = fma(g[j], r, acc[j]);
        }
        double yl = y;   // the loss clamps G W (measures.py:493-504)
        if (small) {
          yl = 0;
#pragma unroll
          for (int j = 0; j < K; ++j) yl = fma(fmax(g[j], eps), hc[j], yl);
        }
        kl += yl - fmax(xv, eps) * log(yl);
      }
    }
  }
  double reg = 0, lap = 0;
  if (valid) {
    double hl[K];
    if (nx > 0) {   // (H L)[j, q] = deg(q) H[j, q] - sum of the 4-neighbours, zero-flux boundary (utils.py:39-76)
      const int r = q / ny, cc = q - r * ny;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double* hj = h + (size_t)j * p;
        double s = 0, deg = 0;
        if (r > 0) { s += hj[q - ny]; deg += 1; }
        if (r < nx - 1) { s += hj[q + ny]; deg += 1; }
        if (cc > 0) { s += hj[q - 1]; deg += 1; }
        if (cc < ny - 1) { s += hj[q + 1]; deg += 1; }
        hl[j] = deg * hr[j] - s;
      }
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) hl[j] = hr[j];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      reg += mu[j] * log(hr[j] + eps_reg);
      lap += hr[j] * hl[j];
    }
    if (mode) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        // updates.py:127-141, in the reference's order of operations
        double num = acc[j];
        double den = colsum_gw[j] + mu[j] / (hc[j] + eps_reg);
        if (lambda_L != 0) {
          const double t = lambda_L * sigma * hstat[K + j];
          num = num + t;
          den = den + t + lambda_L * hl[j];
        }
        num = hc[j] * num;
        const size_t e = (size_t)j * p + q;
        if (mode == 2) {
          num_out[e] = num;
          den_out[e] = den;
        } else {
          double v = fmax(num / den, eps);
          if (fixed_h && fixed_h[e] >= 0) v = fixed_h[e];
          h_out[e] = v;
        }
      }
    }
  }
  double v[3] = {kl, reg, lap};
  block_reduce<3>(v, 3, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 3; ++i) part[(size_t)blockIdx.x * 3 + i] = v[i];
}

// ---- the reference's bisection (dicotomy.py:17-55, :111-173) -----------------------------------------------------------------
template <int K>
struct Col {
  double num[K], den[K];
  double eps;
  __device__ __forceinline__ double f(double x) const {   // dicotomy.py:51-53: sum_i max(num_i / (nu + den_i), eps) - 1
    double s = nan_max(num[0] / (x + den[0]), eps);
#pragma unroll
    for (int i = 1; i < K; ++i) s += nan_max(num[i] / (x + den[i]), eps);
    return s - 1;
  }
  // bracket and its check; false: the reference's assertions fail for this column
  __device__ __forceinline__ bool bracket(double& a, double& b, double& fa) const {
    double nmax = num[0], dmin = den[0], nsum = 0;
    bool ok = true;
    a = -INFINITY;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      ok = ok && num[i] >= 0 && den[i] >= 0;
      nsum += num[i];
      nmax = fmax(nmax, num[i]);
      dmin = fmin(dmin, den[i]);
      if (num[i] > 0) a = fmax(a, num[i] / 2 - den[i]);
    }
    b = (double)K * nmax / 0.5 - dmin;
    if (!ok || !(nsum > 0)) return false;
    fa = f(a);
    const double fb = f(b);
    return !(fb >= 0 || fa <= 0 || isnan(fa) || isnan(fb));
  }
};

template <int K>
__global__ __launch_bounds__(B) void bisect_scan_kernel(const double* __restrict__ num, const double* __restrict__ den, int p, double eps,
                                                        double tol, int maxit, unsigned long long* __restrict__ mask,
                                                        int32_t* __restrict__ status) {
  __shared__ unsigned long long m[2];
  if (threadIdx.x == 0) m[0] = m[1] = ~0ull;
  __syncthreads();
  const int q = blockIdx.x * B + threadIdx.x;
  unsigned long long b0 = ~0ull, b1 = ~0ull;
  if (q < p) {
    Col<K> col;
    col.eps = eps;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      col.num[i] = num[(size_t)i * p + q];
      col.den[i] = den[(size_t)i * p + q];
    }
    double a, b, fa;
    if (col.bracket(a, b, fa)) {
      b0 = b1 = 0;
      double mid = (a + b) / 2, fm = col.f(mid);
      for (int s = 0;; ++s) {
        if (fabs(fm) <= tol) {
          if (s < 64) b0 |= 1ull << s; else b1 |= 1ull << (s - 64);
        }
        if (s >= maxit) break;
        if (fa * fm <= 0) b = mid;
        else { a = mid; fa = fm; }   // (f(a) at the new a is f(mid): the same evaluation the reference repeats)
        mid = (a + b) / 2;
        fm = col.f(mid);
      }
    } else {
      atomicAdd(status, 1);
    }
  }
  atomicAnd(&m[0], b0);
  atomicAnd(&m[1], b1);
  __syncthreads();
  if (threadIdx.x == 0) {   // (integer AND: the order does not matter)
    atomicAnd(&mask[0], m[0]);
    atomicAnd(&mask[1], m[1]);
  }
}

template <int K>
__global__ __launch_bounds__(B) void bisect_apply_kernel(const double* __restrict__ num, const double* __restrict__ den, int p, double eps,
                                                         int maxit, const unsigned long long* __restrict__ mask,
                                                         const double* __restrict__ fixed_h, double* __restrict__ h_out) {
  const int q = blockIdx.x * B + threadIdx.x;
  if (q >= p) return;
  const unsigned long long m0 = mask[0], m1 = mask[1];
  int stop = m0 ? __ffsll((long long)m0) - 1 : (m1 ? 64 + __ffsll((long long)m1) - 1 : maxit);
  stop = min(stop, maxit);
  Col<K> col;
  col.eps = eps;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    col.num[i] = num[(size_t)i * p + q];
    col.den[i] = den[(size_t)i * p + q];
  }
  double a, b, fa;
  double nu = NAN;
  if (col.bracket(a, b, fa)) {
    double mid = (a + b) / 2, fm = col.f(mid);
    for (int s = 0; s < stop; ++s) {
      if (fa * fm <= 0) b = mid;
      else { a = mid; fa = fm; }
      mid = (a + b) / 2;
      fm = col.f(mid);
    }
    nu = mid;
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const size_t e = (size_t)i * p + q;
    double v = fmax(col.num[i] / (col.den[i] + nu), eps);
    if (fixed_h && fixed_h[e] >= 0) v = fixed_h[e];
    h_out[e] = v;
  }
}

// ---- relative change (base.py:323-324) -----------------------------------------------------------------------------------------
constexpr int REL_PER = 8;   // entries per thread
__global__ __launch_bounds__(B) void rel_sum_kernel(const double* __restrict__ a, int64_t count, double* __restrict__ part) {
  __shared__ double sh[NW];
  const int64_t base = (int64_t)blockIdx.x * B * REL_PER + threadIdx.x;
  double s = 0;
  for (int r = 0; r < REL_PER; ++r) {
    const int64_t e = base + (int64_t)r * B;
    if (e < count) s += a[e];
  }
  double v[1] = {s};
  block_reduce<1>(v, 1, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(B) void rel_max_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t count, double tol,
                                                    const double* __restrict__ total, double* __restrict__ part) {
  __shared__ double sh[NW];
  const double shift = tol * (*total / (double)count);
  const int64_t base = (int64_t)blockIdx.x * B * REL_PER + threadIdx.x;
  double m = -INFINITY;
  for (int r = 0; r < REL_PER; ++r) {
    const int64_t e = base + (int64_t)r * B;
    if (e < count) m = fmax(m, fabs(a[e] - b[e]) / (a[e] + shift));
  }
  double v[1] = {m};
  block_reduce<1>(v, 0, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v[0];
}

// ---- the W pass: partial sums of (X / Y) H^T -----------------------------------------------------------------------------------
template <int K, typename XT>
__global__ __launch_bounds__(B) void w_accum_kernel(const XT* __restrict__ x, int n, int p, double xscale, const double* __restrict__ gw,
                                                    const double* __restrict__ h, double eps, double* __restrict__ part) {
  __shared__ double sh[NW * CPB * K];
  const int c0 = blockIdx.y * CPB;
  const int q0 = blockIdx.x * ESPM_F64_WCHUNK, q1 = min(p, q0 + ESPM_F64_WCHUNK);
  double g[CPB][K], acc[CPB * K];
#pragma unroll
  for (int c = 0; c < CPB; ++c)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      g[c][j] = c0 + c < n ? gw[(size_t)(c0 + c) * K + j] : 0.0;
      acc[c * K + j] = 0;
    }
  for (int q = q0 + threadIdx.x; q < q1; q += B) {
    double hc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) hc[j] = fmax(h[(size_t)j * p + q], eps);
#pragma unroll
    for (int c = 0; c < CPB; ++c) {
      if (c0 + c < n) {
        const double xv = xval<XT>(x, (size_t)(c0 + c) * p + q) * xscale;
        double y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) y = fma(g[c][j], hc[j], y);
        const double r = xv / (y != 0 ? y : eps);   // (updates.py:54-56)
#pragma unroll
        for (int j = 0; j < K; ++j) acc[c * K + j] = fma(r, hc[j], acc[c * K + j]);
      }
    }
  }
  block_reduce<CPB * K>(acc, CPB * K, sh);
  if (threadIdx.x < CPB * K) {
    const int c = threadIdx.x / K, j = threadIdx.x - c * K;
    if (c0 + c < n) {
      double t = 0;
#pragma unroll
      for (int i = 0; i < CPB * K; ++i) t = i == threadIdx.x ? acc[i] : t;
      part[((size_t)blockIdx.x * n + c0 + c) * K + j] = t;
    }
  }
}

__global__ __launch_bounds__(B) void w_parts_kernel(const double* __restrict__ part, int nchunk, int64_t nk, double* __restrict__ rh) {
  const int64_t e = (int64_t)blockIdx.x * B + threadIdx.x;
  if (e >= nk) return;
  double t = 0;
  for (int c = 0; c < nchunk; ++c) t += part[(size_t)c * nk + e];
  rh[e] = t;
}

// ---- the W finish: one workgroup ------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(B) void w_finish_kernel(const double* __restrict__ rh, const double* __restrict__ g,
                                                     const double* __restrict__ colsum_g, int n, int m, const double* __restrict__ w,
                                                     const double* __restrict__ hstat, int simplex, const uint8_t* __restrict__ rows,
                                                     int nrows, double eps, double tol, int maxit, const double* __restrict__ fixed_w,
                                                     double* __restrict__ w_out, int32_t* __restrict__ status) {
  __shared__ double sh[NW * 4 * K];
  __shared__ double nu_s[K];
  const int M = g ? m : n;
  // numerators W (G^T R H^T) into w_out (updates.py:58-59), denominators colsum(G) rowsum(H) recomputed where needed
  for (int e = threadIdx.x; e < M * K; e += B) {
    const int i = e / K, j = e - i * K;
    double t;
    if (g) {
      t = 0;
      for (int c = 0; c < n; ++c) t = fma(g[(size_t)c * m + i], rh[(size_t)c * K + j], t);
    } else {
      t = rh[e];
    }
    w_out[e] = fmax(w[e], eps) * t;
  }
  __syncthreads();
  auto den_of = [&](int i, int j) { return (g ? colsum_g[i] : 1.0) * hstat[j]; };
  auto in_rows = [&](int i) { return rows == nullptr || rows[i] != 0; };
  if (threadIdx.x < K) nu_s[threadIdx.x] = 0;
  if (simplex) {
    // bracket of every column (dicotomy.py:17-49) over the rows under the simplex
    double v[4 * K];   // [a | nmax | -dmin | nsum]; plus the precondition check
    int bad = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      v[j] = -INFINITY;
      v[K + j] = -INFINITY;
      v[2 * K + j] = -INFINITY;
      v[3 * K + j] = 0;
    }
    for (int i = threadIdx.x; i < M; i += B) {
      if (!in_rows(i)) continue;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double nm = w_out[(size_t)i * K + j], dn = den_of(i, j);
        bad |= !(nm >= 0 && dn >= 0);
        if (nm > 0) v[j] = fmax(v[j], nm / 2 - dn);
        v[K + j] = fmax(v[K + j], nm);
        v[2 * K + j] = fmax(v[2 * K + j], -dn);
        v[3 * K + j] += nm;
      }
    }
    // (the sums go first in block_reduce: reorder into [nsum | a | nmax | -dmin])
    double r[4 * K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      r[j] = v[3 * K + j];
      r[K + j] = v[j];
      r[2 * K + j] = v[K + j];
      r[3 * K + j] = v[2 * K + j];
    }
    block_reduce<4 * K>(r, K, sh);
    bad = __syncthreads_or(bad);
    double a[K], b[K], fa[K], fm[K], mid[K];
    bool ok = !bad;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      ok = ok && r[j] > 0;
      a[j] = r[K + j];
      b[j] = (double)nrows * r[2 * K + j] / 0.5 - (-r[3 * K + j]);
    }
    // f of all K columns at x (K values), reduced over the rows in a fixed order
    auto feval = [&](const double (&xx)[K], double (&out)[K]) {
      double s[K];
#pragma unroll
      for (int j = 0; j < K; ++j) s[j] = 0;
      for (int i = threadIdx.x; i < M; i += B) {
        if (!in_rows(i)) continue;
#pragma unroll
        for (int j = 0; j < K; ++j) s[j] += nan_max(w_out[(size_t)i * K + j] / (xx[j] + den_of(i, j)), eps);
      }
      block_reduce<K>(s, K, sh);
#pragma unroll
      for (int j = 0; j < K; ++j) out[j] = s[j] - 1;
    };
    if (ok) {
      double fb[K];
      feval(a, fa);
      feval(b, fb);
#pragma unroll
      for (int j = 0; j < K; ++j) ok = ok && !(fb[j] >= 0 || fa[j] <= 0 || isnan(fa[j]) || isnan(fb[j]));
    }
    if (!ok) {
      if (threadIdx.x == 0) atomicAdd(status, 1);
      if (threadIdx.x < K) nu_s[threadIdx.x] = NAN;
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) mid[j] = (a[j] + b[j]) / 2;
      feval(mid, fm);
      for (int s = 0;; ++s) {
        bool conv = true;
#pragma unroll
        for (int j = 0; j < K; ++j) conv = conv && fabs(fm[j]) <= tol;
        if (conv || s >= maxit) break;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (fa[j] * fm[j] <= 0) b[j] = mid[j];
          else { a[j] = mid[j]; fa[j] = fm[j]; }
          mid[j] = (a[j] + b[j]) / 2;
        }
        feval(mid, fm);
      }
      if (threadIdx.x < K) {
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (j == (int)threadIdx.x) nu_s[j] = mid[j];
      }
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < M * K; e += B) {
    const int i = e / K, j = e - i * K;
    const double den = in_rows(i) ? den_of(i, j) + nu_s[j] : den_of(i, j);
    double v = fmax(w_out[e] / den, eps);
    if (fixed_w && fixed_w[e] >= 0) v = fixed_w[e];
    w_out[e] = v;
  }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------------------
inline int nblk_of(int64_t count, int64_t per) { return (int)((count + per - 1) / per); }

template <int K, typename XT>
int launch_h_pass(const void* x, int n, int p, double xscale, const double* gw, const double* colsum_gw, const int32_t* gw_small, const double* h,
                  const double* hstat, const double* mu, double eps_reg, double lambda_L, double sigma, int nx, int ny, double eps, int mode,
                  const double* fixed_h, double* h_out, double* num, double* den, double* part, hipStream_t s) {
  const size_t lds = (size_t)min(n, ESPM_F64_CHUNK) * K * sizeof(double);
  auto kern = h_pass_kernel<K, XT>;
  static bool attr = false;   // (the attribute once per instantiation)
  if (!attr) {
    if (int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)((size_t)ESPM_F64_CHUNK * K * sizeof(double))), "fp64 H pass LDS"))
      return rc;
    attr = true;
  }
  hipLaunchKernelGGL(kern, dim3(nblk_of(p, B)), dim3(B), lds, s, static_cast<const XT*>(x), n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu,
                     eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part);
  return check_hip(hipGetLastError(), "fp64 H pass launch");
}

template <int K>
int launch_h_pass_x(const void* x, int x_type, int n, int p, double xscale, const double* gw, const double* colsum_gw, const int32_t* gw_small,
                    const double* h, const double* hstat, const double* mu, double eps_reg, double lambda_L, double sigma, int nx, int ny,
                    double eps, int mode, const double* fixed_h, double* h_out, double* num, double* den, double* part, hipStream_t s) {
  switch (x_type) {
    case ESPM_F64_X_U8:
      return launch_h_pass<K, uint8_t>(x, n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part, s);
    case ESPM_F64_X_BF16:
      return launch_h_pass<K, bf16_t>(x, n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part, s);
    case ESPM_F64_X_F32:
      return launch_h_pass<K, float>(x, n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part, s);
    case ESPM_F64_X_F64:
      return launch_h_pass<K, double>(x, n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part, s);
    default:
      return set_error(ESPM_EINVAL, "fp64 H pass: x_type %d", x_type);
  }
}

template <int K, typename XT>
int launch_w_accum(const void* x, int n, int p, double xscale, const double* gw, const double* h, double eps, double* part, double* rh,
                   hipStream_t s) {
  const int nchunk = nblk_of(p, ESPM_F64_WCHUNK);
  hipLaunchKernelGGL((w_accum_kernel<K, XT>), dim3(nchunk, nblk_of(n, CPB)), dim3(B), 0, s, static_cast<const XT*>(x), n, p, xscale, gw, h,
                     eps, part);
  if (int rc = check_hip(hipGetLastError(), "fp64 W pass launch")) return rc;
  const int64_t nk = (int64_t)n * K;
  hipLaunchKernelGGL(w_parts_kernel, dim3(nblk_of(nk, B)), dim3(B), 0, s, part, nchunk, nk, rh);
  return check_hip(hipGetLastError(), "fp64 W pass reduction launch");
}

}  // namespace f64k
#endif

}  // namespace espm

using namespace espm;

#define F64_REQUIRE_BUILD()                                                                                                  \
  do {                                                                                                                       \
    if (ESPM_KP != 8) return set_error(ESPM_EUNSUPPORTED, "fp64 mode: built into the 1..%d component library only", ESPM_F64_MAX_K); \
  } while (0)

#define F64_K_SWITCH(k, ...)          \
  switch (k) {                         \
    case 1: { constexpr int K = 1; __VA_ARGS__; } \
    case 2: { constexpr int K = 2; __VA_ARGS__; } \
    case 3: { constexpr int K = 3; __VA_ARGS__; } \
    case 4: { constexpr int K = 4; __VA_ARGS__; } \
    case 5: { constexpr int K = 5; __VA_ARGS__; } \
    case 6: { constexpr int K = 6; __VA_ARGS__; } \
    case 7: { constexpr int K = 7; __VA_ARGS__; } \
    case 8: { constexpr int K = 8; __VA_ARGS__; } \
    default: return set_error(ESPM_EUNSUPPORTED, "fp64 mode: k=%d (1..%d components)", k, ESPM_F64_MAX_K); \
  }

extern "C" {

int64_t espm_f64_scratch_doubles(int n, int p, int k, int64_t count) {
  const int64_t hb = (p + ESPM_F64_BLOCK - 1) / ESPM_F64_BLOCK;
  const int64_t rb = (count + ESPM_F64_BLOCK * 8 - 1) / (ESPM_F64_BLOCK * 8);
  const int64_t wc = (p + ESPM_F64_WCHUNK - 1) / ESPM_F64_WCHUNK;
  int64_t need = hb * 3;
  need = need > hb * 2 * k ? need : hb * 2 * k;
  need = need > 2 * rb + 2 ? need : 2 * rb + 2;
  need = need > wc * n * k ? need : wc * n * k;
  return need;
}

int espm_f64_gw(const double* g, const double* w, int n, int m, int k, double log_shift, double* gw, double* colsum, int32_t* small,
                espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(w && gw && colsum && small && n >= 1 && (g == nullptr || m >= 1), "fp64 gw: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(small, 0, sizeof(int32_t), s), "fp64 gw flag")) return rc;
  F64_K_SWITCH(k, {
    hipLaunchKernelGGL(f64k::gw_kernel<K>, dim3(f64k::nblk_of(n, f64k::B)), dim3(f64k::B), 0, s, g, w, n, m, log_shift, gw, small);
    if (int rc = check_hip(hipGetLastError(), "fp64 gw launch")) return rc;
    hipLaunchKernelGGL(f64k::colsum_kernel<K>, dim3(1), dim3(f64k::B), 0, s, gw, n, colsum);
    return check_hip(hipGetLastError(), "fp64 colsum launch");
  })
#endif
  return ESPM_OK;
}

int espm_f64_hstat(const double* h, int k, int p, double log_shift, double* scratch, double* out, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(h && scratch && out && p >= 1, "fp64 hstat: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = f64k::nblk_of(p, f64k::B);
  F64_K_SWITCH(k, {
    hipLaunchKernelGGL(f64k::hstat_kernel<K>, dim3(nb), dim3(f64k::B), 0, s, h, p, log_shift, scratch);
    if (int rc = check_hip(hipGetLastError(), "fp64 hstat launch")) return rc;
    hipLaunchKernelGGL(f64k::parts_kernel, dim3(1), dim3(f64k::B), 0, s, scratch, nb, 2 * K, K, out);
    return check_hip(hipGetLastError(), "fp64 hstat reduction launch");
  })
#endif
  return ESPM_OK;
}

int espm_f64_h_pass(const void* x, int x_type, int n, int p, double xscale, const double* gw, const double* colsum_gw,
                    const int32_t* gw_small, const double* h, int k, const double* hstat, const double* mu, double eps_reg,
                    double lambda_L, double sigma, int nx, int ny, double log_shift, int mode, const double* fixed_h, double* h_out,
                    double* num, double* den, double* scratch, double* hist_row, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(x && gw && colsum_gw && gw_small && h && mu && scratch && hist_row && n >= 1 && p >= 1, "fp64 H pass: bad arguments");
  ESPM_REQUIRE(mode >= 0 && mode <= 2 && (mode != 1 || h_out) && (mode != 2 || (num && den)), "fp64 H pass: mode %d without its outputs", mode);
  ESPM_REQUIRE(lambda_L == 0 || hstat, "fp64 H pass: lambda_L without the statistics of H");
  ESPM_REQUIRE(nx == 0 || (nx >= 1 && ny >= 1 && (int64_t)nx * ny == p), "fp64 H pass: grid %d x %d does not match p=%d", nx, ny, p);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = ESPM_OK;
  F64_K_SWITCH(k, {
    rc = f64k::launch_h_pass_x<K>(x, x_type, n, p, xscale, gw, colsum_gw, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma, nx, ny, log_shift,
                                  mode, fixed_h, h_out, num, den, scratch, s);
    break;
  })
  if (rc) return rc;
  hipLaunchKernelGGL(f64k::parts_kernel, dim3(1), dim3(f64k::B), 0, s, scratch, f64k::nblk_of(p, f64k::B), 3, 3, hist_row);
  return check_hip(hipGetLastError(), "fp64 loss reduction launch");
#endif
  return ESPM_OK;
}

int espm_f64_bisect(const double* num, const double* den, int k, int p, double log_shift, double tol, int maxit,
                    const double* fixed_h, double* h_out, uint64_t* mask, int32_t* status, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(num && den && h_out && mask && status && p >= 1, "fp64 bisection: bad arguments");
  ESPM_REQUIRE(maxit >= 0 && maxit <= ESPM_F64_MAXIT, "fp64 bisection: maxit=%d (0..%d)", maxit, ESPM_F64_MAXIT);
  if (log_shift > 0 && (double)k * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(mask, 0xff, 2 * sizeof(uint64_t), s), "fp64 bisection mask")) return rc;
  const int nb = f64k::nblk_of(p, f64k::B);
  unsigned long long* m = reinterpret_cast<unsigned long long*>(mask);
  F64_K_SWITCH(k, {
    hipLaunchKernelGGL(f64k::bisect_scan_kernel<K>, dim3(nb), dim3(f64k::B), 0, s, num, den, p, log_shift, tol, maxit, m, status);
    if (int rc = check_hip(hipGetLastError(), "fp64 bisection scan launch")) return rc;
    hipLaunchKernelGGL(f64k::bisect_apply_kernel<K>, dim3(nb), dim3(f64k::B), 0, s, num, den, p, log_shift, maxit, m, fixed_h, h_out);
    return check_hip(hipGetLastError(), "fp64 bisection apply launch");
  })
#endif
  return ESPM_OK;
}

int espm_f64_rel(const double* a, const double* b, int64_t count, double tol, double* scratch, double* out, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(a && b && scratch && out && count >= 1, "fp64 rel: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = f64k::nblk_of(count, f64k::B * f64k::REL_PER);
  double* sums = scratch;
  double* total = scratch + nb;
  double* maxes = scratch + nb + 1;
  hipLaunchKernelGGL(f64k::rel_sum_kernel, dim3(nb), dim3(f64k::B), 0, s, a, count, sums);
  hipLaunchKernelGGL(f64k::parts_kernel, dim3(1), dim3(f64k::B), 0, s, sums, nb, 1, 1, total);
  hipLaunchKernelGGL(f64k::rel_max_kernel, dim3(nb), dim3(f64k::B), 0, s, a, b, count, tol, total, maxes);
  hipLaunchKernelGGL(f64k::parts_kernel, dim3(1), dim3(f64k::B), 0, s, maxes, nb, 1, 0, out);
  return check_hip(hipGetLastError(), "fp64 rel launch");
#endif
  return ESPM_OK;
}

int espm_f64_w_accum(const void* x, int x_type, int n, int p, double xscale, const double* gw, const double* h, int k, double log_shift,
                     double* scratch, double* rh, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(x && gw && h && scratch && rh && n >= 1 && p >= 1, "fp64 W pass: bad arguments");
  ESPM_REQUIRE((n + f64k::CPB - 1) / f64k::CPB <= 65535, "fp64 W pass: n=%d channels", n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  F64_K_SWITCH(k, {
    switch (x_type) {
      case ESPM_F64_X_U8: return f64k::launch_w_accum<K, uint8_t>(x, n, p, xscale, gw, h, log_shift, scratch, rh, s);
      case ESPM_F64_X_BF16: return f64k::launch_w_accum<K, bf16_t>(x, n, p, xscale, gw, h, log_shift, scratch, rh, s);
      case ESPM_F64_X_F32: return f64k::launch_w_accum<K, float>(x, n, p, xscale, gw, h, log_shift, scratch, rh, s);
      case ESPM_F64_X_F64: return f64k::launch_w_accum<K, double>(x, n, p, xscale, gw, h, log_shift, scratch, rh, s);
      default: return set_error(ESPM_EINVAL, "fp64 W pass: x_type %d", x_type);
    }
  })
#endif
  return ESPM_OK;
}

int espm_f64_w_finish(const double* rh, const double* g, const double* colsum_g, int n, int m, int k, const double* w,
                      const double* hstat, int simplex, const uint8_t* rows, int nrows, double log_shift, double tol, int maxit,
                      const double* fixed_w, double* w_out, int32_t* status, espm_stream_t stream) {
  F64_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(rh && w && hstat && w_out && status && n >= 1 && (g == nullptr || (colsum_g && m >= 1)), "fp64 W finish: bad arguments");
  ESPM_REQUIRE(w != w_out, "fp64 W finish: w and w_out must differ");
  const int M = g ? m : n;
  ESPM_REQUIRE(!simplex || (rows ? (nrows >= 1 && nrows <= M) : nrows == M), "fp64 W finish: %d rows under the simplex of %d", nrows, M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (simplex && log_shift > 0 && (double)nrows * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  F64_K_SWITCH(k, {
    hipLaunchKernelGGL(f64k::w_finish_kernel<K>, dim3(1), dim3(f64k::B), 0, s, rh, g, colsum_g, n, m, w, hstat, simplex, rows, nrows,
                       log_shift, tol, maxit, fixed_w, w_out, status);
    return check_hip(hipGetLastError(), "fp64 W finish launch");
  })
#endif
  return ESPM_OK;
}

}  // extern "C"
