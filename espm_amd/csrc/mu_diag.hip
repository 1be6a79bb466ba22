// Per-pixel diagnostics of a fitted model (include/espm_mu.h, "pixel diagnostics"): the Poisson deviance of every pixel and the
// Cramer-Rao bound of its column of H given the spectra D = G W, in one fp64 pass over X.
//
//   one pixel per thread, ESPM_DIAG_BLOCK pixels per workgroup; D staged through LDS in chunks of ESPM_DIAG_CHUNK channels
//   per channel: y = max(D h, log_shift) (k FMAs), one division, one log where x > 0, k (k + 1) / 2 FMAs into the lower triangle of
//                F = D^T diag(1 / y) D, kept in registers
//   channel-major X is read coalesced across the workgroup's pixels; pixel-major X ((p, n), hyperspy's layout) goes through
//                mu_image_pass.hpp's transposing tile.  D is staged UNPADDED and every sum runs over the exact K (no KP here)
//   after the channels: root-free Cholesky F = L diag(d) L^T, the k forward solves for diag(F^-1), the constrained form under the
//                simplex - all on the template K, unrolled, in registers
//
// No float atomics (a pixel belongs to one thread); the only atomic is the integer count of singular pixels.  Only the narrow
// build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry point as a stub.
#include <cfloat>
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace diagk {

constexpr int B = ESPM_DIAG_BLOCK;
constexpr int CH = ESPM_DIAG_CHUNK;
constexpr int TP = B + 1;   // pixel stride of the pixel-major tile

__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // (i, j), j <= i, of the lower triangle

template <int K>
struct Acc {
  double h[K];
  double f[K * (K + 1) / 2];
  double dev;
  double floor_y;

  // one entry of X: its share of the deviance and of F
  __device__ __forceinline__ void add(double xv, const double* __restrict__ g) {
    double gj[K];
    double y = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      gj[j] = g[j];
      y = fma(gj[j], h[j], y);
    }
    y = fmax(y, floor_y);
    const double w = 1.0 / y;
    double t = y - xv;
    if (xv > 0) t = fma(xv, log(xv * w), t);
    dev += t;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double gw = gj[i] * w;
#pragma unroll
      for (int j = 0; j <= i; ++j) f[tri(i, j)] = fma(gw, gj[j], f[tri(i, j)]);
    }
  }
};

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(B) void pixel_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                  const double* __restrict__ h, double log_shift, int simplex, double* __restrict__ dev,
                                                  double* __restrict__ h_std, int32_t* __restrict__ n_singular) {
  __shared__ double ds[CH * K];
  const int q0 = blockIdx.x * B;
  const int q = q0 + threadIdx.x;
  const bool valid = q < p;
  Acc<K> a;
#pragma unroll
  for (int j = 0; j < K; ++j) a.h[j] = valid ? h[(size_t)j * p + q] : 1.0;
#pragma unroll
  for (int i = 0; i < K * (K + 1) / 2; ++i) a.f[i] = 0;
  a.dev = 0;
  a.floor_y = log_shift;

  for (int c0 = 0; c0 < n; c0 += CH) {
    const int cn = min(CH, n - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < cn * K; i += B) ds[i] = d[(size_t)c0 * K + i];
    __syncthreads();
    if constexpr (!PM) {
      if (valid) {
        const XT* xp = x + (size_t)c0 * ld + q;
#pragma unroll 4
        for (int c = 0; c < cn; ++c) a.add((double)xp[(size_t)c * ld], ds + c * K);
      }
    } else {
      constexpr int TS = tile_rows<XT>();
      __shared__ XT tile[TS * TP];
      for (int t0 = 0; t0 < cn; t0 += TS) {
        const int tn = min(TS, cn - t0);
        __syncthreads();   // (the tile's readers of the round before)
        fill_tile<XT, B>(tile, x, ld, q0, p, c0 + t0, tn);
        __syncthreads();
        if (valid)
          for (int c = 0; c < tn; ++c) a.add((double)tile[c * TP + threadIdx.x], ds + (t0 + c) * K);
      }
    }
  }

  // ---- F = L diag(dd) L^T (root-free Cholesky, in place: f holds L below the diagonal); a pivot not above K eps max diag(F): NaN
  double dmax = a.f[tri(0, 0)];
#pragma unroll
  for (int i = 1; i < K; ++i) dmax = fmax(dmax, a.f[tri(i, i)]);
  const double thr = (double)K * DBL_EPSILON * dmax;
  bool bad = false;
  double dd[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double dj = a.f[tri(j, j)];
#pragma unroll
    for (int m = 0; m < j; ++m) dj = fma(-(a.f[tri(j, m)] * a.f[tri(j, m)]), dd[m], dj);
    bad |= !(dj > thr);
    dd[j] = dj;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double v = a.f[tri(i, j)];
#pragma unroll
      for (int m = 0; m < j; ++m) v = fma(-(a.f[tri(i, m)] * a.f[tri(j, m)]), dd[m], v);
      a.f[tri(i, j)] = v / dj;
    }
  }
  // diag(F^-1)_i = sum_{j >= i} z_j^2 / dd_j with L z = e_i
  double cv[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double z[K];
    z[i] = 1.0;
    double s = z[i] * z[i] / dd[i];
#pragma unroll
    for (int j = i + 1; j < K; ++j) {
      double v = 0;
#pragma unroll
      for (int m = i; m < j; ++m) v = fma(-a.f[tri(j, m)], z[m], v);
      z[j] = v;
      s = fma(v, v / dd[j], s);
    }
    cv[i] = s;
  }
  if (simplex) {   // C = F^-1 - u u^T / (1^T u), u = F^-1 1: the bound under sum_i h_i = 1
    double v[K], u[K];
    double s = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      double t = 1.0;
#pragma unroll
      for (int m = 0; m < j; ++m) t = fma(-a.f[tri(j, m)], v[m], t);
      v[j] = t;
      u[j] = t / dd[j];
      s = fma(t, u[j], s);
    }
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
#pragma unroll
      for (int m = j + 1; m < K; ++m) u[j] = fma(-a.f[tri(m, j)], u[m], u[j]);
    }
#pragma unroll
    for (int i = 0; i < K; ++i) cv[i] = cv[i] - u[i] * (u[i] / s);
  }
  if (valid) {
    dev[q] = 2.0 * a.dev;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double c = cv[i];
      h_std[(size_t)i * p + q] = bad ? (double)NAN : sqrt(c < 0 ? 0.0 : c);   // (a rounding-negative variance is 0; a NaN stays)
    }
  }
  const int nbad = __syncthreads_count(valid && bad);
  if (n_singular && threadIdx.x == 0 && nbad) atomicAdd(n_singular, nbad);
}

template <int K, typename XT>
int launch(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, double log_shift, int simplex,
           double* dev, double* h_std, int32_t* n_singular, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + B - 1) / B)), block(B);
  const XT* xt = static_cast<const XT*>(x);
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pixel_kernel<K, XT, true>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, simplex, dev, h_std, n_singular);
  else
    hipLaunchKernelGGL((pixel_kernel<K, XT, false>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, simplex, dev, h_std, n_singular);
  return check_hip(hipGetLastError(), "pixel diagnostics launch");
}

}  // namespace diagk
#endif

}  // namespace espm

using namespace espm;

extern "C" int espm_pixel_diagnostics(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h,
                                      int k, double log_shift, int simplex, double* dev, double* h_std, int32_t* n_singular,
                                      espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel diagnostics: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (k < 1 || k > ESPM_DIAG_MAX_K) return set_error(ESPM_EUNSUPPORTED, "pixel diagnostics: k=%d (1..%d components)", k, ESPM_DIAG_MAX_K);
  ESPM_REQUIRE(x && d && h && dev && h_std && n >= 1 && p >= 1, "pixel diagnostics: bad arguments");
  if (int rc = check_image("pixel diagnostics", x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "pixel diagnostics: log_shift must be positive");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_singular)
    if (int rc = check_hip(hipMemsetAsync(n_singular, 0, sizeof(int32_t), s), "pixel diagnostics counter")) return rc;
  return dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return diagk::launch<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, h, log_shift, simplex, dev, h_std,
                                                                               n_singular, s);
    });
  });
#endif
}
