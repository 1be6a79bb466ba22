// Pixel ML (include/espm_mu.h, "pixel ML"): the Poisson maximum-likelihood abundances of every pixel given the spectra D, over a
// subset M of the components, by EM with an optimality certificate and a stop of the pixel's own - the nested fits behind the
// likelihood-ratio presence test of espm_amd/presence.py.  The one ITERATING image pass: the same slab of X is walked once per EM
// pass, inside the kernel, and every pixel carries its own state (h, its pass count, done) in its thread.
//
//   geometry of diagk::pixel_kernel (mu_diag.hip): one pixel per thread, ESPM_DIAG_BLOCK pixels per workgroup, D staged UNPADDED
//   through LDS in chunks of ESPM_DIAG_CHUNK channels, the exact K a template argument; channel-major X is read coalesced across the
//   workgroup's pixels, pixel-major X goes through mu_image_pass.hpp's transposing tile
//   per entry and pass: y = max(D h, log_shift) (k FMAs), one division, one log where x > 0, k FMAs into q = D^T (x / y)
//   per pass: the scale N / S, the ratios r = q / s, the certificate gap = 2 N (max r - 1), the stop or the EM step - in registers
//   the pass loop runs AT MOST n_pass times (a bounded launch: the host loop of presence.py issues chunks and reads one integer
//   between them) and a workgroup leaves it as soon as all its pixels are done; a done lane keeps taking part in the barriers and
//   the staging and never writes.  D is staged once when it fits one chunk, once per pass and chunk otherwise.
//
// The state a call leaves is the state the next one starts from, and a pass is a function of the pixel's own registers and of values
// every pass reads afresh: n_pass = a then b gives the bits of a + b, and so do both layouts, every dtype that holds the counts, any
// slab and any neighbours.  No float atomics; the three integer counts go through block_count_add.  Only the narrow build
// (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry point as a stub.
#include <cmath>
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"
#include "mu_pixel_ml.hpp"   // the geometry, the walk and the argument checks, shared with mu_pixel_ml_newton.hip

namespace pmlk {

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(B) void pixel_ml_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                     Sums<K> s, uint32_t mask, double log_shift, double tol, int n_pass,
                                                     double* __restrict__ h_io, double* __restrict__ dev_o, double* __restrict__ gap_o,
                                                     int32_t* __restrict__ passes, uint8_t* __restrict__ done,
                                                     unsigned long long* __restrict__ counters) {
  __shared__ double ds[CH * K];
  __shared__ XT tile[PM ? tile_rows<XT>() * TP : 1];
  __shared__ uint32_t cnt_part[ESPM_PML_COUNTERS][B / 64];
  const int q0 = blockIdx.x * B;
  const int q = q0 + threadIdx.x;
  const bool valid = q < p;
  const bool entered = valid && done[q] == 0;   // the pixels this call may write
  if (__syncthreads_count(entered) == 0) return;   // (workgroup-uniform: counters[NOT_DONE] gets nothing from here)
  bool live = entered;
  int st = 0, np = 0;
  double h[K];
#pragma unroll
  for (int j = 0; j < K; ++j) h[j] = live ? h_io[(size_t)j * p + q] : 0.0;
  if (live) np = passes[q];

  double N = 0.0;
  walk<K, XT, PM, false>(x, ld, n, p, q0, d, ds, tile, false, live, [&](double xv, const double*) { N = N + xv; });

  const int m = __popc(mask);
  double dev = 0.0, gap = 0.0;
  if (live) {
    if (N == 0.0) {
#pragma unroll
      for (int j = 0; j < K; ++j) h[j] = 0.0;
      st = 1, live = false;
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (!((mask >> j) & 1u)) h[j] = 0.0;
        else if (np == 0 && !(h[j] > 0.0)) h[j] = N / ((double)m * s.v[j]) * 1e-3;
      }
    }
  }

  uint32_t n_un = 0, n_nf = 0;
  const bool one_chunk = n <= CH;
  for (int it = 0; it < n_pass; ++it) {
    if (__syncthreads_count(live) == 0) break;
    // 1: the scale of least deviance on the ray
    double S = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if ((mask >> j) & 1u) S = fma(s.v[j], h[j], S);
    const double f = N / S;
    double hn[K], qv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) hn[j] = h[j] * f, qv[j] = 0.0;   // (0 * f outside the mask: f is checked below)
    // 2: the channels
    double dv = 0.0;
    uint32_t un = 0;
    walk<K, XT, PM, true>(x, ld, n, p, q0, d, ds, tile, !one_chunk || it == 0, live, [&](double xv, const double* __restrict__ g) {
      double gj[K];
      double y = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        gj[j] = g[j];
        y = fma(gj[j], hn[j], y);
      }
      const bool floored = !(y >= log_shift);
      y = floored ? log_shift : y;
      const double inv = 1.0 / y;
      const double w = xv * inv;
      double t = y - xv;
      if (xv > 0) t = fma(xv, log(w), t);
      dv += t;
      un += (uint32_t)(floored && xv > 0);
#pragma unroll
      for (int j = 0; j < K; ++j) qv[j] = fma(gj[j], w, qv[j]);
    });
    if (live) {
      // 3, 4: the ratios and the certificate
      double r[K];
      double rmax = -INFINITY;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        r[j] = 0.0;
        if ((mask >> j) & 1u) {
          r[j] = qv[j] / s.v[j];
          rmax = fmax(rmax, r[j]);
        }
      }
      dev = 2.0 * dv;
      gap = 2.0 * N * (rmax - 1.0);
      // 5: the stop, or the EM step
      if (!(S > 0.0) || !isfinite(S) || !isfinite(dev) || !isfinite(gap)) {
        st = 2, live = false;
        n_nf = 1;
      } else if (gap <= tol) {
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = hn[j];
        st = 1, live = false;
        n_un = un;
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = hn[j] * r[j];
        np += 1;
      }
    }
  }

  if (entered) {
#pragma unroll
    for (int j = 0; j < K; ++j) h_io[(size_t)j * p + q] = h[j];
    dev_o[q] = dev;
    gap_o[q] = gap;
    passes[q] = np;
    done[q] = (uint8_t)st;
  }
  const uint32_t v[ESPM_PML_COUNTERS] = {live ? 1u : 0u, n_un, n_nf};
  block_count_add<ESPM_PML_COUNTERS, B / 64>(cnt_part, v, counters);
}

template <int K, typename XT>
int launch(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, uint32_t mask, double log_shift,
           double tol, int n_pass, double* h_io, double* dev, double* gap, int32_t* passes, uint8_t* done, unsigned long long* counters,
           hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)p + B - 1) / B)), block(B);
  const XT* xt = static_cast<const XT*>(x);
  Sums<K> sv;
  for (int j = 0; j < K; ++j) sv.v[j] = s[j];
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pixel_ml_kernel<K, XT, true>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, log_shift, tol, n_pass, h_io, dev, gap,
                       passes, done, counters);
  else
    hipLaunchKernelGGL((pixel_ml_kernel<K, XT, false>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, log_shift, tol, n_pass, h_io, dev, gap,
                       passes, done, counters);
  return check_hip(hipGetLastError(), "pixel ML launch");
}

}  // namespace pmlk
#endif

}  // namespace espm

using namespace espm;

extern "C" int espm_pixel_ml(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                             uint32_t mask, double log_shift, double tol, int n_pass, double* h_inout, double* dev, double* gap,
                             int32_t* passes, uint8_t* done, uint64_t* counters, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel ML: built into the 1..%d component library only", ESPM_PML_MAX_K);
#else
  const char* who = "pixel ML";
  if (k < 1 || k > ESPM_PML_MAX_K) return set_error(ESPM_EUNSUPPORTED, "%s: k=%d (1..%d components)", who, k, ESPM_PML_MAX_K);
  if (int rc = pmlk::check_args(who, x, x_dtype, x_layout, ld, n, p, d, s, k, mask, log_shift, tol, n_pass, h_inout, dev, gap, passes, done, counters))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (int rc = check_hip(hipMemsetAsync(cnt + ESPM_PML_NOT_DONE, 0, sizeof(unsigned long long), st), "pixel ML: zeroing the counter")) return rc;
  return dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return pmlk::launch<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, s, mask, log_shift, tol, n_pass,
                                                                             h_inout, dev, gap, passes, done, cnt, st);
    });
  });
#endif
}
