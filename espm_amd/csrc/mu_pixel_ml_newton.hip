// Pixel ML by a safeguarded Newton step (include/espm_mu.h, "pixel ML, Newton"): the per-pixel Poisson maximum-likelihood problem of
// mu_pixel_ml.hip - the same certificate, the same stop, the same outputs - reached in tens of passes where EM takes hundreds to
// thousands.  A unit of its own: mu_pixel_ml.hip, whose rule is defined bit for bit, compiles to what it compiled to without it.
//
//   geometry and walk of pmlk::pixel_ml_kernel (mu_pixel_ml.hpp): one pixel per thread, ESPM_DIAG_BLOCK pixels per workgroup, D staged
//   UNPADDED through LDS in chunks of ESPM_DIAG_CHUNK channels, the exact K a template argument, mu_image_pass.hpp's transposing tile
//   for pixel-major X, ascending fma sums
//   per entry and pass: EM's y, w, dev and q, and K (K + 1) / 2 FMAs into the lower triangle of A = D^T diag(x / y^2) D
//   (diagk::pixel_kernel's triangle with another weight) - the live set of the walk is the scaled h, q and the triangle
//   per pass, between walks: the certificate and the stop as in EM; then the accept / reject test of the trial the pass evaluated, and
//   for an accepted point B = A + tau diag(s / hn), its root-free Cholesky (mu_diag.hip's), the step and the fraction-to-boundary
//   clamp.  e (the EM successor of the accepted point), dev_acc, tau and trial live in the caller's `state` and are read and written
//   HERE only, never carried over a walk in registers.
//
// Components outside the mask take part in the factorisation as rows of the identity with a zero right-hand side: their pivot is 1,
// their step 0, and every sum over them adds an exact zero - the arithmetic of the |M| x |M| system, unrolled over the template K.
// The walk of a channel-major thread keeps 4 entries in flight up to K = 6 and 1 at K = 7, 8, where the triangle leaves no room for more at
// two waves per SIMD (measured at the headline size: 4.7 - 4.8 ms per pass with 4 in flight and one wave, 3.1 - 3.3 ms with 1 and two).
// Resumable as the EM kernel is: everything a pass reads is h_io, passes, done, dev, gap and state, all rewritten by the call.
// No float atomics; the three integer counts go through block_count_add.  Only the narrow build (ESPM_KP == 8) instantiates the
// kernels; the wide builds export the entry point as a stub.
#include <cmath>
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"
#include "mu_pixel_ml.hpp"

namespace pmlk {

__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // (i, j), j <= i, of the lower triangle

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(B) void pixel_ml_newton_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                            Sums<K> s, uint32_t mask, double log_shift, double tol, int n_pass,
                                                            double* __restrict__ h_io, double* __restrict__ dev_o, double* __restrict__ gap_o,
                                                            int32_t* __restrict__ passes, uint8_t* __restrict__ done,
                                                            double* __restrict__ state, unsigned long long* __restrict__ counters) {
  constexpr int T = K * (K + 1) / 2;
  __shared__ double ds[CH * K];
  __shared__ XT tile[PM ? tile_rows<XT>() * TP : 1];
  __shared__ uint32_t cnt_part[ESPM_PML_COUNTERS][B / 64];
  const int q0 = blockIdx.x * B;
  const int q = q0 + threadIdx.x;
  const bool valid = q < p;
  const bool entered = valid && done[q] == 0;   // the pixels this call may write
  if (__syncthreads_count(entered) == 0) return;   // (workgroup-uniform: counters[NOT_DONE] gets nothing from here)
  // the pixel's rows of state (k + ESPM_PMLN_STATE_EXTRA, p): e, then dev_acc, tau, trial
  double* const st_e = state + q;
  double* const st_acc = state + (size_t)K * p + q;
  double* const st_tau = state + (size_t)(K + 1) * p + q;
  double* const st_trial = state + (size_t)(K + 2) * p + q;
  bool live = entered;
  int st = 0, np = 0;
  double h[K];
#pragma unroll
  for (int j = 0; j < K; ++j) h[j] = live ? h_io[(size_t)j * p + q] : 0.0;
  double dev = 0.0, gap = 0.0;
  if (live) {
    np = passes[q];
    if (np > 0) dev = dev_o[q], gap = gap_o[q];   // of the last accepted point: a rejected pass leaves them
  }

  double N = 0.0;
  walk<K, XT, PM, false>(x, ld, n, p, q0, d, ds, tile, false, live, [&](double xv, const double*) { N = N + xv; });

  const int m = __popc(mask);
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
      if (np == 0) {   // the start of the extra state
#pragma unroll
        for (int j = 0; j < K; ++j) st_e[(size_t)j * p] = 0.0;
        *st_acc = INFINITY, *st_tau = 1e-2, *st_trial = 0.0;
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
    double qv[K], a[T];
    if (live) {   // h as the pass found it: what the stop that is not finite leaves.  Parked in h_io, not in registers, over the walk
#pragma unroll
      for (int j = 0; j < K; ++j) h_io[(size_t)j * p + q] = h[j];
#pragma unroll
      for (int j = 0; j < K; ++j) h[j] = h[j] * f;   // h is hn from here on (0 * f outside the mask: f is checked below); a done lane keeps its h
    }
#pragma unroll
    for (int j = 0; j < K; ++j) qv[j] = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i) a[i] = 0.0;
    // 2: the channels
    double dv = 0.0;
    uint32_t un = 0;
    walk<K, XT, PM, true, (K >= 7 ? 1 : 4)>(x, ld, n, p, q0, d, ds, tile, !one_chunk || it == 0, live, [&](double xv, const double* __restrict__ g) {
      double gj[K];
      double y = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        gj[j] = g[j];
        y = fma(gj[j], h[j], y);
      }
      const bool floored = !(y >= log_shift);
      y = floored ? log_shift : y;
      const double inv = 1.0 / y;
      const double w = xv * inv;
      double t = y - xv;
      if (xv > 0) t = fma(xv, log(w), t);
      dv += t;
      un += (uint32_t)(floored && xv > 0);
      const double wy = w * inv;   // x / y^2
#pragma unroll
      for (int j = 0; j < K; ++j) qv[j] = fma(gj[j], w, qv[j]);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const double gw = gj[i] * wy;
#pragma unroll
        for (int j = 0; j <= i; ++j) a[tri(i, j)] = fma(gw, gj[j], a[tri(i, j)]);
      }
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
      const double dev_t = 2.0 * dv;
      const double gap_t = 2.0 * N * (rmax - 1.0);
      // 5: the stop that is not finite; the trial rejected; or the point accepted, and then the stop or the next trial
      if (!(S > 0.0) || !isfinite(S) || !isfinite(dev_t) || !isfinite(gap_t)) {
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = h_io[(size_t)j * p + q];
        dev = dev_t, gap = gap_t;
        st = 2, live = false;
        n_nf = 1;
      } else {
        double tau = *st_tau;
        const bool trial = *st_trial != 0.0;
        if (trial && !(dev_t <= *st_acc)) {   // rejected: the EM successor of the accepted point, and a heavier blend
#pragma unroll
          for (int j = 0; j < K; ++j) h[j] = st_e[(size_t)j * p];
          *st_trial = 0.0;
          *st_tau = fmin(10.0 * tau, 1.0);
          np += 1;
        } else {
          dev = dev_t, gap = gap_t;
          if (gap <= tol) {   // (h as scaled in 1)
            st = 1, live = false;
            n_un = un;
          } else {
            if (trial) tau = fmax(tau / 10.0, 1e-8);
            // B = A_MM + tau diag(s / hn) in place, the identity outside the mask; the right-hand side -g = q - s
            double z[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
              const bool mi = (mask >> i) & 1u;
              r[i] = h[i] * r[i];   // e: the EM successor
              st_e[(size_t)i * p] = r[i];
              z[i] = mi ? -(s.v[i] - qv[i]) : 0.0;
#pragma unroll
              for (int j = 0; j < i; ++j)
                if (!(mi && ((mask >> j) & 1u))) a[tri(i, j)] = 0.0;
              a[tri(i, i)] = mi ? fma(tau, s.v[i] / h[i], a[tri(i, i)]) : 1.0;
            }
            // B = L diag(dd) L^T (root-free Cholesky, in place: a holds L below the diagonal)
            bool bad = false;
            double dd[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
              double dj = a[tri(j, j)];
#pragma unroll
              for (int l = 0; l < j; ++l) dj = fma(-(a[tri(j, l)] * a[tri(j, l)]), dd[l], dj);
              bad |= !(dj > 0.0) || !isfinite(dj);
              dd[j] = dj;
#pragma unroll
              for (int i = j + 1; i < K; ++i) {
                double v = a[tri(i, j)];
#pragma unroll
                for (int l = 0; l < j; ++l) v = fma(-(a[tri(i, l)] * a[tri(j, l)]), dd[l], v);
                a[tri(i, j)] = v / dj;
              }
            }
            // L z = -g; z = z / dd; L^T delta = z
#pragma unroll
            for (int j = 0; j < K; ++j) {
#pragma unroll
              for (int l = 0; l < j; ++l) z[j] = fma(-a[tri(j, l)], z[l], z[j]);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) z[j] = z[j] / dd[j];
#pragma unroll
            for (int j = K - 1; j >= 0; --j) {
#pragma unroll
              for (int l = j + 1; l < K; ++l) z[j] = fma(-a[tri(l, j)], z[l], z[j]);
            }
            // the trial: never below 0.01 hn (fraction to the boundary), never 0; a pivot that is no pivot: the EM step
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const double cand = fmax(fmax(h[j] + z[j], 0.01 * h[j]), 1e-30 * N / s.v[j]);
              h[j] = bad ? r[j] : (((mask >> j) & 1u) ? cand : 0.0);
            }
            *st_acc = dev;
            *st_tau = tau;
            *st_trial = bad ? 0.0 : 1.0;
            np += 1;
          }
        }
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
int launch_newton(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, uint32_t mask, double log_shift,
                  double tol, int n_pass, double* h_io, double* dev, double* gap, int32_t* passes, uint8_t* done, double* state,
                  unsigned long long* counters, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)p + B - 1) / B)), block(B);
  const XT* xt = static_cast<const XT*>(x);
  Sums<K> sv;
  for (int j = 0; j < K; ++j) sv.v[j] = s[j];
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pixel_ml_newton_kernel<K, XT, true>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, log_shift, tol, n_pass, h_io, dev,
                       gap, passes, done, state, counters);
  else
    hipLaunchKernelGGL((pixel_ml_newton_kernel<K, XT, false>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, log_shift, tol, n_pass, h_io, dev,
                       gap, passes, done, state, counters);
  return check_hip(hipGetLastError(), "pixel ML (Newton) launch");
}

}  // namespace pmlk
#endif

}  // namespace espm

using namespace espm;

extern "C" int espm_pixel_ml_newton(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                                    uint32_t mask, double log_shift, double tol, int n_pass, double* h_inout, double* dev, double* gap,
                                    int32_t* passes, uint8_t* done, uint64_t* counters, void* state, size_t state_bytes,
                                    espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel ML (Newton): built into the 1..%d component library only", ESPM_PML_MAX_K);
#else
  const char* who = "pixel ML (Newton)";
  if (k < 1 || k > ESPM_PML_MAX_K) return set_error(ESPM_EUNSUPPORTED, "%s: k=%d (1..%d components)", who, k, ESPM_PML_MAX_K);
  if (int rc = pmlk::check_args(who, x, x_dtype, x_layout, ld, n, p, d, s, k, mask, log_shift, tol, n_pass, h_inout, dev, gap, passes, done, counters))
    return rc;
  ESPM_REQUIRE(state && state_bytes >= ESPM_PMLN_STATE_BYTES(k, p), "%s: state %p of %zu bytes (%zu needed for k=%d, p=%d)", who, state,
               state_bytes, (size_t)ESPM_PMLN_STATE_BYTES(k, p), k, p);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (int rc = check_hip(hipMemsetAsync(cnt + ESPM_PML_NOT_DONE, 0, sizeof(unsigned long long), st), "pixel ML (Newton): zeroing the counter"))
    return rc;
  return dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return pmlk::launch_newton<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, s, mask, log_shift, tol, n_pass,
                                                                                    h_inout, dev, gap, passes, done,
                                                                                    static_cast<double*>(state), cnt, st);
    });
  });
#endif
}
