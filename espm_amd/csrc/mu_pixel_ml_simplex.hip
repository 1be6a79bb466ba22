// Pixel ML on the simplex (include/espm_mu.h, "pixel ML, simplex"): the per-pixel Poisson maximum-likelihood problem of
// mu_pixel_ml_pinned.hip with the fitted abundances held to sum_M h = total, total = 1 - t where component `pin` is held at the
// pixel's own t and 1 where nothing is pinned (pin = -1) - the pixel problem of a simplex_H fit, the reduced fits of its presence
// test and the points of its profile likelihood.  A unit of its own: the other three pixel ML units compile to what they compiled to
// without it.
//
//   geometry and walk of pmlk::pixel_ml_pinned_kernel: one pixel per thread, ESPM_DIAG_BLOCK pixels per workgroup, D staged UNPADDED
//   through LDS in chunks of ESPM_DIAG_CHUNK channels, the exact K a template argument, mu_image_pass.hpp's transposing tile for
//   pixel-major X, ascending fma sums, 4 entries in flight up to K = 6 and 1 at K = 7, 8
//   per entry and pass: the pinned rule's y (the pinned term included), w, dev, q and triangle
//   per pass, between walks: no scale onto the ray and no N (the sum is constrained: there is no free scale); the Frank-Wolfe
//   certificate 2 (lin - total gmin) and the slope 2 (g_pin - lin / total); the Newton rule's accept / reject test; the EM successor
//   with the multiplier of the sum constraint found by a Newton iteration of its own; ONE root-free Cholesky of the blended matrix
//   and TWO solves with it (the step, and the direction the equality multiplier acts along), the clamp and the rescale onto the sum.
//
// `pin` is uniform over the launch and never indexes a register array: every use is a select inside an unrolled loop.
// Resumable as the pinned kernel is; a pixel that enters with done != 0 is never read or written beyond its done byte, and a
// workgroup with none entered returns at once.  No float atomics.  Only the narrow build (ESPM_KP == 8) instantiates the kernels;
// the wide builds export the entry point as a stub.
#include <cmath>
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"
#include "mu_pixel_ml.hpp"

namespace pmlk {

__device__ __forceinline__ constexpr int stri(int i, int j) { return i * (i + 1) / 2 + j; }   // (i, j), j <= i, of the lower triangle

// a - b c with the product ROUNDED (never contracted into an fma): exactly 0 where a is that same rounded product - what makes the
// certificate of a pixel at a vertex, and of a set of one component, exactly 0
__device__ __forceinline__ double sub_product(double a, double b, double c) {
#pragma clang fp contract(off)
  const double bc = b * c;
  return a - bc;
}

constexpr int NU_ITER = 64;   // the multiplier's Newton iteration: at most this many steps

// K = 8, channel-major is asked for two waves per SIMD where the pinned kernel asks (it fits 234 VGPRs); no other instance needs
// asking to reach the pinned kernel's waves per SIMD, and K = 8 pixel-major gets two for its one (profiles/pixel_ml_simplex_resources.txt)
template <int K, bool PM>
constexpr int simplex_waves() {
  return (K == 8 && !PM) ? 2 : 1;
}

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(B) __attribute__((amdgpu_waves_per_eu(simplex_waves<K, PM>()))) void pixel_ml_simplex_kernel(
    const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d, Sums<K> s, uint32_t mask, int pin,
    const double* __restrict__ t_in, double log_shift, double tol, int n_pass, double* __restrict__ h_io, double* __restrict__ dev_o,
    double* __restrict__ gap_o, double* __restrict__ slope_o, int32_t* __restrict__ passes, uint8_t* __restrict__ done,
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
  const bool pinned = pin >= 0;
  bool live = entered;
  int st = 0, np = 0;
  double h[K];
#pragma unroll
  for (int j = 0; j < K; ++j) h[j] = live ? h_io[(size_t)j * p + q] : 0.0;
  // dev, gap and slope are those of the last accepted point and live in the caller's arrays: written HERE when a point is accepted
  // (a rejected pass leaves them), never carried over a walk in registers; t is what h[pin] holds from the entry on
  double tq = 0.0;
  if (live) {
    np = passes[q];
    if (pinned) tq = t_in[q];
    if (np == 0) {
      dev_o[q] = 0.0, gap_o[q] = 0.0;
      if (pinned) slope_o[q] = 0.0;
    }
  }

  uint32_t n_un = 0, n_nf = 0;
  const int m = __popc(mask);
  if (live) {
    if (!(tq >= 0.0 && tq <= 1.0)) {   // no point of the profile: h, dev, gap and slope stay as the call found them (0 before any pass)
      st = 2, live = false;
      n_nf = 1;
    } else {
      if (np == 0) {
        const double total = 1.0 - tq;   // the start: lifted off the boundary and scaled onto the sum; and the start of the extra state
        const double lift = 1e-3 * total / (double)m;
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if ((mask >> j) & 1u) {
            h[j] = fmax(h[j], lift);
            sum = sum + h[j];
          }
        const double scale = total / sum;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          h[j] = h[j] * scale;
          if (m == 1 || total == 0.0) h[j] = total;
          st_e[(size_t)j * p] = 0.0;
        }
        *st_acc = INFINITY, *st_tau = 1e-2, *st_trial = 0.0;
      }
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j == pin) h[j] = tq;
        else if (!((mask >> j) & 1u)) h[j] = 0.0;
      }
    }
  }

  const bool one_chunk = n <= CH;
  for (int it = 0; it < n_pass; ++it) {
    if (__syncthreads_count(live) == 0) break;
    double qv[K], a[T];
#pragma unroll
    for (int j = 0; j < K; ++j) qv[j] = 0.0;
#pragma unroll
    for (int i = 0; i < T; ++i) a[i] = 0.0;
    // the channels, at h as it stands
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
        for (int j = 0; j <= i; ++j) a[stri(i, j)] = fma(gw, gj[j], a[stri(i, j)]);
      }
    });
    if (live) {
      // the certificate and the slope: lin = grad . h / 2, gmin the least component of grad / 2 over the set
      // total = 1 - t is formed HERE from h[pin], pass by pass: carried over the walk it costs every instance up to K = 4 a wave per
      // SIMD, and K = 8 scratch (profiles/pixel_ml_simplex_resources.txt)
      double total = 1.0;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j == pin) total = 1.0 - h[j];
      double lin = 0.0, gmin = INFINITY, gp = 0.0, hq = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double gj = s.v[j] - qv[j];
        if ((mask >> j) & 1u) {
          lin = fma(gj, h[j], lin);
          hq = fma(h[j], qv[j], hq);
          gmin = fmin(gmin, gj);
        }
        if (j == pin) gp = gj;
      }
      const double dev_t = 2.0 * dv;
      const double gap_t = m == 0 ? 0.0 : 2.0 * sub_product(lin, total, gmin);
      const double sl = 2.0 * (m == 0 ? gp : (total == 0.0 ? gp - gmin : gp - lin / total));
      // the stop that is not finite; the trial rejected; or the point accepted, and then the stop or the next trial
      if (!isfinite(dev_t) || !isfinite(gap_t)) {   // (h is as the pass found it)
        dev_o[q] = dev_t, gap_o[q] = gap_t;
        if (pinned) slope_o[q] = sl;
        st = 2, live = false;
        n_nf = 1;
      } else {
        double tau = *st_tau;
        const bool trial = *st_trial != 0.0;
        if (trial && !(dev_t <= *st_acc)) {   // rejected: the EM successor of the accepted point, and a heavier blend
#pragma unroll
          for (int j = 0; j < K; ++j) h[j] = (j == pin) ? h[j] : st_e[(size_t)j * p];
          *st_trial = 0.0;
          *st_tau = fmin(10.0 * tau, 1.0);
          np += 1;
        } else {
          dev_o[q] = dev_t, gap_o[q] = gap_t;
          if (pinned) slope_o[q] = sl;
          if (gap_t <= tol) {
            st = 1, live = false;
            n_un = un;
          } else if (hq == 0.0) {
            // no modelled count: the deviance is linear in h_M with the gradient 2 s, least at the vertex of the smallest s (the
            // lowest index on ties), where the next pass certifies
            int best = -1;
            double sbest = INFINITY;
#pragma unroll
            for (int j = 0; j < K; ++j)
              if (((mask >> j) & 1u) && s.v[j] < sbest) sbest = s.v[j], best = j;
#pragma unroll
            for (int j = 0; j < K; ++j) {
              h[j] = (j == pin) ? h[j] : (j == best ? total : 0.0);
              st_e[(size_t)j * p] = (j == pin) ? 0.0 : h[j];
            }
            *st_acc = dev_t;
            *st_trial = 0.0;
            np += 1;
          } else {
            if (trial) tau = fmax(tau / 10.0, 1e-8);
            // e, the EM successor on the simplex: n_j = h_j q_j / total, e_j = total n_j / (s_j + nu) with nu the root of
            // sum n_j / (s_j + nu) = 1, by Newton from the left (psi is convex and decreasing: the iteration rises)
            double r[K];
            double nu = -INFINITY;
            const double itot = 1.0 / total;
#pragma unroll
            for (int j = 0; j < K; ++j) {
              r[j] = ((mask >> j) & 1u) ? (h[j] * qv[j]) * itot : 0.0;
              if (r[j] > 0.0) nu = fmax(nu, r[j] - s.v[j]);
            }
#pragma unroll 1
            for (int i = 0; i < NU_ITER; ++i) {
              double psi = 0.0, dps = 0.0;
#pragma unroll
              for (int j = 0; j < K; ++j)
                if (r[j] > 0.0) {
                  const double iv = 1.0 / (s.v[j] + nu);
                  const double c = r[j] * iv;
                  psi = psi + c;
                  dps = fma(c, iv, dps);
                }
              const double next = nu + (psi - 1.0) / dps;
              if (!(next > nu)) break;
              nu = next;
            }
            double se = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
              r[j] = r[j] > 0.0 ? total * (r[j] * (1.0 / (s.v[j] + nu))) : 0.0;
              se = se + r[j];
            }
            se = total / se;
#pragma unroll
            for (int j = 0; j < K; ++j) st_e[(size_t)j * p] = r[j] * se;
            // B = A over the ACTIVE set (in M with h > 0: an abundance at exactly 0 stays there, as under EM) with
            // B_jj = fma(tau, max(q_j, s_j) / h_j, A_jj), the identity elsewhere (the pinned row too); z = -g = q - s, v = 1
            double z[K], v[K];
#pragma unroll
            for (int i = 0; i < K; ++i) {
              const bool mi = ((mask >> i) & 1u) && h[i] > 0.0;
              z[i] = mi ? -(s.v[i] - qv[i]) : 0.0;
              v[i] = mi ? 1.0 : 0.0;
#pragma unroll
              for (int j = 0; j < i; ++j)
                if (!(mi && ((mask >> j) & 1u) && h[j] > 0.0)) a[stri(i, j)] = 0.0;
              a[stri(i, i)] = mi ? fma(tau, fmax(qv[i], s.v[i]) / h[i], a[stri(i, i)]) : 1.0;
            }
            // B = L diag(dd) L^T (root-free Cholesky, in place: a holds L below the diagonal)
            bool bad = false;
            double dd[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
              double dj = a[stri(j, j)];
#pragma unroll
              for (int l = 0; l < j; ++l) dj = fma(-(a[stri(j, l)] * a[stri(j, l)]), dd[l], dj);
              bad |= !(dj > 0.0) || !isfinite(dj);
              dd[j] = dj;
#pragma unroll
              for (int i = j + 1; i < K; ++i) {
                double w = a[stri(i, j)];
#pragma unroll
                for (int l = 0; l < j; ++l) w = fma(-(a[stri(i, l)] * a[stri(j, l)]), dd[l], w);
                a[stri(i, j)] = w / dj;
              }
            }
            // L z = -g, L v = 1; each / dd; L^T u = z, L^T v = v: the two solves share every load of L
#pragma unroll
            for (int j = 0; j < K; ++j) {
#pragma unroll
              for (int l = 0; l < j; ++l) {
                z[j] = fma(-a[stri(j, l)], z[l], z[j]);
                v[j] = fma(-a[stri(j, l)], v[l], v[j]);
              }
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const double id = 1.0 / dd[j];
              z[j] = z[j] * id, v[j] = v[j] * id;
            }
#pragma unroll
            for (int j = K - 1; j >= 0; --j) {
#pragma unroll
              for (int l = j + 1; l < K; ++l) {
                z[j] = fma(-a[stri(l, j)], z[l], z[j]);
                v[j] = fma(-a[stri(l, j)], v[l], v[j]);
              }
            }
            // delta = u - (sum u / sum v) v: the step with the sum held; the trial never below 0.01 h (fraction to the boundary),
            // scaled onto the sum; a pivot that is no pivot, or a trial that is not finite: the EM successor
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) su = su + z[j], sv = sv + v[j];
            const double mult = su / sv;
            double sc = 0.0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const bool mj = ((mask >> j) & 1u) && h[j] > 0.0;
              z[j] = mj ? fmax(h[j] + fma(-mult, v[j], z[j]), 0.01 * h[j]) : 0.0;
              sc = sc + z[j];
            }
            sc = total / sc;
#pragma unroll
            for (int j = 0; j < K; ++j) {
              z[j] = z[j] * sc;
              bad |= !isfinite(z[j]);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) h[j] = (j == pin) ? h[j] : (bad ? st_e[(size_t)j * p] : z[j]);
            *st_acc = dev_t;
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
    passes[q] = np;
    done[q] = (uint8_t)st;
  }
  const uint32_t v[ESPM_PML_COUNTERS] = {live ? 1u : 0u, n_un, n_nf};
  block_count_add<ESPM_PML_COUNTERS, B / 64>(cnt_part, v, counters);
}

template <int K, typename XT>
int launch_simplex(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, uint32_t mask, int pin,
                   const double* t, double log_shift, double tol, int n_pass, double* h_io, double* dev, double* gap, double* slope,
                   int32_t* passes, uint8_t* done, double* state, unsigned long long* counters, hipStream_t st) {
  const dim3 grid((unsigned)(((int64_t)p + B - 1) / B)), block(B);
  const XT* xt = static_cast<const XT*>(x);
  Sums<K> sv;
  for (int j = 0; j < K; ++j) sv.v[j] = s[j];
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pixel_ml_simplex_kernel<K, XT, true>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, pin, t, log_shift, tol, n_pass,
                       h_io, dev, gap, slope, passes, done, state, counters);
  else
    hipLaunchKernelGGL((pixel_ml_simplex_kernel<K, XT, false>), grid, block, 0, st, xt, ld, n, p, d, sv, mask, pin, t, log_shift, tol, n_pass,
                       h_io, dev, gap, slope, passes, done, state, counters);
  return check_hip(hipGetLastError(), "pixel ML (simplex) launch");
}

// what espm_pixel_ml_simplex refuses before the device is touched: the pinned entry's refusals, with pin = -1 for "nothing pinned"
// (then the mask may not be empty, and t and slope may be null); k is checked by the caller: ESPM_EUNSUPPORTED
inline int check_simplex_args(const char* who, const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s,
                              int k, uint32_t mask, int pin, const double* t, double log_shift, double tol, int n_pass, const double* h_inout,
                              const double* dev, const double* gap, const double* slope, const int32_t* passes, const uint8_t* done,
                              const uint64_t* counters) {
  ESPM_REQUIRE(x && d && s && h_inout && dev && gap && passes && done && counters,
               "%s: bad arguments (x %p, d %p, s %p, h %p, dev %p, gap %p, passes %p, done %p, counters %p)", who, x, (const void*)d,
               (const void*)s, (const void*)h_inout, (const void*)dev, (const void*)gap, (const void*)passes, (const void*)done, (const void*)counters);
  ESPM_REQUIRE(pin >= -1 && pin < k, "%s: pin=%d (one of the %d components, or -1 for none)", who, pin, k);
  ESPM_REQUIRE(pin < 0 || (t && slope), "%s: bad arguments (t %p, slope %p with pin=%d)", who, (const void*)t, (const void*)slope, pin);
  if (int rc = check_image(who, x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "%s: log_shift=%g must be positive", who, log_shift);
  ESPM_REQUIRE(tol > 0, "%s: tol=%g must be positive", who, tol);
  ESPM_REQUIRE(n_pass >= 1, "%s: n_pass=%d (at least one pass)", who, n_pass);
  ESPM_REQUIRE((mask >> k) == 0, "%s: mask 0x%x over %d components (bits beyond them)", who, mask, k);
  ESPM_REQUIRE(pin >= 0 || mask != 0, "%s: an empty mask and nothing pinned (nothing to hold the sum)", who);
  if (pin >= 0) {
    ESPM_REQUIRE(!((mask >> pin) & 1u), "%s: pin=%d is in the mask 0x%x (the pinned component is not fitted)", who, pin, mask);
    ESPM_REQUIRE(s[pin] > 0 && std::isfinite(s[pin]), "%s: component %d is pinned and its spectrum sums to %g", who, pin, s[pin]);
  }
  for (int j = 0; j < k; ++j)
    if ((mask >> j) & 1u)
      ESPM_REQUIRE(s[j] > 0 && std::isfinite(s[j]), "%s: component %d is in the mask and its spectrum sums to %g", who, j, s[j]);
  return ESPM_OK;
}

}  // namespace pmlk
#endif

}  // namespace espm

using namespace espm;

extern "C" int espm_pixel_ml_simplex(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                                     uint32_t mask, int pin, const double* t, double log_shift, double tol, int n_pass, double* h_inout,
                                     double* dev, double* gap, double* slope, int32_t* passes, uint8_t* done, uint64_t* counters, void* state,
                                     size_t state_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel ML (simplex): built into the 1..%d component library only", ESPM_PML_MAX_K);
#else
  const char* who = "pixel ML (simplex)";
  if (k < 1 || k > ESPM_PML_MAX_K) return set_error(ESPM_EUNSUPPORTED, "%s: k=%d (1..%d components)", who, k, ESPM_PML_MAX_K);
  if (int rc = pmlk::check_simplex_args(who, x, x_dtype, x_layout, ld, n, p, d, s, k, mask, pin, t, log_shift, tol, n_pass, h_inout, dev, gap,
                                        slope, passes, done, counters))
    return rc;
  ESPM_REQUIRE(state && state_bytes >= ESPM_PMLN_STATE_BYTES(k, p), "%s: state %p of %zu bytes (%zu needed for k=%d, p=%d)", who, state,
               state_bytes, (size_t)ESPM_PMLN_STATE_BYTES(k, p), k, p);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (int rc = check_hip(hipMemsetAsync(cnt + ESPM_PML_NOT_DONE, 0, sizeof(unsigned long long), st), "pixel ML (simplex): zeroing the counter"))
    return rc;
  return dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return pmlk::launch_simplex<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, s, mask, pin, t, log_shift, tol,
                                                                                     n_pass, h_inout, dev, gap, slope, passes, done,
                                                                                     static_cast<double*>(state), cnt, st);
    });
  });
#endif
}
