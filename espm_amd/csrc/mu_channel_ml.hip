// The step of the channel ML (include/espm_mu.h, "channel ML step"): with the abundances H held and no dictionary, the spectra
// decouple per channel - channel c is ONE pixel problem whose observations are the p pixels of row c of X, whose design is H^T and
// whose column sums s_j = sum_p h_jp are the same for every channel.  The walk over the observations is espm_spectra_ml_pass_batch
// (mu_spectra_ml.hip: per channel dev, q (k) and the lower triangle of A); this unit is what the pixel kernels do BETWEEN two walks
// (mu_pixel_ml_newton.hip, mu_pixel_ml_pinned.hip), run for n_models x n problems in lockstep:
//
//   one thread per (model b, channel c): grid (channel blocks of ESPM_CDIAG_BLOCK, models), the exact K a template argument; h, q, the
//   triangle, r, z and the pivots in registers exactly as in the pixel kernels' between-walk code - nothing is indexed at run time
//   (the pinned component is a select inside an unrolled loop), so nothing goes to scratch (profiles/channel_ml_resources.txt)
//   the rule of model b is chosen by pin[b], uniform over the workgroup: -1 the free-scale rule (the Newton rule, whose scale onto
//   the ray is applied HERE, to the point the next pass evaluates), j >= 0 the pinned rule on component j
//   a problem with done != 0 is neither read nor written; a workgroup without a live problem returns at entry
//   each workgroup adds its problems still live to live[b] (integers, block_count_add, onto the counter the call zeroed); a second
//   launch of n_models threads sets active[b] = (live[b] != 0) - stream order is the only synchronisation there is
//
// No float atomics: two calls give the same bits, and a problem's bits do not depend on its neighbours or on the other models.
// Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry point as a stub.
#include <cmath>
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace cmlk {

constexpr int CB = ESPM_CDIAG_BLOCK;
constexpr int GROUP = 16;   // models per launch: their pins travel by value (2 k ends of k <= 8 components: one launch)
static_assert(CB % 64 == 0, "whole waves");

struct Pins {
  signed char v[GROUP];
};

template <int K>
struct Sums {   // s, by value: uniform over the launch
  double v[K];
};

__device__ __forceinline__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // (i, j), j <= i, of the lower triangle

template <int K>
__global__ __launch_bounds__(CB) void step_kernel(int n, int b0, Pins pins, Sums<K> s, uint32_t mask_all, int start, double tol,
                                                  const double* __restrict__ dev_in, const double* __restrict__ q_in,
                                                  const double* __restrict__ a_in, const double* __restrict__ xsum,
                                                  const double* __restrict__ t_in, double* __restrict__ d, double* __restrict__ state,
                                                  double* __restrict__ dev_o, double* __restrict__ gap_o, double* __restrict__ slope_o,
                                                  int32_t* __restrict__ passes, uint8_t* __restrict__ done,
                                                  unsigned long long* __restrict__ live_cnt) {
  constexpr int T = K * (K + 1) / 2;
  __shared__ uint32_t cnt_part[1][CB / 64];
  const size_t b = (size_t)b0 + blockIdx.y;
  const int pin = pins.v[blockIdx.y];
  const bool pinned = pin >= 0;
  const uint32_t mask = pinned ? (mask_all & ~(1u << pin)) : mask_all;   // M: the fitted set
  const int c = blockIdx.x * CB + threadIdx.x;
  const bool valid = c < n;
  const size_t i = b * (size_t)n + (valid ? c : 0);
  const bool entered = valid && done[i] == 0;   // the problems this call may write
  if (__syncthreads_count(entered) == 0) return;   // (workgroup-uniform: live[b] gets nothing from here)
  // the problem's rows of state (2 k + ESPM_CML_STATE_EXTRA, n) of its model: the accepted point, e, then dev_acc, tau, trial
  double* const st_pt = state + b * (size_t)(2 * K + ESPM_CML_STATE_EXTRA) * n + (valid ? c : 0);
  double* const st_e = st_pt + (size_t)K * n;
  double* const st_acc = st_pt + (size_t)(2 * K) * n;
  double* const st_tau = st_pt + (size_t)(2 * K + 1) * n;
  double* const st_trial = st_pt + (size_t)(2 * K + 2) * n;
  int st = 0;
  if (entered) {
    double h[K];
#pragma unroll
    for (int j = 0; j < K; ++j) h[j] = d[i * K + j];
    const double N = xsum[c];
    const int m = __popc(mask);
    bool rescale = false;   // the free rule: the next point goes onto the ray sum_M s_j h_j = N
    if (start) {
      // pass 0: the rule's own start fill; nothing of a pass is consumed and none is counted
      const double tq = pinned ? t_in[i] : 0.0;
      if (pinned && (!(tq >= 0.0) || !isfinite(tq))) {
        st = 2;   // no point of the profile: d stays as the caller left it
      } else if (!pinned && N == 0.0) {
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = 0.0;
        st = 1;
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (j == pin) h[j] = tq;
          else if (!((mask >> j) & 1u) || N == 0.0) h[j] = 0.0;
          else if (!(h[j] > 0.0)) h[j] = N / ((double)m * s.v[j]) * 1e-3;
        }
        rescale = !pinned;
      }
#pragma unroll
      for (int j = 0; j < K; ++j) st_e[(size_t)j * n] = 0.0;
      *st_acc = INFINITY, *st_tau = 1e-2, *st_trial = 0.0;
      dev_o[i] = 0.0, gap_o[i] = 0.0;
      if (pinned) slope_o[i] = 0.0;
      passes[i] = 0;
    } else {
      double qv[K], a[T];
#pragma unroll
      for (int j = 0; j < K; ++j) qv[j] = q_in[i * K + j];
#pragma unroll
      for (int l = 0; l < T; ++l) a[l] = a_in[i * T + l];
      // the ratios, the certificate and the slope
      double r[K];
      double rmax = -INFINITY, lin = 0.0, sl = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        r[j] = 0.0;
        if ((mask >> j) & 1u) {
          r[j] = qv[j] / s.v[j];
          rmax = fmax(rmax, r[j]);
          lin = fma(s.v[j] - qv[j], h[j], lin);
        }
        if (j == pin) sl = 2.0 * (s.v[j] - qv[j]);
      }
      const double dev_t = dev_in[i];
      const double gap_t = pinned ? 2.0 * fma(N, fmax(rmax - 1.0, 0.0), lin) : 2.0 * N * (rmax - 1.0);
      // the stop that is not finite; the trial rejected; or the point accepted, and then the stop or the next trial
      if (!isfinite(dev_t) || !isfinite(gap_t)) {
        dev_o[i] = dev_t, gap_o[i] = gap_t;
        if (pinned) slope_o[i] = sl;
        st = 2;
      } else {
        double tau = *st_tau;
        const bool trial = *st_trial != 0.0;
        if (trial && !(dev_t <= *st_acc)) {   // rejected: the EM successor of the accepted point, and a heavier blend
#pragma unroll
          for (int j = 0; j < K; ++j) h[j] = (j == pin) ? h[j] : st_e[(size_t)j * n];
          *st_trial = 0.0;
          *st_tau = fmin(10.0 * tau, 1.0);
          passes[i] += 1;
          rescale = !pinned;
        } else {
          dev_o[i] = dev_t, gap_o[i] = gap_t;
          if (pinned) slope_o[i] = sl;
#pragma unroll
          for (int j = 0; j < K; ++j) st_pt[(size_t)j * n] = h[j];
          if (gap_t <= tol) {
            st = 1;   // d keeps the certified point
          } else {
            if (trial) tau = fmax(tau / 10.0, 1e-8);
            // B = A_MM + tau diag(s / h) in place, the identity outside M (the pinned row too); the right-hand side -g = q - s
            double z[K];
#pragma unroll
            for (int u = 0; u < K; ++u) {
              const bool mu = (mask >> u) & 1u;
              r[u] = h[u] * r[u];   // e: the EM successor
              st_e[(size_t)u * n] = r[u];
              z[u] = mu ? -(s.v[u] - qv[u]) : 0.0;
#pragma unroll
              for (int j = 0; j < u; ++j)
                if (!(mu && ((mask >> j) & 1u))) a[tri(u, j)] = 0.0;
              a[tri(u, u)] = mu ? fma(tau, s.v[u] / h[u], a[tri(u, u)]) : 1.0;
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
              for (int u = j + 1; u < K; ++u) {
                double v = a[tri(u, j)];
#pragma unroll
                for (int l = 0; l < j; ++l) v = fma(-(a[tri(u, l)] * a[tri(j, l)]), dd[l], v);
                a[tri(u, j)] = v / dj;
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
            // the trial: never below 0.01 h (fraction to the boundary), never 0; a pivot that is no pivot: the EM step
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const double cand = fmax(fmax(h[j] + z[j], 0.01 * h[j]), 1e-30 * N / s.v[j]);
              h[j] = (j == pin) ? h[j] : (bad ? r[j] : (((mask >> j) & 1u) ? cand : 0.0));
            }
            *st_acc = dev_t;
            *st_tau = tau;
            *st_trial = bad ? 0.0 : 1.0;
            passes[i] += 1;
            rescale = !pinned;
          }
        }
      }
    }
    if (rescale) {   // the scale of least deviance on the ray, ahead of the pass that evaluates the point
      double S = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if ((mask >> j) & 1u) S = fma(s.v[j], h[j], S);
      if (!(S > 0.0) || !isfinite(S)) {
        st = 2;   // h as the step left it
      } else {
        const double f = N / S;
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = h[j] * f;
      }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) d[i * K + j] = h[j];
    if (start) {   // the accepted point of a problem that has not been evaluated yet: its start, as the first pass will see it
#pragma unroll
      for (int j = 0; j < K; ++j) st_pt[(size_t)j * n] = h[j];
    }
    done[i] = (uint8_t)st;
  }
  block_count_add<1, CB / 64>(cnt_part, {(entered && st == 0) ? 1u : 0u}, live_cnt + b);   // (every thread of the workgroup is here)
}

// active[b] = whether model b has a live problem left: what the next batched pass skips a model by
__global__ __launch_bounds__(256) void flags_kernel(int n_models, const unsigned long long* __restrict__ live_cnt,
                                                    uint8_t* __restrict__ active) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < n_models) active[b] = live_cnt[b] != 0 ? 1 : 0;
}

template <int K>
int launch(int n, int n_models, const int32_t* pin, const double* s, uint32_t mask, int start, double tol, const double* dev_in,
           const double* q, const double* a_tri, const double* xsum, const double* t, double* d, double* state, double* dev, double* gap,
           double* slope, int32_t* passes, uint8_t* done, unsigned long long* live, hipStream_t st) {
  Sums<K> sv;
  for (int j = 0; j < K; ++j) sv.v[j] = s[j];
  for (int b0 = 0; b0 < n_models; b0 += GROUP) {
    const int nb = n_models - b0 < GROUP ? n_models - b0 : GROUP;
    Pins pv = {};
    for (int b = 0; b < nb; ++b) pv.v[b] = (signed char)pin[b0 + b];
    const dim3 grid((unsigned)((n + CB - 1) / CB), (unsigned)nb), block(CB);
    hipLaunchKernelGGL((step_kernel<K>), grid, block, 0, st, n, b0, pv, sv, mask, start, tol, dev_in, q, a_tri, xsum, t, d, state, dev, gap,
                       slope, passes, done, live);
    if (int rc = check_hip(hipGetLastError(), "channel ML step launch")) return rc;
  }
  return ESPM_OK;
}

}  // namespace cmlk
#endif

}  // namespace espm

using namespace espm;

extern "C" int espm_channel_ml_step(int n, int k, int n_models, int start, const double* dev_in, const double* q, const double* a_tri,
                                    const double* xsum, const double* s, uint32_t mask, const int32_t* pin, const double* t, double tol,
                                    double* d, void* state, size_t state_bytes, double* dev, double* gap, double* slope, int32_t* passes,
                                    uint8_t* done, uint8_t* active, int64_t* live, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "channel ML step: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  const char* who = "channel ML step";
  if (k < 1 || k > ESPM_DIAG_MAX_K) return set_error(ESPM_EUNSUPPORTED, "%s: k=%d (1..%d components)", who, k, ESPM_DIAG_MAX_K);
  ESPM_REQUIRE(xsum && s && pin && d && state && dev && gap && passes && done && active && live,
               "%s: bad arguments (xsum %p, s %p, pin %p, d %p, state %p, dev %p, gap %p, passes %p, done %p, active %p, live %p)", who,
               (const void*)xsum, (const void*)s, (const void*)pin, (const void*)d, state, (const void*)dev, (const void*)gap,
               (const void*)passes, (const void*)done, (const void*)active, (const void*)live);
  ESPM_REQUIRE(start || (dev_in && q && a_tri), "%s: bad arguments (the sums of a pass: dev %p, q %p, a_tri %p)", who, (const void*)dev_in,
               (const void*)q, (const void*)a_tri);
  ESPM_REQUIRE(n >= 1 && (n + ESPM_CDIAG_BLOCK - 1) / ESPM_CDIAG_BLOCK <= 65535, "%s: n=%d (1..%d channels)", who, n,
               65535 * ESPM_CDIAG_BLOCK);
  ESPM_REQUIRE(n_models >= 1 && n_models <= ESPM_SML_MAX_MODELS, "%s: n_models=%d (1..%d)", who, n_models, ESPM_SML_MAX_MODELS);
  ESPM_REQUIRE(tol > 0, "%s: tol=%g must be positive", who, tol);
  ESPM_REQUIRE(mask != 0 && (mask >> k) == 0, "%s: mask 0x%x over %d components (empty, or bits beyond them)", who, mask, k);
  for (int j = 0; j < k; ++j)
    if ((mask >> j) & 1u)
      ESPM_REQUIRE(s[j] > 0 && std::isfinite(s[j]), "%s: component %d is in the mask and its column of H^T sums to %g", who, j, s[j]);
  bool any_pinned = false;
  for (int b = 0; b < n_models; ++b) {
    ESPM_REQUIRE(pin[b] == -1 || (pin[b] >= 0 && pin[b] < k && ((mask >> pin[b]) & 1u)),
                 "%s: pin[%d]=%d (-1, or a component of the mask 0x%x)", who, b, pin[b], mask);
    any_pinned |= pin[b] >= 0;
  }
  ESPM_REQUIRE(!any_pinned || (t && slope), "%s: bad arguments (a pinned model needs t %p and slope %p)", who, (const void*)t,
               (const void*)slope);
  ESPM_REQUIRE(state_bytes >= ESPM_CML_STATE_BYTES(k, n, n_models), "%s: state of %zu bytes (%zu needed for k=%d, n=%d, n_models=%d)", who,
               state_bytes, (size_t)ESPM_CML_STATE_BYTES(k, n, n_models), k, n, n_models);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(live);
  if (int rc = check_hip(hipMemsetAsync(cnt, 0, (size_t)n_models * sizeof(unsigned long long), st), "channel ML step: zeroing the live counts"))
    return rc;
  if (int rc = dispatch_k_exact(k, [&](auto kk) {
        return cmlk::launch<decltype(kk)::value>(n, n_models, pin, s, mask, start, tol, dev_in, q, a_tri, xsum, t, d,
                                                 static_cast<double*>(state), dev, gap, slope, passes, done, cnt, st);
      }))
    return rc;
  hipLaunchKernelGGL(cmlk::flags_kernel, dim3((unsigned)((n_models + 255) / 256)), dim3(256), 0, st, n_models, cnt, active);
  return check_hip(hipGetLastError(), "channel ML step: the flags");
#endif
}
