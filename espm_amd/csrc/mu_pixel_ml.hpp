// What the two pixel ML units share (mu_pixel_ml.hip: the EM rule; mu_pixel_ml_newton.hip: the Newton rule): the geometry, the walk
// over the channels of a workgroup's pixels, and what both entry points ask of their arguments before the device is touched.
//
// Included INSIDE namespace espm, behind the unit's `#if ESPM_KP == 8`, after mu_common.hpp, <cmath>, <type_traits> and
// mu_image_pass.hpp.
#pragma once

namespace pmlk {

constexpr int B = ESPM_DIAG_BLOCK;
constexpr int CH = ESPM_DIAG_CHUNK;
constexpr int TP = B + 1;   // pixel stride of the pixel-major tile
static_assert(B % 64 == 0 && ESPM_PML_COUNTERS <= B, "whole waves; a thread per counter");

template <int K>
struct Sums {   // s, by value: uniform over the launch
  double v[K];
};

// The channels of the workgroup's pixels, ascending: f(x, row of D in LDS) for every entry of an `active` thread.  WITH_D: the rows of
// D are staged (and `restage` says whether ds still holds the one chunk there is); every thread of the workgroup comes here.  UNROLL:
// the entries of a channel-major thread in flight (the Newton rule's K = 7, 8 trade them for a second wave per SIMD).
template <int K, typename XT, bool PM, bool WITH_D, int UNROLL = 4, typename F>
__device__ __forceinline__ void walk(const XT* __restrict__ x, int64_t ld, int n, int p, int q0, const double* __restrict__ d, double* ds,
                                     XT* tile, bool restage, bool active, F f) {
  const int q = q0 + threadIdx.x;
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int cn = min(CH, n - c0);
    if (WITH_D && restage) {   // (workgroup-uniform)
      __syncthreads();   // (the readers of the round before)
      for (int i = threadIdx.x; i < cn * K; i += B) ds[i] = d[(size_t)c0 * K + i];
      __syncthreads();
    }
    if constexpr (!PM) {
      if (active) {
        const XT* xp = x + (size_t)c0 * ld + q;
#pragma unroll UNROLL
        for (int c = 0; c < cn; ++c) f((double)xp[(size_t)c * ld], ds + c * K);
      }
    } else {
      constexpr int TS = tile_rows<XT>();
      for (int t0 = 0; t0 < cn; t0 += TS) {
        const int tn = min(TS, cn - t0);
        __syncthreads();   // (the tile's readers of the round before)
        fill_tile<XT, B>(tile, x, ld, q0, p, c0 + t0, tn);
        __syncthreads();
        if (active)
          for (int c = 0; c < tn; ++c) f((double)tile[c * TP + threadIdx.x], ds + (t0 + c) * K);
      }
    }
  }
}

// what espm_pixel_ml and espm_pixel_ml_newton refuse before the device is touched (k is checked by the caller: ESPM_EUNSUPPORTED)
inline int check_args(const char* who, const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                      uint32_t mask, double log_shift, double tol, int n_pass, const double* h_inout, const double* dev, const double* gap,
                      const int32_t* passes, const uint8_t* done, const uint64_t* counters) {
  ESPM_REQUIRE(x && d && s && h_inout && dev && gap && passes && done && counters,
               "%s: bad arguments (x %p, d %p, s %p, h %p, dev %p, gap %p, passes %p, done %p, counters %p)", who, x, (const void*)d,
               (const void*)s, (const void*)h_inout, (const void*)dev, (const void*)gap, (const void*)passes, (const void*)done, (const void*)counters);
  if (int rc = check_image(who, x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "%s: log_shift=%g must be positive", who, log_shift);
  ESPM_REQUIRE(tol > 0, "%s: tol=%g must be positive", who, tol);
  ESPM_REQUIRE(n_pass >= 1, "%s: n_pass=%d (at least one pass)", who, n_pass);
  ESPM_REQUIRE(mask != 0 && (mask >> k) == 0,"%s: mask 0x%x over %d components (empty, or bits beyond them)", who, mask, k);
  for (int j = 0; j < k; ++j)
    if ((mask >> j) & 1u)
      ESPM_REQUIRE(s[j] > 0 && std::isfinite(s[j]), "%s: component %d is in the mask and its spectrum sums to %g", who, j, s[j]);
  return ESPM_OK;
}

}  // namespace pmlk
