// fp64 mode on the sparse count store (include/espm_mu.h, "fp64 mode, sparse store"): the H pass and the W accumulation of
// mu_fp64.hip walking the non-zero elements of a count image instead of all n x p entries.  Everything downstream of them
// (bisection, W finish, rel, G W, statistics of H) is mu_fp64.hip's, unchanged.
//
//   H pass   one lane per pixel; the lists of 64 consecutive pixels are interleaved dword-wise, so a wave's load of "element r
//            of every list" is one coalesced row.  G W is read by channel index at random: it sits in LDS row-major (n, K) where
//            n K doubles fit ESPM_F64S_LDS_BYTES (a b64 read goes out in two halves of 32 lanes over 64 banks; with random rows
//            no layout is conflict free, row-major lets the K reads of an element merge into wide ones), and is read through L2
//            otherwise.  After the lists, one loop over ALL channels that reads no X: sum(log Y) of the pixel with an fp32 log
//            (it enters the loss times log_shift), and the empty channels' log_shift terms with an fp32 reciprocal.  An empty
//            pixel is a column of log_shift: its lane does that loop with an fp64 division (its whole update is that term).
//   W pass   one workgroup per (block of ESPM_F64S_WBLOCK pixels, channel), its threads stride over the list (plain CSR: the
//            loads coalesce), gather max(H, eps) of each element's pixel, and the workgroup's K sums are one fixed tree.  An
//            empty channel is a row of log_shift over every pixel, in fp64: it is the whole of that channel's rh.
//
// Reductions are fixed trees (lists ascending, wave shuffles, waves in order, workgroups in order); no float atomics.
#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
namespace f64s {

constexpr int B = ESPM_F64_BLOCK;      // threads of a W-pass workgroup
constexpr int HB = ESPM_F64S_HBLOCK;   // threads (= pixels) of an H-pass workgroup
constexpr int WBLK = ESPM_F64S_WBLOCK;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
  return v;   // lane 0
}

// NV sums per thread -> workgroup totals in thread 0 (the waves added in order).  sh: (T / WAVE) * NV doubles of LDS.
template <int NV, int T>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double r = wave_sum(v[i]);
    if (lane == 0) sh[wv * NV + i] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      double t = sh[i];
      for (int w = 1; w < T / WAVE; ++w) t += sh[w * NV + i];
      v[i] = t;
    }
  }
}

// out[i] = sum over b < nblk of part[b * nv + i], in a fixed order.  One workgroup.
__global__ __launch_bounds__(B) void parts_kernel(const double* __restrict__ part, int nblk, int nv, double* __restrict__ out) {
  __shared__ double sh[B / WAVE];
  for (int i = 0; i < nv; ++i) {
    double t = 0;
    for (int b = threadIdx.x; b < nblk; b += B) t += part[(size_t)b * nv + i];
    double v[1] = {t};
    __syncthreads();
    block_sum<1, B>(v, sh);
    if (threadIdx.x == 0) out[i] = v[0];
  }
}

// ---- the H pass ----------------------------------------------------------------------------------------------------------------
template <int K, bool LDS>
__global__ __launch_bounds__(HB) void h_pass_kernel(const uint32_t* __restrict__ elem, const int64_t* __restrict__ off,
                                                    const int32_t* __restrict__ ec, int n_ec, const uint8_t* __restrict__ ep_flag, int n,
                                                    int p, double xscale, const double* __restrict__ gw,
                                                    const double* __restrict__ colsum_gw, const int32_t* __restrict__ gw_small,
                                                    const double* __restrict__ h, const double* __restrict__ hstat,
                                                    const double* __restrict__ mu, double eps_reg, double lambda_L, double sigma, int nx,
                                                    int ny, double eps, int mode, const double* __restrict__ fixed_h,
                                                    double* __restrict__ h_out, double* __restrict__ num_out, double* __restrict__ den_out,
                                                    double* __restrict__ part) {
  extern __shared__ double gws[];   // LDS: (n, K) G W; afterwards the reduction's (HB / WAVE) * 3 doubles
  const int q = blockIdx.x * HB + threadIdx.x;
  const bool valid = q < p;
  const bool small = *gw_small != 0;
  if (LDS) {
    for (int i = threadIdx.x; i < n * K; i += HB) gws[i] = gw[i];
    __syncthreads();
  }
  double hr[K], hc[K], acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    hr[j] = valid ? h[(size_t)j * p + q] : 1.0;
    hc[j] = fmax(hr[j], eps);
    acc[j] = 0;
  }
  // ---- the non-zero elements of the pixel: element r of the 64 lists of this wave's group is one row of 64 dwords
  double xlog = 0, lognz = 0;   // sum max(x, eps) log y and sum log y over them
  {
    const int grp = q >> 6, lane = threadIdx.x & (WAVE - 1);   // (HB is a multiple of 64: a wave is one group)
    const int ngrp = (p + WAVE - 1) >> 6;
    if (grp < ngrp) {
      const int64_t o0 = off[grp];
      const int rows = (int)((off[grp + 1] - o0) >> 6);
      const uint32_t* e = elem + o0 + lane;
      for (int r = 0; r < rows; ++r) {
        const uint32_t d = e[(size_t)r * WAVE];
        if (d == 0) continue;   // (padding up to the group's longest list)
        const int c = (int)(d & 0xffffu);
        const double xv = (double)(d >> 16) * xscale;
        const double* g = (LDS ? gws : gw) + (size_t)c * K;
        double gr[K];
#pragma unroll
        for (int j = 0; j < K; ++j) gr[j] = g[j];
        double y = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) y = fma(gr[j], hc[j], y);
        if (mode) {
          const double rr = xv / (y != 0 ? y : eps);   // (updates.py:129-131)
#pragma unroll
          for (int j = 0; j < K; ++j) acc[j] = fma(gr[j], rr, acc[j]);
        }
        double yl = y;   // the loss clamps G W (measures.py:493-504)
        if (small) {
          yl = 0;
#pragma unroll
          for (int j = 0; j < K; ++j) yl = fma(fmax(gr[j], eps), hc[j], yl);
        }
        const double l = log(yl);
        xlog = fma(fmax(xv, eps), l, xlog);
        lognz += l;
      }
    }
  }
  // ---- the log_shift terms (header: "zeros that are not zeros")
  const bool ep = valid && ep_flag && ep_flag[q] != 0;
  const double fill = eps * xscale;   // the effective value of a filled entry
  double logall = 0, logec = 0, fa[K];
#pragma unroll
  for (int j = 0; j < K; ++j) fa[j] = 0;
  if (valid) {
    // every channel, no X: sum log Y (fp32 log of the fp64 y, fp64 sum); G W at a uniform address, from global memory
    for (int c = 0; c < n; ++c) {
      const double* g = gw + (size_t)c * K;
      double y = 0, yl = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) y = fma(g[j], hc[j], y);
      yl = y;
      if (small) {
        yl = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) yl = fma(fmax(g[j], eps), hc[j], yl);
      }
      logall += (double)logf((float)yl);
      if (ep && mode) {   // an empty pixel: every channel holds log_shift, and that is all of its numerator: fp64
        const double rr = 1.0 / (y != 0 ? y : eps);
#pragma unroll
        for (int j = 0; j < K; ++j) fa[j] = fma(g[j], rr, fa[j]);
      }
    }
    if (!ep) {
      for (int i = 0; i < n_ec; ++i) {   // the empty channels: rows of log_shift
        const double* g = gw + (size_t)ec[i] * K;
        double y = 0, yl = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) y = fma(g[j], hc[j], y);
        yl = y;
        if (small) {
          yl = 0;
#pragma unroll
          for (int j = 0; j < K; ++j) yl = fma(fmax(g[j], eps), hc[j], yl);
        }
        logec += (double)logf((float)yl);
        if (mode) {
          const double rr = (double)(1.0f / (float)(y != 0 ? y : eps));
#pragma unroll
          for (int j = 0; j < K; ++j) fa[j] = fma(g[j], rr, fa[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = fma(fill, fa[j], acc[j]);
  double kl = 0;
  if (valid) {
    // sum(Y) - sum max(X, eps) log Y: a zero of a kept line weighs eps, a filled entry max(fill, eps)
    double sy = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) sy = fma(colsum_gw[j], hc[j], sy);   // (colsum_gw: of max(G W, eps) when gw_small, see the entry point)
    const double fv = fmax(fill, eps);
    kl = ep ? sy - fv * logall : sy - xlog - eps * (logall - lognz - logec) - fv * logec;
  }
  double reg = 0, lap = 0;
  if (valid) {
    double hl[K];
    if (nx > 0) {   // (H L)[j, q]: 5-point stencil, zero-flux boundary (utils.py:39-76)
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
        // updates.py:127-141, in the reference's order of operations (as mu_fp64.hip's epilogue)
        double num = acc[j];
        double den = colsum_gw[K + j] + mu[j] / (hc[j] + eps_reg);
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
  __syncthreads();   // (the G W image in LDS is no longer read)
  block_sum<3, HB>(v, gws);
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 3; ++i) part[(size_t)blockIdx.x * 3 + i] = v[i];
}

// cs (2K): [0, K) the column sums the loss uses (of max(G W, eps) when *gw_small), [K, 2K) colsum(G W) for the update.  One workgroup.
template <int K>
__global__ __launch_bounds__(B) void colsums_kernel(const double* __restrict__ gw, int n, const double* __restrict__ colsum_gw,
                                                    const int32_t* __restrict__ gw_small, double eps, double* __restrict__ cs) {
  __shared__ double sh[(B / WAVE) * K];
  const bool small = *gw_small != 0;
  double v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = 0;
  if (small)
    for (int c = threadIdx.x; c < n; c += B)
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] += fmax(gw[(size_t)c * K + j], eps);
  block_sum<K, B>(v, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      cs[j] = small ? v[j] : colsum_gw[j];
      cs[K + j] = colsum_gw[j];
    }
}

// ---- the W pass ----------------------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(B) void w_accum_kernel(const uint32_t* __restrict__ elem, const int64_t* __restrict__ off,
                                                    const uint8_t* __restrict__ ec_flag, const int32_t* __restrict__ ep,
                                                    const int32_t* __restrict__ ep_off, int n, int p, double xscale,
                                                    const double* __restrict__ gw, const double* __restrict__ h, double eps,
                                                    double* __restrict__ part) {
  __shared__ double sh[(B / WAVE) * K];
  const int c = blockIdx.x, blk = blockIdx.y;
  const int q0 = blk * WBLK, q1 = min(p, q0 + WBLK);
  double g[K], acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    g[j] = gw[(size_t)c * K + j];
    acc[j] = 0;
  }
  auto add = [&](int q, double xv) {
    double hc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) hc[j] = fmax(h[(size_t)j * p + q], eps);
    double y = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) y = fma(g[j], hc[j], y);
    const double r = xv / (y != 0 ? y : eps);   // (updates.py:54-56)
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = fma(r, hc[j], acc[j]);
  };
  const double fill = eps * xscale;
  if (ec_flag && ec_flag[c]) {
    for (int q = q0 + threadIdx.x; q < q1; q += B) add(q, fill);   // an empty channel: a row of log_shift
  } else {
    const size_t l = (size_t)blk * n + c;
    const int64_t e0 = off[l], e1 = off[l + 1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += B) {
      const uint32_t d = elem[e];
      add(q0 + (int)(d & 0xffffu), (double)(d >> 16) * xscale);
    }
    if (ep_off)   // the empty pixels of the block: columns of log_shift
      for (int i = ep_off[blk] + threadIdx.x; i < ep_off[blk + 1]; i += B) add(ep[i], fill);
  }
  block_sum<K, B>(acc, sh);
  if (threadIdx.x == 0)
#pragma unroll
    for (int j = 0; j < K; ++j) part[((size_t)blk * n + c) * K + j] = acc[j];
}

__global__ __launch_bounds__(B) void w_parts_kernel(const double* __restrict__ part, int nblk, int64_t nk, double* __restrict__ rh) {
  const int64_t e = (int64_t)blockIdx.x * B + threadIdx.x;
  if (e >= nk) return;
  double t = 0;
  for (int b = 0; b < nblk; ++b) t += part[(size_t)b * nk + e];
  rh[e] = t;
}

inline int nblk_of(int64_t count, int64_t per) { return (int)((count + per - 1) / per); }

template <int K, bool LDS>
int launch_h_pass(const uint32_t* elem, const int64_t* off, const int32_t* ec, int n_ec, const uint8_t* ep_flag, int n, int p, double xscale,
                  const double* gw, const double* cs, const int32_t* gw_small, const double* h, const double* hstat, const double* mu,
                  double eps_reg, double lambda_L, double sigma, int nx, int ny, double eps, int mode, const double* fixed_h, double* h_out,
                  double* num, double* den, double* part, hipStream_t s) {
  const size_t red = (size_t)(HB / WAVE) * 3 * sizeof(double);
  size_t lds = LDS ? (size_t)n * K * sizeof(double) : 0;
  lds = lds > red ? lds : red;
  auto kern = h_pass_kernel<K, LDS>;
  static bool attr = false;   // (the attribute once per instantiation)
  if (LDS && !attr) {
    if (int rc = check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               ESPM_F64S_LDS_BYTES), "fp64 sparse H pass LDS"))
      return rc;
    attr = true;
  }
  hipLaunchKernelGGL(kern, dim3(nblk_of(p, HB)), dim3(HB), lds, s, elem, off, ec, n_ec, ep_flag, n, p, xscale, gw, cs, gw_small, h, hstat, mu,
                     eps_reg, lambda_L, sigma, nx, ny, eps, mode, fixed_h, h_out, num, den, part);
  return check_hip(hipGetLastError(), "fp64 sparse H pass launch");
}

}  // namespace f64s
#endif

}  // namespace espm

using namespace espm;

#define F64S_REQUIRE_BUILD()                                                                                                          \
  do {                                                                                                                                \
    if (ESPM_KP != 8) return set_error(ESPM_EUNSUPPORTED, "fp64 mode: built into the 1..%d component library only", ESPM_F64_MAX_K); \
  } while (0)

#define F64S_K_SWITCH(k, ...)          \
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

int64_t espm_f64_sparse_scratch_doubles(int n, int p, int k) {
  const int64_t hb = (p + ESPM_F64S_HBLOCK - 1) / ESPM_F64S_HBLOCK;
  const int64_t wb = (p + ESPM_F64S_WBLOCK - 1) / ESPM_F64S_WBLOCK;
  const int64_t hneed = hb * 3 + 2 * k, wneed = wb * n * k;
  return hneed > wneed ? hneed : wneed;
}

int espm_f64_sparse_h_pass(const uint32_t* h_elem, const int64_t* h_off, const int32_t* ec, int n_ec, const uint8_t* ep_flag, int n, int p,
                           double xscale, const double* gw, const double* colsum_gw, const int32_t* gw_small, const double* h, int k,
                           const double* hstat, const double* mu, double eps_reg, double lambda_L, double sigma, int nx, int ny,
                           double log_shift, int mode, const double* fixed_h, double* h_out, double* num, double* den, double* scratch,
                           double* hist_row, espm_stream_t stream) {
  F64S_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(h_elem && h_off && gw && colsum_gw && gw_small && h && mu && scratch && hist_row && n >= 1 && p >= 1,
               "fp64 sparse H pass: bad arguments");
  ESPM_REQUIRE(n <= ESPM_F64S_MAX_N && n_ec >= 0 && n_ec <= n && (n_ec == 0 || ec), "fp64 sparse H pass: n=%d channels, %d empty", n, n_ec);
  ESPM_REQUIRE(mode >= 0 && mode <= 2 && (mode != 1 || h_out) && (mode != 2 || (num && den)), "fp64 sparse H pass: mode %d without its outputs", mode);
  ESPM_REQUIRE(lambda_L == 0 || hstat, "fp64 sparse H pass: lambda_L without the statistics of H");
  ESPM_REQUIRE(nx == 0 || (nx >= 1 && ny >= 1 && (int64_t)nx * ny == p), "fp64 sparse H pass: grid %d x %d does not match p=%d", nx, ny, p);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = f64s::nblk_of(p, f64s::HB);
  double* cs = scratch + (size_t)nb * 3;   // 2k column sums behind the partials
  int rc = ESPM_OK;
  F64S_K_SWITCH(k, {
    hipLaunchKernelGGL(f64s::colsums_kernel<K>, dim3(1), dim3(f64s::B), 0, s, gw, n, colsum_gw, gw_small, log_shift, cs);
    if ((rc = check_hip(hipGetLastError(), "fp64 sparse column sums launch"))) return rc;
    if ((size_t)n * K * sizeof(double) <= (size_t)ESPM_F64S_LDS_BYTES)
      rc = f64s::launch_h_pass<K, true>(h_elem, h_off, ec, n_ec, ep_flag, n, p, xscale, gw, cs, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma,
                                        nx, ny, log_shift, mode, fixed_h, h_out, num, den, scratch, s);
    else
      rc = f64s::launch_h_pass<K, false>(h_elem, h_off, ec, n_ec, ep_flag, n, p, xscale, gw, cs, gw_small, h, hstat, mu, eps_reg, lambda_L, sigma,
                                         nx, ny, log_shift, mode, fixed_h, h_out, num, den, scratch, s);
    break;
  })
  if (rc) return rc;
  hipLaunchKernelGGL(f64s::parts_kernel, dim3(1), dim3(f64s::B), 0, s, scratch, nb, 3, hist_row);
  return check_hip(hipGetLastError(), "fp64 sparse loss reduction launch");
#endif
  return ESPM_OK;
}

int espm_f64_sparse_w_accum(const uint32_t* w_elem, const int64_t* w_off, const uint8_t* ec_flag, const int32_t* ep, const int32_t* ep_off,
                            int n, int p, double xscale, const double* gw, const double* h, int k, double log_shift, double* scratch,
                            double* rh, espm_stream_t stream) {
  F64S_REQUIRE_BUILD();
#if ESPM_KP == 8
  ESPM_REQUIRE(w_elem && w_off && gw && h && scratch && rh && n >= 1 && p >= 1 && (ep_off == nullptr || ep), "fp64 sparse W pass: bad arguments");
  ESPM_REQUIRE(n <= ESPM_F64S_MAX_N, "fp64 sparse W pass: n=%d channels", n);
  const int nblk = f64s::nblk_of(p, f64s::WBLK);
  ESPM_REQUIRE(nblk <= 65535, "fp64 sparse W pass: p=%d pixels", p);
  hipStream_t s = static_cast<hipStream_t>(stream);
  F64S_K_SWITCH(k, {
    hipLaunchKernelGGL(f64s::w_accum_kernel<K>, dim3(n, nblk), dim3(f64s::B), 0, s, w_elem, w_off, ec_flag, ep, ep_off, n, p, xscale, gw, h,
                       log_shift, scratch);
    if (int rc = check_hip(hipGetLastError(), "fp64 sparse W pass launch")) return rc;
    const int64_t nk = (int64_t)n * K;
    hipLaunchKernelGGL(f64s::w_parts_kernel, dim3(f64s::nblk_of(nk, f64s::B)), dim3(f64s::B), 0, s, scratch, nblk, nk, rh);
    return check_hip(hipGetLastError(), "fp64 sparse W pass reduction launch");
  })
#endif
  return ESPM_OK;
}

}  // extern "C"
