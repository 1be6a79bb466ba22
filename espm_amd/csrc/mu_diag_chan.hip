// Per-channel diagnostics of a fitted model (include/espm_mu.h, "channel diagnostics"): the transpose-side sibling of mu_diag.hip.  One
// fp64 pass over X that reduces over PIXELS: per channel c, with y = max(d h, log_shift), the Poisson deviance, sum_p x, sum_p y and
// the lower triangle of M_c = sum_p h_p h_p^T / y_cp, the expected Fisher information of row c of D = G W with the abundances held.
//
//   one channel per thread, ESPM_CDIAG_BLOCK channels per workgroup, ESPM_CDIAG_PCHUNK pixels per workgroup: grid (pixel chunks,
//                channel blocks) - 2048 channels x 512^2 pixels are 128 x 8 = 1024 workgroups
//   the row of d (k), the three sums and the k (k + 1) / 2 entries of M stay in registers; the chunk's columns of h go through LDS a
//                tile of pixels at a time and are read back as broadcasts (every lane of a wave reads the same address)
//   per entry: y (k FMAs), one division, one log where x > 0, k products h_i / y and k (k + 1) / 2 FMAs
//   pixel-major X ((p, n), hyperspy's layout) is read directly: the lanes of a wave read consecutive channels of one pixel's row,
//                eight rows in flight per thread; channel-major X goes through an LDS tile (channels, pixel tile) that is filled with
//                loads running along the pixels and read back transposed, one row per lane, rows an odd number of dwords apart -
//                both layouts run the same accumulation in the same order and give the same bits
//   each workgroup writes its 3 + k (k + 1) / 2 partial sums per channel to scratch[chunk][sum][channel]; a second launch adds the
//                chunks in ascending order.  No float atomics: two calls give the same bits.
//
// Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry points as stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"   // (the host side only: this tile has a geometry of its own)

namespace cdiagk {

constexpr int CB = ESPM_CDIAG_BLOCK;
constexpr int PC = ESPM_CDIAG_PCHUNK;

// pixels per tile: the columns of h staged per round and, for channel-major X, the width of the transposing tile; the tile's rows
// are TP elements apart, an odd number of dwords (u8: 17, u16: 33, f32: 33; f64: 34, whose 8-byte reads pair the banks), 17-35 KB
template <typename XT>
struct Tile {
  static constexpr int P = sizeof(XT) <= 2 ? 64 : sizeof(XT) == 4 ? 32 : 16;
  static constexpr int TP = P + (sizeof(XT) == 1 ? 4 : sizeof(XT) == 2 ? 2 : 1);
};
constexpr int PM_TILE = 64;   // pixel-major X has no tile of its own: 64 columns of h per round

__host__ __device__ constexpr int n_tri(int k) { return k * (k + 1) / 2; }
__host__ __device__ constexpr int n_acc(int k) { return 3 + n_tri(k); }   // dev, sum x, sum y, the triangle

template <int K>
struct Acc {
  double d[K];
  double m[K * (K + 1) / 2];
  double dev, xs, ys;
  double floor_y;

  // one entry of X; hs: the tile's columns of h, component j of pixel q at hs[j * PT + q] (the same address in every lane)
  template <int PT>
  __device__ __forceinline__ void add(double xv, const double* __restrict__ hs, int q) {
    double hj[K];
    double y = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      hj[j] = hs[j * PT + q];
      y = fma(d[j], hj[j], y);
    }
    y = fmax(y, floor_y);
    const double w = 1.0 / y;
    double t = y - xv;
    if (xv > 0) t = fma(xv, log(xv * w), t);
    dev += t;
    xs += xv;
    ys += y;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double hw = hj[i] * w;
#pragma unroll
      for (int j = 0; j <= i; ++j) m[i * (i + 1) / 2 + j] = fma(hw, hj[j], m[i * (i + 1) / 2 + j]);
    }
  }
};

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(CB) void channel_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                     const double* __restrict__ h, double log_shift, double* __restrict__ part) {
  constexpr int PT = PM ? PM_TILE : Tile<XT>::P;
  constexpr int NA = n_acc(K);
  __shared__ double hs[K * PT];
  const int c0 = blockIdx.y * CB;
  const int c = c0 + threadIdx.x;
  const bool valid = c < n;
  const int q0 = blockIdx.x * PC;           // (p < 2^31: the entry point's int)
  const int qn = min(PC, p - q0);
  Acc<K> a;
#pragma unroll
  for (int j = 0; j < K; ++j) a.d[j] = valid ? d[(size_t)c * K + j] : 0.0;
#pragma unroll
  for (int i = 0; i < K * (K + 1) / 2; ++i) a.m[i] = 0;
  a.dev = a.xs = a.ys = 0;
  a.floor_y = log_shift;

  for (int t0 = 0; t0 < qn; t0 += PT) {
    const int tn = min(PT, qn - t0);
    __syncthreads();   // (the readers of the round before)
    for (int i = threadIdx.x; i < K * PT; i += CB) {
      const int j = i / PT, q = i % PT;
      hs[i] = q < tn ? h[(size_t)j * p + (q0 + t0 + q)] : 0.0;
    }
    if constexpr (PM) {
      __syncthreads();
      const XT* xp = x + (size_t)(q0 + t0) * ld + c;
      for (int q = 0; q < tn; q += 8) {
        XT xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = (valid && q + u < tn) ? xp[(size_t)(q + u) * ld] : XT(0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (q + u < tn) a.template add<PT>((double)xv[u], hs, q + u);
      }
    } else {
      constexpr int TP = Tile<XT>::TP;
      __shared__ XT tile[CB * TP];
      // element e of the tile: channel e / PT, pixel e % PT - consecutive lanes read consecutive pixels of one channel's row
#pragma unroll 8
      for (int i = 0; i < PT; ++i) {
        const int e = i * CB + threadIdx.x;
        const int cc = e / PT, q = e % PT;
        XT v = XT(0);
        if (c0 + cc < n && q < tn) v = x[(size_t)(c0 + cc) * ld + (q0 + t0 + q)];
        tile[cc * TP + q] = v;
      }
      __syncthreads();
      const XT* row = tile + threadIdx.x * TP;
#pragma unroll 2   // (4 cost 35 more registers at k = 5 and a wave per SIMD)
      for (int q = 0; q < tn; ++q) a.template add<PT>((double)row[q], hs, q);
    }
  }

  if (valid) {   // scratch[chunk][sum][channel]: coalesced here and in the reduction
    double* out = part + (size_t)blockIdx.x * NA * n + c;
    out[0] = a.dev;
    out[(size_t)n] = a.xs;
    out[(size_t)2 * n] = a.ys;
#pragma unroll
    for (int i = 0; i < K * (K + 1) / 2; ++i) out[(size_t)(3 + i) * n] = a.m[i];
  }
}

// the chunks of every (sum, channel) added in ascending order: the one order there is, whatever the grid did
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int n, int na, int n_chunks, double* __restrict__ dev,
                                                     double* __restrict__ xsum, double* __restrict__ ysum, double* __restrict__ m_tri) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)na * n) return;
  const int s = (int)(i / n), c = (int)(i % n);
  double v = 0;
  for (int q = 0; q < n_chunks; ++q) v += part[((size_t)q * na + s) * n + c];
  if (s == 0) dev[c] = 2.0 * v;
  else if (s == 1) xsum[c] = v;
  else if (s == 2) ysum[c] = v;
  else m_tri[(size_t)c * (na - 3) + (s - 3)] = v;
}

template <int K, typename XT>
int launch(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, double log_shift, double* part,
           hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + PC - 1) / PC), (unsigned)((n + CB - 1) / CB)), block(CB);
  const XT* xt = static_cast<const XT*>(x);
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((channel_kernel<K, XT, true>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, part);
  else
    hipLaunchKernelGGL((channel_kernel<K, XT, false>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, part);
  return check_hip(hipGetLastError(), "channel diagnostics launch");
}

}  // namespace cdiagk
#endif

}  // namespace espm

using namespace espm;

extern "C" size_t espm_channel_diagnostics_scratch(int n, int p, int k) {
#if ESPM_KP != 8
  (void)n; (void)p; (void)k;
  return 0;
#else
  if (n < 1 || p < 1 || k < 1 || k > ESPM_DIAG_MAX_K) return 0;
  const size_t chunks = (size_t)(((int64_t)p + ESPM_CDIAG_PCHUNK - 1) / ESPM_CDIAG_PCHUNK);
  return chunks * (size_t)cdiagk::n_acc(k) * (size_t)n * sizeof(double);
#endif
}

extern "C" int espm_channel_diagnostics(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d,
                                        const double* h, int k, double log_shift, double* dev, double* xsum, double* ysum, double* m_tri,
                                        void* scratch, size_t scratch_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "channel diagnostics: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (k < 1 || k > ESPM_DIAG_MAX_K) return set_error(ESPM_EUNSUPPORTED, "channel diagnostics: k=%d (1..%d components)", k, ESPM_DIAG_MAX_K);
  ESPM_REQUIRE(x && d && h && dev && xsum && ysum && m_tri && scratch && n >= 1 && p >= 1, "channel diagnostics: bad arguments");
  if (int rc = check_image("channel diagnostics", x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "channel diagnostics: log_shift must be positive");
  ESPM_REQUIRE((n + ESPM_CDIAG_BLOCK - 1) / ESPM_CDIAG_BLOCK <= 65535, "channel diagnostics: n=%d (at most %d channels)", n,
               65535 * ESPM_CDIAG_BLOCK);
  const size_t need = espm_channel_diagnostics_scratch(n, p, k);
  ESPM_REQUIRE(scratch_bytes >= need, "channel diagnostics: scratch of %zu bytes, %zu needed (espm_channel_diagnostics_scratch)",
               scratch_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(scratch);
  const int rc = dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return cdiagk::launch<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, h, log_shift, part, s);
    });
  });
  if (rc) return rc;
  const int na = cdiagk::n_acc(k);
  const int n_chunks = (int)(((int64_t)p + ESPM_CDIAG_PCHUNK - 1) / ESPM_CDIAG_PCHUNK);
  const unsigned blocks = (unsigned)(((int64_t)na * n + 255) / 256);
  hipLaunchKernelGGL(cdiagk::reduce_kernel, dim3(blocks), dim3(256), 0, s, part, n, na, n_chunks, dev, xsum, ysum, m_tri);
  return check_hip(hipGetLastError(), "channel diagnostics reduction");
#endif
}
