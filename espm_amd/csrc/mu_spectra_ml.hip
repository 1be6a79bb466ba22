// One pass of the spectra ML (include/espm_mu.h, "spectra ML pass"): what the safeguarded Newton rule for W given H needs from the
// image, reduced over the PIXELS per channel.  The geometry, the tile and the reduction are mu_diag_chan.hip's (its file comment has
// the reasons); the accumulated sums are the observed-weight ones.  Per channel c, with y = max(d_c . h_p, log_shift):
//
//   dev_c = 2 sum_p (x ln(x / y) - x + y), sum_p x, sum_p y,
//   q_cj  = sum_p (x / y) h_jp                          (k sums: Q, whose G^T Q is the ratio numerator of the W step)
//   A_c   = sum_p (x / y^2) h_p h_p^T, lower triangle   (k (k + 1) / 2 sums: the observed information of row c of D = G W)
//
//   one channel per thread, ESPM_CDIAG_BLOCK channels and ESPM_CDIAG_PCHUNK pixels per workgroup: grid (pixel chunks, channel blocks)
//   d (k), q (k), the triangle and the three sums stay in registers (k = 8: 55 doubles); the chunk's columns of h go through LDS a
//                tile of pixels at a time and are read back as broadcasts
//   per entry: y (k FMAs), one division, x / y, one log where x > 0, x / y^2, k FMAs into q, k products and k (k + 1) / 2 FMAs into A
//   pixel-major X is read directly, eight rows in flight per thread (four at k = 7, 8: the registers the accumulators take);
//                channel-major X goes through the transposing LDS tile - both layouts run the same accumulation in the same order
//   each workgroup writes its 3 + k + k (k + 1) / 2 partial sums per channel to scratch[chunk][sum][channel]; a second launch adds
//                the chunks in ascending order.  No float atomics: two calls give the same bits.  The entries with counts under the
//                floor are an integer count (block_count_add onto the zeroed counter).
//
// The batched entry point (espm_spectra_ml_pass_batch) runs the same body for B models of one image, the model index in the third grid
// dimension, with its own slice of d, of the scratch and of the outputs; a model whose flag is 0 leaves both launches at entry.
//
// Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry points as stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace smlk {

constexpr int CB = ESPM_CDIAG_BLOCK;
constexpr int PC = ESPM_CDIAG_PCHUNK;
static_assert(CB % 64 == 0, "whole waves");

// pixels per tile and the padded row of the transposing tile: mu_diag_chan.hip's (rows an odd number of dwords apart)
template <typename XT>
struct Tile {
  static constexpr int P = sizeof(XT) <= 2 ? 64 : sizeof(XT) == 4 ? 32 : 16;
  static constexpr int TP = P + (sizeof(XT) == 1 ? 4 : sizeof(XT) == 2 ? 2 : 1);
};
constexpr int PM_TILE = 64;   // pixel-major X has no tile of its own: 64 columns of h per round

__host__ __device__ constexpr int n_tri(int k) { return k * (k + 1) / 2; }
__host__ __device__ constexpr int n_acc(int k) { return 3 + k + n_tri(k); }   // dev, sum x, sum y, q, the triangle

template <int K>
struct Acc {
  double d[K];
  double q[K];
  double a[K * (K + 1) / 2];
  double dev, xs, ys;
  double floor_y;
  uint32_t n_un;

  // one entry of X; hs: the tile's columns of h, component j of pixel t at hs[j * PT + t] (the same address in every lane)
  template <int PT>
  __device__ __forceinline__ void add(double xv, const double* __restrict__ hs, int t) {
    double hj[K];
    double y = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      hj[j] = hs[j * PT + t];
      y = fma(d[j], hj[j], y);
    }
    const bool floored = !(y >= floor_y);
    y = floored ? floor_y : y;
    n_un += (uint32_t)(floored && xv > 0);   // (a lane past the last channel reads zeros: it counts nothing)
    const double i = 1.0 / y;
    const double w = xv * i;
    double s = y - xv;
    if (xv > 0) s = fma(xv, log(w), s);
    dev += s;
    xs += xv;
    ys += y;
    const double v = w * i;
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = fma(w, hj[j], q[j]);
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const double hv = hj[r] * v;
#pragma unroll
      for (int j = 0; j <= r; ++j) a[r * (r + 1) / 2 + j] = fma(hv, hj[j], a[r * (r + 1) / 2 + j]);
    }
  }
};

// the pass of ONE model at d, its partial sums to part and its count onto *unmodelled: the whole body of both kernels below
template <int K, typename XT, bool PM>
__device__ __forceinline__ void pass_body(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                          const double* __restrict__ h, double log_shift, double* __restrict__ part,
                                          unsigned long long* __restrict__ unmodelled) {
  constexpr int PT = PM ? PM_TILE : Tile<XT>::P;
  constexpr int NA = n_acc(K);
  constexpr int FL = K >= 7 ? 4 : 8;   // rows of pixel-major X in flight per thread
  __shared__ double hs[K * PT];
  __shared__ uint32_t cnt_part[1][CB / 64];
  const int c0 = blockIdx.y * CB;
  const int c = c0 + threadIdx.x;
  const bool valid = c < n;
  const int q0 = blockIdx.x * PC;           // (p < 2^31: the entry point's int)
  const int qn = min(PC, p - q0);
  Acc<K> a;
#pragma unroll
  for (int j = 0; j < K; ++j) a.d[j] = valid ? d[(size_t)c * K + j] : 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) a.q[j] = 0;
#pragma unroll
  for (int i = 0; i < K * (K + 1) / 2; ++i) a.a[i] = 0;
  a.dev = a.xs = a.ys = 0;
  a.floor_y = log_shift;
  a.n_un = 0;

  for (int t0 = 0; t0 < qn; t0 += PT) {
    const int tn = min(PT, qn - t0);
    __syncthreads();   // (the readers of the round before)
    for (int i = threadIdx.x; i < K * PT; i += CB) {
      const int j = i / PT, t = i % PT;
      hs[i] = t < tn ? h[(size_t)j * p + (q0 + t0 + t)] : 0.0;
    }
    if constexpr (PM) {
      __syncthreads();
      const XT* xp = x + (size_t)(q0 + t0) * ld + c;
      for (int t = 0; t < tn; t += FL) {
        XT xv[FL];
#pragma unroll
        for (int u = 0; u < FL; ++u) xv[u] = (valid && t + u < tn) ? xp[(size_t)(t + u) * ld] : XT(0);
#pragma unroll
        for (int u = 0; u < FL; ++u)
          if (t + u < tn) a.template add<PT>((double)xv[u], hs, t + u);
      }
    } else {
      constexpr int TP = Tile<XT>::TP;
      __shared__ XT tile[CB * TP];
      // element e of the tile: channel e / PT, pixel e % PT - consecutive lanes read consecutive pixels of one channel's row
#pragma unroll 8
      for (int i = 0; i < PT; ++i) {
        const int e = i * CB + threadIdx.x;
        const int cc = e / PT, t = e % PT;
        XT v = XT(0);
        if (c0 + cc < n && t < tn) v = x[(size_t)(c0 + cc) * ld + (q0 + t0 + t)];
        tile[cc * TP + t] = v;
      }
      __syncthreads();
      const XT* row = tile + threadIdx.x * TP;
#pragma unroll 2
      for (int t = 0; t < tn; ++t) a.template add<PT>((double)row[t], hs, t);
    }
  }

  if (valid) {   // scratch[chunk][sum][channel]: coalesced here and in the reduction
    double* out = part + (size_t)blockIdx.x * NA * n + c;
    out[0] = a.dev;
    out[(size_t)n] = a.xs;
    out[(size_t)2 * n] = a.ys;
#pragma unroll
    for (int j = 0; j < K; ++j) out[(size_t)(3 + j) * n] = a.q[j];
#pragma unroll
    for (int i = 0; i < K * (K + 1) / 2; ++i) out[(size_t)(3 + K + i) * n] = a.a[i];
  }
  block_count_add<1, CB / 64>(cnt_part, {valid ? a.n_un : 0u}, unmodelled);   // (every thread of the workgroup is here)
}

template <int K, typename XT, bool PM>
__global__ __launch_bounds__(CB) void pass_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                  const double* __restrict__ h, double log_shift, double* __restrict__ part,
                                                  unsigned long long* __restrict__ unmodelled) {
  pass_body<K, XT, PM>(x, ld, n, p, d, h, log_shift, part, unmodelled);
}

// model blockIdx.z of a batch: d (B, n, K), part (B, chunks, sums, n), unmodelled (B,).  A retired model's workgroups leave at entry
// (the flag is the same for the whole workgroup: nobody waits at a barrier), before anything of X, d or h is read.
template <int K, typename XT, bool PM>
__global__ __launch_bounds__(CB) void pass_batch_kernel(const XT* __restrict__ x, int64_t ld, int n, int p, const double* __restrict__ d,
                                                        const double* __restrict__ h, const uint8_t* __restrict__ active, double log_shift,
                                                        double* __restrict__ part, unsigned long long* __restrict__ unmodelled) {
  const size_t b = blockIdx.z;
  if (active && !active[b]) return;
  pass_body<K, XT, PM>(x, ld, n, p, d + b * (size_t)n * K, h, log_shift, part + b * (size_t)gridDim.x * n_acc(K) * n, unmodelled + b);
}

// the chunks of every (sum, channel) added in ascending order: the one order there is, whatever the grid did (xsum null: not wanted)
__device__ __forceinline__ void reduce_body(const double* __restrict__ part, int n, int k, int n_chunks, double* __restrict__ dev,
                                            double* __restrict__ xsum, double* __restrict__ ysum, double* __restrict__ q,
                                            double* __restrict__ a_tri) {
  const int na = n_acc(k), nt = n_tri(k);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)na * n) return;
  const int s = (int)(i / n), c = (int)(i % n);
  double v = 0;
  for (int u = 0; u < n_chunks; ++u) v += part[((size_t)u * na + s) * n + c];
  if (s == 0) dev[c] = 2.0 * v;
  else if (s == 1) { if (xsum) xsum[c] = v; }
  else if (s == 2) ysum[c] = v;
  else if (s < 3 + k) q[(size_t)c * k + (s - 3)] = v;
  else a_tri[(size_t)c * nt + (s - 3 - k)] = v;
}

__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int n, int k, int n_chunks, double* __restrict__ dev,
                                                     double* __restrict__ xsum, double* __restrict__ ysum, double* __restrict__ q,
                                                     double* __restrict__ a_tri) {
  reduce_body(part, n, k, n_chunks, dev, xsum, ysum, q, a_tri);
}

// model blockIdx.y of a batch; a retired model's outputs are not written
__global__ __launch_bounds__(256) void reduce_batch_kernel(const double* __restrict__ part, int n, int k, int n_chunks,
                                                           const uint8_t* __restrict__ active, double* __restrict__ dev,
                                                           double* __restrict__ ysum, double* __restrict__ q, double* __restrict__ a_tri) {
  const size_t b = blockIdx.y;
  if (active && !active[b]) return;
  const size_t bn = b * (size_t)n;
  reduce_body(part + bn * n_acc(k) * n_chunks, n, k, n_chunks, dev + bn, nullptr, ysum + bn, q + bn * k, a_tri + bn * n_tri(k));
}

// the counters of the models that run, zeroed ahead of the pass (the flags live on the device: the host cannot pick them out)
__global__ __launch_bounds__(256) void zero_active_kernel(const uint8_t* __restrict__ active, int n_models,
                                                          unsigned long long* __restrict__ unmodelled) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < n_models && active[b]) unmodelled[b] = 0;
}

template <int K, typename XT>
int launch(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, double log_shift, double* part,
           unsigned long long* unmodelled, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + PC - 1) / PC), (unsigned)((n + CB - 1) / CB)), block(CB);
  const XT* xt = static_cast<const XT*>(x);
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pass_kernel<K, XT, true>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, part, unmodelled);
  else
    hipLaunchKernelGGL((pass_kernel<K, XT, false>), grid, block, 0, s, xt, ld, n, p, d, h, log_shift, part, unmodelled);
  return check_hip(hipGetLastError(), "spectra ML pass launch");
}

template <int K, typename XT>
int launch_batch(const void* x, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int n_models,
                 const uint8_t* active, double log_shift, double* part, unsigned long long* unmodelled, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + PC - 1) / PC), (unsigned)((n + CB - 1) / CB), (unsigned)n_models), block(CB);
  const XT* xt = static_cast<const XT*>(x);
  if (x_layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((pass_batch_kernel<K, XT, true>), grid, block, 0, s, xt, ld, n, p, d, h, active, log_shift, part, unmodelled);
  else
    hipLaunchKernelGGL((pass_batch_kernel<K, XT, false>), grid, block, 0, s, xt, ld, n, p, d, h, active, log_shift, part, unmodelled);
  return check_hip(hipGetLastError(), "spectra ML batch pass launch");
}

}  // namespace smlk
#endif

}  // namespace espm

using namespace espm;

extern "C" size_t espm_spectra_ml_pass_scratch(int n, int p, int k) {
#if ESPM_KP != 8
  (void)n; (void)p; (void)k;
  return 0;
#else
  if (n < 1 || p < 1 || k < 1 || k > ESPM_DIAG_MAX_K) return 0;
  const size_t chunks = (size_t)(((int64_t)p + ESPM_CDIAG_PCHUNK - 1) / ESPM_CDIAG_PCHUNK);
  return chunks * (size_t)smlk::n_acc(k) * (size_t)n * sizeof(double);
#endif
}

extern "C" int espm_spectra_ml_pass(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h,
                                    int k, double log_shift, double* dev, double* xsum, double* ysum, double* q, double* a_tri,
                                    int64_t* unmodelled, void* scratch, size_t scratch_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "spectra ML pass: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (k < 1 || k > ESPM_DIAG_MAX_K) return set_error(ESPM_EUNSUPPORTED, "spectra ML pass: k=%d (1..%d components)", k, ESPM_DIAG_MAX_K);
  ESPM_REQUIRE(x && d && h && dev && xsum && ysum && q && a_tri && unmodelled && scratch && n >= 1 && p >= 1,
               "spectra ML pass: bad arguments");
  if (int rc = check_image("spectra ML pass", x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "spectra ML pass: log_shift must be positive");
  ESPM_REQUIRE((n + ESPM_CDIAG_BLOCK - 1) / ESPM_CDIAG_BLOCK <= 65535, "spectra ML pass: n=%d (at most %d channels)", n,
               65535 * ESPM_CDIAG_BLOCK);
  const size_t need = espm_spectra_ml_pass_scratch(n, p, k);
  ESPM_REQUIRE(scratch_bytes >= need, "spectra ML pass: scratch of %zu bytes, %zu needed (espm_spectra_ml_pass_scratch)", scratch_bytes,
               need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(unmodelled, 0, sizeof(int64_t), s), "spectra ML pass: zeroing the counter")) return rc;
  double* part = static_cast<double*>(scratch);
  unsigned long long* un = reinterpret_cast<unsigned long long*>(unmodelled);
  const int rc = dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return smlk::launch<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, h, log_shift, part, un, s);
    });
  });
  if (rc) return rc;
  const int na = smlk::n_acc(k);
  const int n_chunks = (int)(((int64_t)p + ESPM_CDIAG_PCHUNK - 1) / ESPM_CDIAG_PCHUNK);
  const unsigned blocks = (unsigned)(((int64_t)na * n + 255) / 256);
  hipLaunchKernelGGL(smlk::reduce_kernel, dim3(blocks), dim3(256), 0, s, part, n, k, n_chunks, dev, xsum, ysum, q, a_tri);
  return check_hip(hipGetLastError(), "spectra ML pass reduction");
#endif
}

extern "C" size_t espm_spectra_ml_pass_batch_scratch(int n, int p, int k, int n_models) {
  if (n_models < 1 || n_models > ESPM_SML_MAX_MODELS) return 0;
  return (size_t)n_models * espm_spectra_ml_pass_scratch(n, p, k);
}

extern "C" int espm_spectra_ml_pass_batch(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d,
                                          const double* h, int k, int n_models, const uint8_t* active, double log_shift, double* dev,
                                          double* ysum, double* q, double* a_tri, int64_t* unmodelled, void* scratch, size_t scratch_bytes,
                                          espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "spectra ML batch pass: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (k < 1 || k > ESPM_DIAG_MAX_K)
    return set_error(ESPM_EUNSUPPORTED, "spectra ML batch pass: k=%d (1..%d components)", k, ESPM_DIAG_MAX_K);
  ESPM_REQUIRE(x && d && h && dev && ysum && q && a_tri && unmodelled && scratch && n >= 1 && p >= 1, "spectra ML batch pass: bad arguments");
  ESPM_REQUIRE(n_models >= 1 && n_models <= ESPM_SML_MAX_MODELS, "spectra ML batch pass: n_models=%d (1..%d)", n_models, ESPM_SML_MAX_MODELS);
  if (int rc = check_image("spectra ML batch pass", x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(log_shift > 0, "spectra ML batch pass: log_shift must be positive");
  ESPM_REQUIRE((n + ESPM_CDIAG_BLOCK - 1) / ESPM_CDIAG_BLOCK <= 65535, "spectra ML batch pass: n=%d (at most %d channels)", n,
               65535 * ESPM_CDIAG_BLOCK);
  const size_t need = espm_spectra_ml_pass_batch_scratch(n, p, k, n_models);
  ESPM_REQUIRE(scratch_bytes >= need, "spectra ML batch pass: scratch of %zu bytes, %zu needed (espm_spectra_ml_pass_batch_scratch)",
               scratch_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* un = reinterpret_cast<unsigned long long*>(unmodelled);
  if (active) {
    hipLaunchKernelGGL(smlk::zero_active_kernel, dim3((unsigned)((n_models + 255) / 256)), dim3(256), 0, s, active, n_models, un);
    if (int rc = check_hip(hipGetLastError(), "spectra ML batch pass: zeroing the counters")) return rc;
  } else if (int rc = check_hip(hipMemsetAsync(unmodelled, 0, (size_t)n_models * sizeof(int64_t), s),
                                "spectra ML batch pass: zeroing the counters")) {
    return rc;
  }
  double* part = static_cast<double*>(scratch);
  const int rc = dispatch_k_exact(k, [&](auto kk) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return smlk::launch_batch<decltype(kk)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, h, n_models, active, log_shift,
                                                                                  part, un, s);
    });
  });
  if (rc) return rc;
  const int na = smlk::n_acc(k);
  const int n_chunks = (int)(((int64_t)p + ESPM_CDIAG_PCHUNK - 1) / ESPM_CDIAG_PCHUNK);
  const unsigned blocks = (unsigned)(((int64_t)na * n + 255) / 256);
  hipLaunchKernelGGL(smlk::reduce_batch_kernel, dim3(blocks, (unsigned)n_models), dim3(256), 0, s, part, n, k, n_chunks, active, dev, ysum,
                     q, a_tri);
  return check_hip(hipGetLastError(), "spectra ML batch pass reduction");
#endif
}
