// Residual products (include/espm_mu.h, "residual products"): the Pearson residual matrix E = (X - Y) / sqrt(Y), Y = D H, applied to g
// dense vectors at once from either side - E^T U (a value per pixel) or E V (a value per channel) - with the Pearson chi^2 of every
// pixel or channel.  E is never stored: a block subspace iteration for its leading singular triplets (espm_amd/residuals.py) is a
// sequence of such passes over X, and (x - y) / sqrt(y) is not linear in anything the weighted marginals sum.
//
// The kernel has the geometry of margk::marginals_kernel (mu_marginals.hip's file comment): the LANE index runs along a row of X and a
// thread owns one, the WALK index is the summed axis, the one the vectors belong to.  Pixel side: lane = pixel, walk = channel; channel
// side: lane = channel, walk = pixel.  The lane's k-vector lives in registers; the walk's k-vector and its g values go through LDS
// (the header's stage and stage_own) in rounds of 256 and are read back as broadcasts.  Channel-major X serves the pixel side directly
// and the channel side through the transposing tile; pixel-major X the other way round.  Per entry: the header's rule - y (k FMAs),
// one comparison, one subtraction, one square root, one division, g + 1 FMAs - in the same order in both layouts: the same bits.
//
//   pixel side    grid (lane blocks); the whole walk, channels ascending, in the pixel's thread; the g sums and chi2 stored as they end
//   channel side  grid (pixel chunks of ESPM_RESID_PCHUNK, lane blocks); pixels ascending; the partial sums go to
//                 scratch[chunk][vector, then chi2][channel]; reduce_kernel adds the chunks in ascending order
//
// The vectors are dense: every walk index is read, there is nothing to skip and no list of live indices.  On the direct path the loads
// of eight rows of X are issued side by side, none of them behind a branch (a round that ends inside the eight repeats its last row).
//
// No value is accumulated atomically.  The number of entries with counts where the model has no rate is a sum of integers
// (block_count_add, onto the zeroed counter).  Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace residk {

constexpr int BT = ESPM_RESID_BLOCK;
constexpr int PC = ESPM_RESID_PCHUNK;
constexpr int CH = 256;      // walk indices per staging round: stage_rows<KP>() of every KP built here
constexpr int TP = BT + 1;   // lane stride of the transposing tile
constexpr int64_t FLUSH = (int64_t)1 << 24;   // walk indices after which a thread's count goes to the counter: 64 lanes of them stay below 2^32
static_assert(BT == 256 && CH == BT, "four waves of 64 lanes; a thread stages one walk index of a round");
static_assert(PC % CH == 0 && FLUSH % CH == 0, "whole rounds of the staged vectors");
static_assert(stage_rows<4>() == CH && stage_rows<8>() == CH, "the rounds of the header's stage");

// KP: the padded stride of the k components (4 or 8).  GP: the padded stride of the g vectors (4 or 8).
// PIXEL_SIDE: lane = pixel, grid (lane blocks), the whole walk; o (g, lanes), o_chi2 (lanes) or null.
// otherwise:  lane = channel, grid (pixel chunks, lane blocks); o is the scratch [chunk][g + 1][lane], the last row chi2.
// TILE: the lane index runs across the rows of x (x[lane * ld + walk]) and x goes through the transposing tile.
template <int KP, int GP, typename XT, bool PIXEL_SIDE, bool TILE>
__global__ __launch_bounds__(BT) void residual_kernel(const XT* __restrict__ x, int64_t ld, int lanes, int walks, Vec lv, Vec wv, int k, Vec gv,
                                                      int g, double log_shift, double* __restrict__ o, double* __restrict__ o_chi2,
                                                      unsigned long long* __restrict__ unmodelled) {
  constexpr int TS = tile_rows<XT>();
  __shared__ double ds[CH * KP];
  __shared__ double ws[CH * GP];
  __shared__ uint32_t cnt_part[1][BT / 64];
  const int64_t l0 = (int64_t)(PIXEL_SIDE ? blockIdx.x : blockIdx.y) * BT;
  const int64_t l = l0 + threadIdx.x;
  const bool valid = l < lanes;
  const int64_t w_begin = PIXEL_SIDE ? 0 : (int64_t)blockIdx.x * PC;
  const int64_t w_end = PIXEL_SIDE ? (int64_t)walks : (w_begin + PC < walks ? w_begin + PC : (int64_t)walks);
  double a[KP], acc[GP], chi = 0.0;
  uint32_t n_un = 0;
#pragma unroll
  for (int j = 0; j < KP; ++j) a[j] = valid && j < k ? lv.ptr[(int64_t)j * lv.cs + l * lv.qs] : 0.0;
#pragma unroll
  for (int q = 0; q < GP; ++q) acc[q] = 0.0;

  // one entry of X at the walk index c of the round (a lane past the end has a == 0: floored, and it counts nothing)
  auto add = [&](XT xe, int c) {
    const double* __restrict__ vq = ws + c * GP;
    const double* __restrict__ gk = ds + c * KP;
    const double xv = (double)xe;
    double y = 0.0;
#pragma unroll
    for (int j = 0; j < KP; ++j) y = fma(a[j], gk[j], y);
    const bool floored = !(y >= log_shift);
    double e = 0.0;
    if (!floored) {
      const double num = xv - y;
      const double den = sqrt(y);
      e = num / den;
    }
    n_un += (uint32_t)(floored && valid && xv > 0);
#pragma unroll
    for (int q = 0; q < GP; ++q) acc[q] = fma(vq[q], e, acc[q]);
    chi = fma(e, e, chi);
  };

  const int64_t l_read = valid ? l : l0;   // (a lane past the end reads the block's first row or column - l0 < lanes - and stores nothing)
  for (int64_t c0 = w_begin; c0 < w_end; c0 += CH) {
    const int cn = (int)(w_end - c0 < CH ? w_end - c0 : CH);
    if (PIXEL_SIDE && c0 != 0 && c0 % FLUSH == 0 && unmodelled) {   // (workgroup-uniform; the channel side walks PC indices)
      block_count_add<1>(cnt_part, {n_un}, unmodelled);
      n_un = 0;
    }
    __syncthreads();   // (the readers of the round before)
    stage_own<GP, BT>(ws, gv, c0, cn, g);   // the g values of this thread's walk index
    if constexpr (PIXEL_SIDE) stage<KP, BT>(ds, wv, c0, cn, k);   // rows of d
    else stage_own<KP, BT>(ds, wv, c0, cn, k);                    // columns of h: along the walk
    __syncthreads();
    if constexpr (!TILE) {
      const XT* xp = x + c0 * ld + l_read;
      for (int i = 0; i < cn; i += 8) {   // eight loads in flight
        XT xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int c = i + u < cn ? i + u : cn - 1;
          xv[u] = xp[(int64_t)c * ld];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i + u < cn) add(xv[u], i + u);   // (uniform)
      }
    } else {
      __shared__ XT tile[TS * TP];
      static_assert(TS % 8 == 0, "the tile is read back eight walk indices at a time");
      for (int t0 = 0; t0 < cn; t0 += TS) {
        const int tn = cn - t0 < TS ? cn - t0 : TS;
        __syncthreads();   // (the tile's readers of the round before)
        fill_tile<XT, BT>(tile, x, ld, l0, lanes, c0 + t0, tn);
        __syncthreads();
        for (int c = 0; c < tn; c += 8) {
          XT xv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) xv[u] = tile[(c + u) * TP + threadIdx.x];   // (c + u < TS: inside the tile, zeros beyond tn and the lanes)
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (c + u < tn) add(xv[u], t0 + c + u);   // (uniform)
        }
      }
    }
  }
  if (valid) {
    if constexpr (PIXEL_SIDE) {
#pragma unroll
      for (int q = 0; q < GP; ++q)
        if (q < g) o[(int64_t)q * lanes + l] = acc[q];
      if (o_chi2) o_chi2[l] = chi;
    } else {
      double* op = o + (int64_t)blockIdx.x * (g + 1) * lanes + l;
#pragma unroll
      for (int q = 0; q < GP; ++q)
        if (q < g) op[(int64_t)q * lanes] = acc[q];
      op[(int64_t)g * lanes] = chi;
    }
  }
  if (unmodelled) block_count_add<1>(cnt_part, {n_un}, unmodelled);   // (workgroup-uniform)
}

// the chunks of every (vector or chi2, channel) added in ascending order: the one order there is, whatever the grid did
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int g, int n, int n_chunks, double* __restrict__ out,
                                                     double* __restrict__ chi2) {
  const int64_t rows = (int64_t)(g + 1) * n;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  double v = 0.0;
  for (int q = 0; q < n_chunks; ++q) v += part[(int64_t)q * rows + i];
  if (i < (int64_t)g * n) out[i] = v;
  else if (chi2) chi2[i - (int64_t)g * n] = v;
}

template <int KP, int GP, typename XT>
int launch(const void* x, int layout, int64_t ld, int n, int p, int side, const double* vec, int g, const double* d, const double* h, int k,
           double log_shift, double* out, double* chi2, unsigned long long* unmodelled, double* part, hipStream_t s) {
  const XT* xt = static_cast<const XT*>(x);
  const Vec hv = {h, (int64_t)p, 1}, dvec = {d, 1, (int64_t)k};
  const dim3 block(BT);
  if (side == ESPM_RESID_PIXELS) {
    const dim3 grid((unsigned)(((int64_t)p + BT - 1) / BT));
    const Vec gv = {vec, (int64_t)n, 1};
    if (layout == ESPM_LAYOUT_CM)
      hipLaunchKernelGGL((residual_kernel<KP, GP, XT, true, false>), grid, block, 0, s, xt, ld, p, n, hv, dvec, k, gv, g, log_shift, out, chi2, unmodelled);
    else
      hipLaunchKernelGGL((residual_kernel<KP, GP, XT, true, true>), grid, block, 0, s, xt, ld, p, n, hv, dvec, k, gv, g, log_shift, out, chi2, unmodelled);
    return check_hip(hipGetLastError(), "residual products launch");
  }
  const int n_chunks = (int)(((int64_t)p + PC - 1) / PC);
  const dim3 grid((unsigned)n_chunks, (unsigned)((n + BT - 1) / BT));
  const Vec gv = {vec, (int64_t)p, 1};
  double* none = nullptr;
  if (layout == ESPM_LAYOUT_CM)
    hipLaunchKernelGGL((residual_kernel<KP, GP, XT, false, true>), grid, block, 0, s, xt, ld, n, p, dvec, hv, k, gv, g, log_shift, part, none, unmodelled);
  else
    hipLaunchKernelGGL((residual_kernel<KP, GP, XT, false, false>), grid, block, 0, s, xt, ld, n, p, dvec, hv, k, gv, g, log_shift, part, none, unmodelled);
  if (int rc = check_hip(hipGetLastError(), "residual products launch")) return rc;
  const int64_t rows = (int64_t)(g + 1) * n;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, part, g, n, n_chunks, out, chi2);
  return check_hip(hipGetLastError(), "residual products reduction");
}

// f(std::integral_constant<int, S>) for the padded stride S = 4 or 8 that holds v vectors
template <typename F>
int dispatch_stride(int v, F&& f) {
  if (v <= 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

}  // namespace residk
#endif

}  // namespace espm

using namespace espm;

extern "C" size_t espm_residual_products_scratch(int side, int n, int p, int g) {
#if ESPM_KP != 8
  (void)side; (void)n; (void)p; (void)g;
  return 0;
#else
  if (side != ESPM_RESID_CHANNELS || n < 1 || p < 1 || g < 1 || g > ESPM_RESID_MAX_G) return 0;
  const size_t chunks = (size_t)(((int64_t)p + ESPM_RESID_PCHUNK - 1) / ESPM_RESID_PCHUNK);
  return chunks * ((size_t)g + 1) * (size_t)n * sizeof(double);
#endif
}

extern "C" int espm_residual_products(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int side, const double* vec, int g,
                                      const double* d, const double* h, int k, double log_shift, double* out, double* chi2, int64_t* unmodelled,
                                      void* scratch, size_t scratch_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "residual products: built into the 1..%d component library only", ESPM_RESID_MAX_K);
#else
  const char* who = "residual products";
  ESPM_REQUIRE(x && vec && d && h && out, "%s: bad arguments (x %p, vec %p, d %p, h %p, out %p)", who, x, (const void*)vec, (const void*)d,
               (const void*)h, (void*)out);
  ESPM_REQUIRE(side == ESPM_RESID_PIXELS || side == ESPM_RESID_CHANNELS, "%s: side %d", who, side);
  if (int rc = check_image(who, x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(g >= 1 && g <= ESPM_RESID_MAX_G, "%s: g=%d (1..%d vectors)", who, g, ESPM_RESID_MAX_G);
  ESPM_REQUIRE(k >= 1 && k <= ESPM_RESID_MAX_K, "%s: k=%d (1..%d components)", who, k, ESPM_RESID_MAX_K);
  ESPM_REQUIRE(log_shift > 0, "%s: log_shift=%g must be positive", who, log_shift);
  double* part = nullptr;
  if (side == ESPM_RESID_CHANNELS) {
    ESPM_REQUIRE((n + ESPM_RESID_BLOCK - 1) / ESPM_RESID_BLOCK <= 65535, "%s: n=%d (at most %d channels)", who, n, 65535 * ESPM_RESID_BLOCK);
    const size_t need = espm_residual_products_scratch(side, n, p, g);
    ESPM_REQUIRE(scratch, "%s: bad arguments (scratch %p, %zu bytes needed)", who, scratch, need);
    ESPM_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes, %zu needed (espm_residual_products_scratch)", who, scratch_bytes, need);
    part = static_cast<double*>(scratch);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (unmodelled)
    if (int rc = check_hip(hipMemsetAsync(unmodelled, 0, sizeof(int64_t), s), "residual products: zeroing the counter")) return rc;
  unsigned long long* un = reinterpret_cast<unsigned long long*>(unmodelled);
  return residk::dispatch_stride(k, [&](auto kp) {
    return residk::dispatch_stride(g, [&](auto gp) {
      return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
        return residk::launch<decltype(kp)::value, decltype(gp)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, side, vec, g, d, h, k,
                                                                                                     log_shift, out, chi2, un, part, s);
      });
    });
  });
#endif
}
