// Weighted marginals (include/espm_mu.h, "weighted marginals"): sums of the image, of its model and of the deviance term along one axis,
// for g weight vectors at once.  Weights over the channels give maps (an energy window, a background-corrected line), weights over the
// pixels give spectra (a phase mask, a label map, abundances as soft masks); the background correction of a line is linear in X, so a
// net line map is ONE signed weight vector and its Poisson variance the same pass with the weights squared.
//
// The kernel has the shape of attribk::expected_kernel (mu_image_pass.hpp's walk).  X is a matrix whose rows are ld apart; the index
// that runs along a row is the LANE index (a thread owns one, and the sums of one lane are one thread's), the index that runs across
// the rows is the WALK index - the SUMMED axis, the one the weights belong to.  Pixel side: lane = pixel, walk = channel; channel
// side: lane = channel, walk = pixel.  Channel-major X serves the pixel side directly and the channel side through the transposing
// tile; pixel-major X the other way round.  The lane's k-vector (h[:, pixel] or d[channel, :]) lives in registers; the walk's k-vector
// and its g weights go through LDS (the header's stage and stage_own) in rounds of 256 walk indices and are read back as broadcasts.  Per entry: the
// header's rule - y (k FMAs), one division, one log where x > 0, 3 g FMAs - in the same order in both layouts: the same bits.
//
//   pixel side    grid (lane blocks); the whole walk, channels ascending, in the pixel's thread; the g x 3 sums are stored as they end
//   channel side  grid (pixel chunks of ESPM_MARG_PCHUNK, lane blocks); pixels ascending; the partial sums go to
//                 scratch[chunk][sum][group][channel]; reduce_kernel adds the chunks in ascending order
//   k == 0        no model: only sum w x, and an entry with x == 0 costs its read only
//
// The skip.  A weight belongs to a walk index, so "all g weights of this index are 0" is the same for every lane of the workgroup.
// A thread stages the weights of ONE walk index of the round (stage_own) and knows whether it is live.  A round without a live index
// is left before its k-vectors are staged.  A dead index is never added, and
//   direct path   a ballot and the waves' counts make the ascending list of the round's live indices (idx[]); the walk runs over the
//                 LIST, eight rows of X at a time, their loads issued side by side and unconditionally (a list that ends inside the
//                 eight repeats its last index; a lane past the end reads the block's first column).  Behind a branch per row the loads
//                 went out one by one, a memory latency each: 8 windows of 20 channels took 0.33 ms instead of 0.06.
//   tile path     live[] marks the indices and tile_live[] the tiles; a tile - 64, 32 or 16 consecutive entries of every lane's row, one
//                 or two cache lines - is not filled when all its indices are dead, and a dead index inside a live tile is read with the
//                 tile and passed over (the flag is read as a scalar).
// So a window of 20 channels costs 20 rows of X, not 2048.  No bit changes: the live indices are added in ascending order and
// fma(0, v, a) == a for finite v (the header's argument).  A round whose every index is live looks nothing up.
//
// No value is accumulated atomically.  Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace margk {

constexpr int BT = ESPM_MARG_BLOCK;
constexpr int PC = ESPM_MARG_PCHUNK;
constexpr int CH = 256;      // walk indices per staging round: stage_rows<KP>() of every KP built here
constexpr int TP = BT + 1;   // lane stride of the transposing tile
static_assert(BT == 256 && CH == BT, "four waves of 64 lanes; a thread marks one walk index of a round");
static_assert(PC % CH == 0, "whole rounds of the staged vectors");
static_assert(stage_rows<4>() == CH && stage_rows<8>() == CH, "the rounds of the header's stage");

// KP: the padded stride of the k components (4 or 8), 0: no model.  GP: the padded stride of the g weight vectors (4 or 8).
// PIXEL_SIDE: lane = pixel, grid (lane blocks), the whole walk; o_xs, o_ys, o_dv (g, lanes), the deviance doubled.
// otherwise:  lane = channel, grid (pixel chunks, lane blocks); o_xs is the scratch [chunk][sum][group][lane], sums xs, ys, dv.
// TILE: the lane index runs across the rows of x (x[lane * ld + walk]) and x goes through the transposing tile.
template <int KP, int GP, typename XT, bool PIXEL_SIDE, bool TILE>
__global__ __launch_bounds__(BT) void marginals_kernel(const XT* __restrict__ x, int64_t ld, int lanes, int walks, Vec lv, Vec wv, int k, Vec gv,
                                                       int g, double log_shift, double* __restrict__ o_xs, double* __restrict__ o_ys,
                                                       double* __restrict__ o_dv) {
  constexpr int KA = KP ? KP : 1;
  constexpr int NA = KP ? 3 : 1;   // sums per group
  constexpr int TS = tile_rows<XT>();
  __shared__ double ds[CH * KA];
  __shared__ double ws[CH * GP];
  __shared__ unsigned short idx[TILE ? 1 : CH];          // direct path: the live walk indices of the round, ascending
  __shared__ int wave_cnt[BT / 64];
  __shared__ unsigned char live[TILE ? CH : 1];          // tile path: whether a walk index of the round is live,
  __shared__ unsigned char tile_live[TILE ? CH / TS : 1];   // and whether a tile holds a live one
  const int64_t l0 = (int64_t)(PIXEL_SIDE ? blockIdx.x : blockIdx.y) * BT;
  const int64_t l = l0 + threadIdx.x;
  const bool valid = l < lanes;
  const int64_t w_begin = PIXEL_SIDE ? 0 : (int64_t)blockIdx.x * PC;
  const int64_t w_end = PIXEL_SIDE ? (int64_t)walks : (w_begin + PC < walks ? w_begin + PC : (int64_t)walks);
  double a[KA], xs[GP], ys[GP], dv[GP];
#pragma unroll
  for (int j = 0; j < KA; ++j) a[j] = KP && valid && j < k ? lv.ptr[(int64_t)j * lv.cs + l * lv.qs] : 0.0;
#pragma unroll
  for (int q = 0; q < GP; ++q) xs[q] = ys[q] = dv[q] = 0.0;

  // one entry of X at the walk index c of the round
  auto add = [&](XT xe, int c) {
    const double* __restrict__ wq = ws + c * GP;
    const double xv = (double)xe;
    if constexpr (KP == 0) {
      if (xe != XT(0)) {
#pragma unroll
        for (int q = 0; q < GP; ++q) xs[q] = fma(wq[q], xv, xs[q]);
      }
    } else {
      const double* __restrict__ gk = ds + c * KP;
      double y = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j) y = fma(a[j], gk[j], y);
      y = fmax(y, log_shift);
      const double r = 1.0 / y;
      double t = y - xv;
      if (xv > 0) t = fma(xv, log(xv * r), t);
#pragma unroll
      for (int q = 0; q < GP; ++q) {
        const double w = wq[q];
        xs[q] = fma(w, xv, xs[q]);
        ys[q] = fma(w, y, ys[q]);
        dv[q] = fma(w, t, dv[q]);
      }
    }
  };

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t l_read = valid ? l : l0;   // (a lane past the end reads the block's first row or column - l0 < lanes - and stores nothing)
  for (int64_t c0 = w_begin; c0 < w_end; c0 += CH) {
    const int cn = (int)(w_end - c0 < CH ? w_end - c0 : CH);
    __syncthreads();   // (the readers of the round before)
    const bool mine = stage_own<GP, BT>(ws, gv, c0, cn, g);   // this thread's walk index: its weights, and whether it carries one
    const unsigned long long wave_live = __ballot(mine);
    if constexpr (TILE) live[threadIdx.x] = mine;
    else if (lane == 0) wave_cnt[wave] = __popcll(wave_live);
    const int n_live = __syncthreads_count(mine);
    if (n_live == 0) continue;   // (workgroup-uniform: no index of this round has a weight)
    if constexpr (TILE) {
      if (threadIdx.x < CH / TS) {
        bool any = false;
        for (int c = 0; c < TS; ++c) any |= live[threadIdx.x * TS + c] != 0;
        tile_live[threadIdx.x] = any;
      }
    } else if (mine) {   // the live indices of the round, in ascending order, one after the other
      int at = __popcll(wave_live & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) at += wave_cnt[w];
      idx[at] = (unsigned short)threadIdx.x;
    }
    if constexpr (KP != 0) {
      if constexpr (PIXEL_SIDE) stage<KP, BT>(ds, wv, c0, cn, k);   // rows of d
      else stage_own<KP, BT>(ds, wv, c0, cn, k);                    // columns of h: along the walk
    }
    __syncthreads();
    // live index number j of the round (direct path; clamped to the last one: a load that is issued whatever happens reads a live index
    // once more).  The same for every lane: a scalar.  A round whose every index is live looks nothing up.
    const bool dense = n_live == cn;
    auto nth = [&](int j) {
      j = j < n_live ? j : n_live - 1;
      return dense ? j : __builtin_amdgcn_readfirstlane((int)idx[j]);
    };
    if constexpr (!TILE) {
      const XT* xp = x + c0 * ld + l_read;
      for (int i = 0; i < n_live; i += 8) {   // eight loads in flight: none of them behind a branch
        int cu[8];
        XT xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          cu[u] = nth(i + u);
          xv[u] = xp[(int64_t)cu[u] * ld];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (i + u < n_live) add(xv[u], cu[u]);   // (uniform)
      }
    } else {
      __shared__ XT tile[TS * TP];
      static_assert(TS % 8 == 0, "the tile is read back eight walk indices at a time");
      for (int t0 = 0; t0 < cn; t0 += TS) {
        if (!dense && !tile_live[t0 / TS]) continue;   // (workgroup-uniform)
        const int tn = cn - t0 < TS ? cn - t0 : TS;
        __syncthreads();   // (the tile's readers of the round before)
        fill_tile<XT, BT>(tile, x, ld, l0, lanes, c0 + t0, tn);
        __syncthreads();
        for (int c = 0; c < tn; c += 8) {
          XT xv[8];
          bool on[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            on[u] = c + u < tn && (dense || __builtin_amdgcn_readfirstlane((int)live[t0 + c + u]) != 0);   // (the same for every lane: a scalar)
            xv[u] = tile[(c + u) * TP + threadIdx.x];   // (c + u < TS: inside the tile, zeros beyond tn and beyond the lanes)
          }
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (on[u]) add(xv[u], t0 + c + u);   // (uniform)
        }
      }
    }
  }
  if (valid) {
    if constexpr (PIXEL_SIDE) {
#pragma unroll
      for (int q = 0; q < GP; ++q)
        if (q < g) {
          o_xs[(int64_t)q * lanes + l] = xs[q];
          if constexpr (KP != 0) {
            o_ys[(int64_t)q * lanes + l] = ys[q];
            o_dv[(int64_t)q * lanes + l] = 2.0 * dv[q];
          }
        }
    } else {
      double* o = o_xs + (int64_t)blockIdx.x * NA * g * lanes + l;
#pragma unroll
      for (int q = 0; q < GP; ++q)
        if (q < g) {
          o[(int64_t)q * lanes] = xs[q];
          if constexpr (KP != 0) {
            o[((int64_t)g + q) * lanes] = ys[q];
            o[((int64_t)2 * g + q) * lanes] = dv[q];
          }
        }
    }
  }
}

// the chunks of every (sum, group, channel) added in ascending order: the one order there is, whatever the grid did
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int64_t gn, int na, int n_chunks, double* __restrict__ xs,
                                                     double* __restrict__ ys, double* __restrict__ dev) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)na * gn) return;
  const int s = (int)(i / gn);
  const int64_t r = i % gn;
  double v = 0.0;
  for (int q = 0; q < n_chunks; ++q) v += part[((int64_t)q * na + s) * gn + r];
  if (s == 0) xs[r] = v;
  else if (s == 1) ys[r] = v;
  else dev[r] = 2.0 * v;
}

template <int KP, int GP, typename XT>
int launch(const void* x, int layout, int64_t ld, int n, int p, int side, const double* wgt, int g, const double* d, const double* h, int k,
           double log_shift, double* xs, double* ys, double* dev, double* part, hipStream_t s) {
  const XT* xt = static_cast<const XT*>(x);
  const Vec hv = {h, (int64_t)p, 1}, dvec = {d, 1, (int64_t)k};
  const dim3 block(BT);
  if (side == ESPM_MARG_PIXELS) {
    const dim3 grid((unsigned)(((int64_t)p + BT - 1) / BT));
    const Vec gv = {wgt, (int64_t)n, 1};
    if (layout == ESPM_LAYOUT_CM)
      hipLaunchKernelGGL((marginals_kernel<KP, GP, XT, true, false>), grid, block, 0, s, xt, ld, p, n, hv, dvec, k, gv, g, log_shift, xs, ys, dev);
    else
      hipLaunchKernelGGL((marginals_kernel<KP, GP, XT, true, true>), grid, block, 0, s, xt, ld, p, n, hv, dvec, k, gv, g, log_shift, xs, ys, dev);
    return check_hip(hipGetLastError(), "weighted marginals launch");
  }
  const int n_chunks = (int)(((int64_t)p + PC - 1) / PC);
  const dim3 grid((unsigned)n_chunks, (unsigned)((n + BT - 1) / BT));
  const Vec gv = {wgt, (int64_t)p, 1};
  double* none = nullptr;
  if (layout == ESPM_LAYOUT_CM)
    hipLaunchKernelGGL((marginals_kernel<KP, GP, XT, false, true>), grid, block, 0, s, xt, ld, n, p, dvec, hv, k, gv, g, log_shift, part, none, none);
  else
    hipLaunchKernelGGL((marginals_kernel<KP, GP, XT, false, false>), grid, block, 0, s, xt, ld, n, p, dvec, hv, k, gv, g, log_shift, part, none, none);
  if (int rc = check_hip(hipGetLastError(), "weighted marginals launch")) return rc;
  const int na = KP ? 3 : 1;
  const int64_t gn = (int64_t)g * n;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)((na * gn + 255) / 256)), dim3(256), 0, s, part, gn, na, n_chunks, xs, ys, dev);
  return check_hip(hipGetLastError(), "weighted marginals reduction");
}

// f(std::integral_constant<int, S>) for the padded stride S = 4 or 8 that holds v vectors; S = 0 for v == 0 where ZERO allows it
template <bool ZERO, typename F>
int dispatch_stride(int v, F&& f) {
  if constexpr (ZERO)
    if (v == 0) return f(std::integral_constant<int, 0>{});
  if (v <= 4) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

}  // namespace margk
#endif

}  // namespace espm

using namespace espm;

extern "C" size_t espm_weighted_marginals_scratch(int side, int n, int p, int g) {
#if ESPM_KP != 8
  (void)side; (void)n; (void)p; (void)g;
  return 0;
#else
  if (side != ESPM_MARG_CHANNELS || n < 1 || p < 1 || g < 1 || g > ESPM_MARG_MAX_G) return 0;
  const size_t chunks = (size_t)(((int64_t)p + ESPM_MARG_PCHUNK - 1) / ESPM_MARG_PCHUNK);
  return chunks * 3 * (size_t)g * (size_t)n * sizeof(double);
#endif
}

extern "C" int espm_weighted_marginals(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int side, const double* wgt, int g,
                                       const double* d, const double* h, int k, double log_shift, double* xs, double* ys, double* dev,
                                       void* scratch, size_t scratch_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "weighted marginals: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  const char* who = "weighted marginals";
  ESPM_REQUIRE(x && wgt && xs, "%s: bad arguments (x %p, wgt %p, xs %p)", who, x, (const void*)wgt, (void*)xs);
  ESPM_REQUIRE(side == ESPM_MARG_PIXELS || side == ESPM_MARG_CHANNELS, "%s: side %d", who, side);
  if (int rc = check_image(who, x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE(g >= 1 && g <= ESPM_MARG_MAX_G, "%s: g=%d (1..%d weight vectors)", who, g, ESPM_MARG_MAX_G);
  ESPM_REQUIRE(k >= 0 && k <= ESPM_MARG_MAX_K, "%s: k=%d (0..%d components)", who, k, ESPM_MARG_MAX_K);
  if (k > 0) {
    ESPM_REQUIRE(d && h && ys && dev, "%s: k=%d needs the model and its outputs (d %p, h %p, ys %p, dev %p)", who, k, (const void*)d,
                 (const void*)h, (void*)ys, (void*)dev);
    ESPM_REQUIRE(log_shift > 0, "%s: log_shift=%g must be positive", who, log_shift);
  } else {
    ESPM_REQUIRE(!d && !h && !ys && !dev, "%s: k=0 takes no model and forms no model sums (d %p, h %p, ys %p, dev %p must be NULL)", who,
                 (const void*)d, (const void*)h, (void*)ys, (void*)dev);
  }
  double* part = nullptr;
  if (side == ESPM_MARG_CHANNELS) {
    ESPM_REQUIRE((n + ESPM_MARG_BLOCK - 1) / ESPM_MARG_BLOCK <= 65535, "%s: n=%d (at most %d channels)", who, n, 65535 * ESPM_MARG_BLOCK);
    const size_t need = espm_weighted_marginals_scratch(side, n, p, g);
    ESPM_REQUIRE(scratch, "%s: bad arguments (scratch %p, %zu bytes needed)", who, scratch, need);
    ESPM_REQUIRE(scratch_bytes >= need, "%s: scratch of %zu bytes, %zu needed (espm_weighted_marginals_scratch)", who, scratch_bytes, need);
    part = static_cast<double*>(scratch);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  return margk::dispatch_stride<true>(k, [&](auto kp) {
    return margk::dispatch_stride<false>(g, [&](auto gp) {
      return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
        return margk::launch<decltype(kp)::value, decltype(gp)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, side, wgt, g, d, h, k,
                                                                                                    log_shift, xs, ys, dev, part, s);
      });
    });
  });
#endif
}
