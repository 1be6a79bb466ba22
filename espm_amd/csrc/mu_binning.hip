// Pixel binning (include/espm_mu.h, "pixel binning"): the bin sums S_gc of a spectrum image over (by, bx) blocks of pixels, and the four
// sums the best-binning estimator is made of, straight from X in its own dtype and layout.  Bandwidth-bound, one pass over X each.
//
//   channel-major X ((n, p)): a work item is (channel, bin row).  The lanes run along the pixels of an image row: a thread owns a
//                column of the strip and adds the bin row's `by` image rows of it (eight loads in flight), the column sums go to LDS
//                and thread b adds the bx columns of bin b.  A strip is as many whole bins as fit ESPM_BIN_BLOCK columns (one bin,
//                walked in pieces, when bx is larger).
//   pixel-major X ((p, n), hyperspy's layout): a work item is (bin, 64 channels).  The lanes of a wave run along the channels; the four
//                waves of the workgroup take every fourth pixel of the bin and thread c of wave 0 adds the four partial sums from LDS.
//   integer input is summed exactly in 64-bit integers, floating-point input in fp64; every order of additions is fixed by the
//                shape alone, so two calls give the same bits.
//                A pixel-major candidate with fewer than ESPM_BIN_PARTS work items (large bins) is cut into slabs of image rows first:
//                their sums go through the scratch and a second launch joins them, in ascending order, before they are squared.
//   espm_rebin_pixels: one work item per workgroup, S rounded once to the output dtype.
//   espm_binning_sums: ESPM_BIN_PARTS workgroups per launch walk the work items in a fixed stride; a thread keeps sum S^2 / n_g and
//                sum S / n_g (the totals' launch: sum x, sum x^2) in fp64, the workgroup reduces them in a fixed order and writes
//                scratch[slot][workgroup]; one launch per candidate bin, then one launch adds every slot's partials in ascending
//                order.  No atomics.
//
// Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry points as stubs.
#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
namespace bink {

constexpr int BT = ESPM_BIN_BLOCK;
constexpr int PARTS = ESPM_BIN_PARTS;
constexpr int PM_C = 64;             // channels per work item of pixel-major X: one wave's lanes
constexpr int PM_SUB = BT / PM_C;    // the waves share a bin's pixels
static_assert(BT == 256 && PM_SUB == 4, "four waves of 64 lanes");

template <typename XT> struct Sum { using T = double; };
template <> struct Sum<uint8_t> { using T = uint64_t; };
template <> struct Sum<uint16_t> { using T = uint64_t; };

__device__ __forceinline__ void add8(uint64_t& s, const uint8_t (&v)[8]) {
  s += (uint32_t)v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6] + v[7];
}
__device__ __forceinline__ void add8(uint64_t& s, const uint16_t (&v)[8]) {
  s += (uint32_t)v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6] + v[7];
}
template <typename XT>
__device__ __forceinline__ void add8(double& s, const XT (&v)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) s += (double)v[u];
}

// the image and one bin: by <= ny and bx <= nx (the entry points clamp: a larger bin is the whole axis)
struct Geo {
  int64_t ld;
  int n, ny, nx, by, bx, gny, gnx;
};

// One (channel, bin row) of channel-major X; xc: the channel's row of X.  emit(gx, S, n_g) runs in one thread per bin.
// Every thread of the workgroup calls this (barriers inside); cs: BT sums of LDS.
template <typename XT, typename Emit>
__device__ __forceinline__ void cm_bin_row(const XT* __restrict__ xc, const Geo& g, int gy, typename Sum<XT>::T* cs, Emit emit) {
  using ST = typename Sum<XT>::T;
  const int tid = threadIdx.x;
  const int y0 = gy * g.by, rows = min(g.by, g.ny - y0);
  const int nb = g.bx <= BT ? BT / g.bx : 1;   // bins per strip
  const int64_t sw = (int64_t)nb * g.bx;       // columns per strip
  for (int64_t x0 = 0; x0 < g.nx; x0 += sw) {
    const int xe = (int)min((int64_t)g.nx, x0 + sw);
    ST s = 0;
    for (int64_t col = x0 + tid; col < xe; col += BT) {   // (one trip unless bx > BT)
      const XT* px = xc + (int64_t)y0 * g.nx + col;
      int r = 0;
      for (; r + 8 <= rows; r += 8) {
        XT v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = px[(int64_t)(r + u) * g.nx];
        add8(s, v);
      }
      for (; r < rows; ++r) s += (ST)px[(int64_t)r * g.nx];
    }
    __syncthreads();   // (the readers of the strip before)
    cs[tid] = s;
    __syncthreads();
    const int64_t b0 = x0 + (int64_t)tid * g.bx;   // first column of this thread's bin
    if (tid < nb && b0 < xe) {
      const int cols = g.bx <= BT ? min(g.bx, (int)(xe - b0)) : (int)(xe - x0);
      const int cnt = min(cols, BT), off = g.bx <= BT ? tid * g.bx : 0;
      ST S = 0;
      for (int i = 0; i < cnt; ++i) S += cs[off + i];
      emit((int)(x0 / g.bx) + tid, S, (double)rows * (double)cols);
    }
  }
}

// The sum over the pixels [y0, y0 + rows) x [x0, x0 + cols) of pixel-major X for PM_C channels from c0 (a bin, or a slab of its image
// rows).  emit(c, S) runs in the thread of wave 0 that owns channel c.  Every thread of the workgroup calls this (barriers inside).
// Wide blocks are walked row by row, a wave taking every fourth pixel of the row (eight loads in flight off one row pointer); narrow
// ones as one list of pixels, every fourth to a wave.  Which walk is taken follows from the shape alone.
template <typename XT, typename Emit>
__device__ __forceinline__ void pm_bin(const XT* __restrict__ x, const Geo& g, int y0, int rows, int x0, int cols, int c0,
                                       typename Sum<XT>::T* cs, Emit emit) {
  using ST = typename Sum<XT>::T;
  const int tid = threadIdx.x, cl = tid & (PM_C - 1), sub = tid / PM_C, c = c0 + cl;
  ST s = 0;
  if (c < g.n) {
    if (cols >= 8 * PM_SUB) {
      for (int r = 0; r < rows; ++r) {
        const XT* px = x + ((int64_t)(y0 + r) * g.nx + x0) * g.ld + c;
        int cc = sub;
        for (; cc + 7 * PM_SUB < cols; cc += 8 * PM_SUB) {
          XT v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = px[(int64_t)(cc + u * PM_SUB) * g.ld];
          add8(s, v);
        }
        for (; cc < cols; cc += PM_SUB) s += (ST)px[(int64_t)cc * g.ld];
      }
    } else {
      int r = sub / cols, cc = sub % cols;   // this wave's pixels: sub, sub + 4, ... of the block, row by row
      while (r < rows) {
        XT v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          v[u] = r < rows ? x[((int64_t)(y0 + r) * g.nx + (x0 + cc)) * g.ld + c] : XT(0);
          cc += PM_SUB;
          while (cc >= cols && r < rows) {
            cc -= cols;
            ++r;
          }
        }
        add8(s, v);
      }
    }
  }
  __syncthreads();   // (the readers of the item before)
  cs[tid] = s;
  __syncthreads();
  if (sub == 0 && c < g.n) {
    ST S = cs[cl];
#pragma unroll
    for (int u = 1; u < PM_SUB; ++u) S += cs[u * PM_C + cl];
    emit(c, S);
  }
}

// rows and columns of bin (gy, gx)
struct Block {
  int y0, rows, x0, cols;
};
__device__ __forceinline__ Block block_of(const Geo& g, int gy, int gx) {
  Block b;
  b.y0 = gy * g.by, b.rows = min(g.by, g.ny - b.y0);
  b.x0 = gx * g.bx, b.cols = min(g.bx, g.nx - b.x0);
  return b;
}

template <typename OT, typename ST>
__device__ __forceinline__ OT round_once(ST S) { return (OT)(double)S; }   // (integer sums are below 2^53: the conversion to double is exact)

template <typename XT, typename OT, bool PM>
__global__ __launch_bounds__(BT) void rebin_kernel(const XT* __restrict__ x, Geo g, OT* __restrict__ out, int64_t out_ld) {
  using ST = typename Sum<XT>::T;
  __shared__ ST cs[BT];
  if constexpr (PM) {
    const int bin = blockIdx.x;
    const Block b = block_of(g, bin / g.gnx, bin % g.gnx);
    pm_bin<XT>(x, g, b.y0, b.rows, b.x0, b.cols, blockIdx.y * PM_C, cs, [&](int c, ST S) { out[(int64_t)bin * out_ld + c] = round_once<OT>(S); });
  } else {
    const int c = blockIdx.x / g.gny, gy = blockIdx.x % g.gny;
    OT* orow = out + (int64_t)c * out_ld + (int64_t)gy * g.gnx;
    cm_bin_row<XT>(x + (int64_t)c * g.ld, g, gy, cs, [&](int gx, ST S, double) { orow[gx] = round_once<OT>(S); });
  }
}

// sum S^2 / n_g and sum S / n_g of one candidate bin: partials to part[0][wg] and part[1][wg] (rows PARTS apart)
template <typename XT, bool PM>
__global__ __launch_bounds__(BT) void bin_sums_kernel(const XT* __restrict__ x, Geo g, double* __restrict__ part) {
  using ST = typename Sum<XT>::T;
  __shared__ ST cs[BT];
  __shared__ double red[(BT / 64 + 1) * 2];
  double v[2] = {0.0, 0.0};
  auto take = [&](int, ST S, double ng) {
    const double s = (double)S;
    v[0] += s * s / ng;
    v[1] += s / ng;
  };
  if constexpr (PM) {
    const int cblocks = (g.n + PM_C - 1) / PM_C;
    const int64_t items = (int64_t)g.gny * g.gnx * cblocks;
    for (int64_t it = blockIdx.x; it < items; it += PARTS) {
      const int bin = (int)(it / cblocks), cb = (int)(it % cblocks);
      const Block b = block_of(g, bin / g.gnx, bin % g.gnx);
      const double ng = (double)b.rows * (double)b.cols;
      pm_bin<XT>(x, g, b.y0, b.rows, b.x0, b.cols, cb * PM_C, cs, [&](int c, ST S) { take(c, S, ng); });
    }
  } else {
    const int64_t items = (int64_t)g.n * g.gny;
    for (int64_t it = blockIdx.x; it < items; it += PARTS) {
      const int c = (int)(it / g.gny), gy = (int)(it % g.gny);
      cm_bin_row<XT>(x + (int64_t)c * g.ld, g, gy, cs, take);
    }
  }
  block_reduce<2, 2>(v, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = v[0];
    part[PARTS + blockIdx.x] = v[1];
  }
}

// A candidate of pixel-major X with too few (bin, channel block) pairs to fill the device: every bin is cut into `splits` slabs of `rps`
// image rows, one workgroup each, whose sums go to sbuf[bin][slab][channel] as doubles (exact for counts: below 2^53) ...
template <typename XT>
__global__ __launch_bounds__(BT) void pm_slab_kernel(const XT* __restrict__ x, Geo g, int splits, int rps, double* __restrict__ sbuf) {
  using ST = typename Sum<XT>::T;
  __shared__ ST cs[BT];
  const int cblocks = (g.n + PM_C - 1) / PM_C;
  const int cb = blockIdx.x % cblocks, slab = blockIdx.x / cblocks, bin = slab / splits, sp = slab % splits;
  const Block b = block_of(g, bin / g.gnx, bin % g.gnx);
  const int r0 = min(b.rows, sp * rps), rn = min(rps, b.rows - r0);   // (the last slabs of a short bin may be empty: they write 0)
  double* so = sbuf + (int64_t)slab * g.n;
  pm_bin<XT>(x, g, b.y0 + r0, rn, b.x0, b.cols, cb * PM_C, cs, [&](int c, ST S) { so[c] = (double)S; });
}
// ... and are joined here: S_gc = the slabs in ascending order, then S^2 / n_g and S / n_g as in bin_sums_kernel
__global__ __launch_bounds__(BT) void pm_join_kernel(Geo g, int splits, const double* __restrict__ sbuf, double* __restrict__ part) {
  __shared__ double red[(BT / 64 + 1) * 2];
  double v[2] = {0.0, 0.0};
  const int64_t total = (int64_t)g.gny * g.gnx * g.n;
  for (int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x; e < total; e += (int64_t)PARTS * BT) {
    const int bin = (int)(e / g.n), c = (int)(e % g.n);
    const Block b = block_of(g, bin / g.gnx, bin % g.gnx);
    const double ng = (double)b.rows * (double)b.cols;
    double S = 0.0;
    for (int sp = 0; sp < splits; ++sp) S += sbuf[((int64_t)bin * splits + sp) * g.n + c];
    v[0] += S * S / ng;
    v[1] += S / ng;
  }
  block_reduce<2, 2>(v, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = v[0];
    part[PARTS + blockIdx.x] = v[1];
  }
}

// sum x and sum x^2 over the cube, seen as `rows` rows of `cols` entries ld apart: partials to part[0][wg], part[1][wg]
template <typename XT>
__global__ __launch_bounds__(BT) void totals_kernel(const XT* __restrict__ x, int64_t ld, int64_t rows, int64_t cols, double* __restrict__ part) {
  using ST = typename Sum<XT>::T;
  __shared__ double red[(BT / 64 + 1) * 2];
  constexpr int U = 8;
  const int64_t chunks = (cols + U * BT - 1) / (U * BT), items = rows * chunks;
  ST t1 = 0, t2 = 0;
  for (int64_t it = blockIdx.x; it < items; it += PARTS) {
    const int64_t row = it / chunks, q0 = (it % chunks) * (U * BT) + threadIdx.x;
    const XT* xr = x + row * ld;
    XT xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xv[u] = q0 + u * BT < cols ? xr[q0 + u * BT] : XT(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const ST e = (ST)xv[u];
      t1 += e;
      t2 += e * e;
    }
  }
  double v[2] = {(double)t1, (double)t2};
  block_reduce<2, 2>(v, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = v[0];
    part[PARTS + blockIdx.x] = v[1];
  }
}

// out[s] = the PARTS partials of slot s: a thread's in ascending order, then the workgroup's fixed order - one workgroup per slot
__global__ __launch_bounds__(BT) void slots_kernel(const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double red[BT / 64 + 1];
  const double* ps = part + (size_t)blockIdx.x * PARTS;
  double v[1] = {0.0};
  for (int i = threadIdx.x; i < PARTS; i += BT) v[0] += ps[i];
  block_reduce<1, 1>(v, red);
  if (threadIdx.x == 0) out[blockIdx.x] = v[0];
}

inline Geo geo(int64_t ld, int n, int ny, int nx, int by, int bx) {
  Geo g;
  g.ld = ld, g.n = n, g.ny = ny, g.nx = nx;
  g.by = by < ny ? by : ny, g.bx = bx < nx ? bx : nx;
  g.gny = (ny + g.by - 1) / g.by, g.gnx = (nx + g.bx - 1) / g.bx;
  return g;
}

template <typename XT, typename OT>
int launch_rebin(const void* x, int layout, const Geo& g, void* out, int64_t out_ld, hipStream_t s) {
  const XT* xt = static_cast<const XT*>(x);
  OT* ot = static_cast<OT*>(out);
  if (layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((rebin_kernel<XT, OT, true>), dim3((unsigned)(g.gny * g.gnx), (unsigned)((g.n + PM_C - 1) / PM_C)), dim3(BT), 0, s, xt,
                       g, ot, out_ld);
  else
    hipLaunchKernelGGL((rebin_kernel<XT, OT, false>), dim3((unsigned)((int64_t)g.n * g.gny)), dim3(BT), 0, s, xt, g, ot, out_ld);
  return check_hip(hipGetLastError(), "rebin launch");
}

// slabs per bin of a pixel-major candidate: 1 where its (bin, channel block) pairs already make PARTS work items, else what brings
// them there, at most one slab per image row of a bin; bins x slabs x channel blocks stays below 2 PARTS (the slab buffer's size)
inline int pm_splits(const Geo& g) {
  const int64_t pairs = (int64_t)g.gny * g.gnx * ((g.n + PM_C - 1) / PM_C);
  if (pairs >= PARTS) return 1;
  const int64_t want = (PARTS + pairs - 1) / pairs;
  return (int)(want < g.by ? want : g.by);
}
constexpr size_t SLAB_DOUBLES = (size_t)2 * PARTS * PM_C;

template <typename XT>
int launch_sums(const void* x, int layout, const Geo& g, double* part, double* sbuf, hipStream_t s) {
  const XT* xt = static_cast<const XT*>(x);
  const int splits = layout == ESPM_LAYOUT_PM ? pm_splits(g) : 1;
  if (splits > 1) {
    const int rps = (g.by + splits - 1) / splits, cblocks = (g.n + PM_C - 1) / PM_C;
    hipLaunchKernelGGL((pm_slab_kernel<XT>), dim3((unsigned)(g.gny * g.gnx * splits * cblocks)), dim3(BT), 0, s, xt, g, splits, rps, sbuf);
    if (int rc = check_hip(hipGetLastError(), "binning slabs launch")) return rc;
    hipLaunchKernelGGL(pm_join_kernel, dim3(PARTS), dim3(BT), 0, s, g, splits, sbuf, part);
  } else if (layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((bin_sums_kernel<XT, true>), dim3(PARTS), dim3(BT), 0, s, xt, g, part);
  else
    hipLaunchKernelGGL((bin_sums_kernel<XT, false>), dim3(PARTS), dim3(BT), 0, s, xt, g, part);
  return check_hip(hipGetLastError(), "binning sums launch");
}

template <typename XT>
int launch_totals(const void* x, int layout, int64_t ld, int n, int64_t p, double* part, hipStream_t s) {
  const bool pm = layout == ESPM_LAYOUT_PM;
  hipLaunchKernelGGL((totals_kernel<XT>), dim3(PARTS), dim3(BT), 0, s, static_cast<const XT*>(x), ld, pm ? p : (int64_t)n,
                     pm ? (int64_t)n : p, part);
  return check_hip(hipGetLastError(), "binning totals launch");
}

}  // namespace bink
#endif

}  // namespace espm

using namespace espm;

#if ESPM_KP == 8
// what both entry points ask of the image, before the device is touched
static int binning_check_image(const char* who, const void* x, int x_dtype, int x_layout, int64_t ld, int n, int ny, int nx) {
  ESPM_REQUIRE(x && n >= 1 && ny >= 1 && nx >= 1, "%s: bad arguments", who);
  ESPM_REQUIRE((int64_t)ny * nx < ((int64_t)1 << 31), "%s: %d x %d pixels (fewer than 2^31)", who, ny, nx);
  ESPM_REQUIRE(x_layout == ESPM_LAYOUT_CM || x_layout == ESPM_LAYOUT_PM, "%s: x_layout %d", who, x_layout);
  const int64_t row = x_layout == ESPM_LAYOUT_CM ? (int64_t)ny * nx : (int64_t)n;
  ESPM_REQUIRE(ld >= row, "%s: ld=%lld below the row length %lld", who, (long long)ld, (long long)row);
  ESPM_REQUIRE(x_dtype >= ESPM_DIAG_X_U8 && x_dtype <= ESPM_DIAG_X_F64, "%s: x_dtype %d", who, x_dtype);
  return ESPM_OK;
}
#endif

extern "C" int espm_rebin_pixels(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int ny, int nx, int by, int bx, void* out,
                                 int out_dtype, int64_t out_ld, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel binning: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (int rc = binning_check_image("rebin", x, x_dtype, x_layout, ld, n, ny, nx)) return rc;
  ESPM_REQUIRE(out, "rebin: bad arguments");
  ESPM_REQUIRE(by >= 1 && bx >= 1, "rebin: bin (%d, %d) (positive factors)", by, bx);
  ESPM_REQUIRE(out_dtype == ESPM_DIAG_X_F32 || out_dtype == ESPM_DIAG_X_F64, "rebin: out_dtype %d (f32 or f64)", out_dtype);
  const bink::Geo g = bink::geo(ld, n, ny, nx, by, bx);
  const int64_t bins = (int64_t)g.gny * g.gnx, orow = x_layout == ESPM_LAYOUT_CM ? bins : (int64_t)n;
  ESPM_REQUIRE(out_ld >= orow, "rebin: out_ld=%lld below the row length %lld", (long long)out_ld, (long long)orow);
  ESPM_REQUIRE((int64_t)n * g.gny < ((int64_t)1 << 31) && (n + bink::PM_C - 1) / bink::PM_C <= 65535,
               "rebin: %d channels x %d bin rows (fewer than 2^31 work items)", n, g.gny);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool f32 = out_dtype == ESPM_DIAG_X_F32;
  switch (x_dtype) {
#define ESPM_REBIN_CASE(CODE, XT) \
  case CODE: return f32 ? bink::launch_rebin<XT, float>(x, x_layout, g, out, out_ld, s) : bink::launch_rebin<XT, double>(x, x_layout, g, out, out_ld, s);
    ESPM_REBIN_CASE(ESPM_DIAG_X_U8, uint8_t)
    ESPM_REBIN_CASE(ESPM_DIAG_X_U16, uint16_t)
    ESPM_REBIN_CASE(ESPM_DIAG_X_F32, float)
    ESPM_REBIN_CASE(ESPM_DIAG_X_F64, double)
#undef ESPM_REBIN_CASE
  }
  return ESPM_OK;
#endif
}

extern "C" size_t espm_binning_sums_scratch(int n, int ny, int nx, int n_bins) {
#if ESPM_KP != 8
  (void)n; (void)ny; (void)nx; (void)n_bins;
  return 0;
#else
  if (n < 1 || ny < 1 || nx < 1 || n_bins < 1) return 0;
  return ((size_t)(2 + 2 * (size_t)n_bins) * ESPM_BIN_PARTS + bink::SLAB_DOUBLES) * sizeof(double);   // the slots, then the slab buffer
#endif
}

extern "C" int espm_binning_sums(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int ny, int nx, const int32_t* bins, int n_bins,
                                 double* out, void* scratch, size_t scratch_bytes, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "pixel binning: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (int rc = binning_check_image("binning sums", x, x_dtype, x_layout, ld, n, ny, nx)) return rc;
  ESPM_REQUIRE(out && scratch && bins, "binning sums: bad arguments");
  ESPM_REQUIRE(n_bins >= 1, "binning sums: n_bins=%d (at least one candidate)", n_bins);
  for (int i = 0; i < n_bins; ++i)
    ESPM_REQUIRE(bins[2 * i] >= 1 && bins[2 * i + 1] >= 1, "binning sums: bin %d is (%d, %d) (positive factors)", i, bins[2 * i], bins[2 * i + 1]);
  const size_t need = espm_binning_sums_scratch(n, ny, nx, n_bins);
  ESPM_REQUIRE(scratch_bytes >= need, "binning sums: scratch of %zu bytes, %zu needed (espm_binning_sums_scratch)", scratch_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(scratch);
  double* sbuf = part + (size_t)(2 + 2 * (size_t)n_bins) * ESPM_BIN_PARTS;
  const int64_t p = (int64_t)ny * nx;
  int rc = ESPM_OK;
#define ESPM_BIN_DTYPE(CALL)                               \
  switch (x_dtype) {                                       \
    case ESPM_DIAG_X_U8: { using XT = uint8_t; rc = CALL; break; }   \
    case ESPM_DIAG_X_U16: { using XT = uint16_t; rc = CALL; break; } \
    case ESPM_DIAG_X_F32: { using XT = float; rc = CALL; break; }    \
    default: { using XT = double; rc = CALL; break; }                \
  }
  ESPM_BIN_DTYPE(bink::launch_totals<XT>(x, x_layout, ld, n, p, part, s))
  if (rc) return rc;
  for (int i = 0; i < n_bins; ++i) {
    const bink::Geo g = bink::geo(ld, n, ny, nx, bins[2 * i], bins[2 * i + 1]);
    double* pi = part + (size_t)(2 + 2 * i) * ESPM_BIN_PARTS;
    ESPM_BIN_DTYPE(bink::launch_sums<XT>(x, x_layout, g, pi, sbuf, s))
    if (rc) return rc;
  }
#undef ESPM_BIN_DTYPE
  hipLaunchKernelGGL(bink::slots_kernel, dim3((unsigned)(2 + 2 * n_bins)), dim3(bink::BT), 0, s, part, out);
  return check_hip(hipGetLastError(), "binning sums reduction");
#endif
}
