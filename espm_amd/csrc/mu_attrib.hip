// Count attribution (include/espm_mu.h, "count attribution"): how many of the MEASURED counts stand behind every component of a fitted
// model d h - in expectation (the EM responsibilities, the numerator of the multiplicative update) and as a random split of the image
// into k integer images that add up to it exactly (the Poisson splitting theorem).
//
// Every kernel here has the same shape (mu_image_pass.hpp's walk).  X is a matrix whose rows are ld apart; the index that runs along a
// row is the LANE index (a thread owns one), the index that runs across the rows is the WALK index (a thread walks it).  Channel-major
// X: lane = pixel, walk = channel; pixel-major X: lane = channel, walk = pixel.  A thread keeps its lane's k-vector in registers
// (h[:, pixel], or d[channel, :]); the k-vectors of the walk go through LDS (stage) and are read back as broadcasts.  The model's value
// y = sum_i d_i h_i of an entry is the same expression whichever of the two vectors is whose, so both layouts compute the same bits.
//
//   expected_kernel  what a lane gathers over its walk: acc_i = sum_walk (x / Y) g_i, g the walk's vector, Y = max(y, log_shift); an
//                entry with x == 0 costs its read only.
//                  pixel side (lane = pixel, the whole walk in one thread, channels ascending): num_h = h acc, and counts = sum x
//                  channel side (lane = channel, ESPM_ATTRIB_PCHUNK pixels per workgroup, pixels ascending): the partial sums of
//                  ratio go to scratch[chunk][component][channel]; reduce_kernel adds the chunks in ascending order
//                channel-major X serves the pixel side directly and the channel side through an LDS tile that is filled along the
//                rows and read back transposed; pixel-major X the other way round.  Two passes over X - one per side - instead of one
//                that serves both: one pass would have to add k values per entry across the lanes of a workgroup.
//   assign_kernel    the rule of the header, entry by entry: the k cumulative rates without fused multiply-adds, their running maximum
//                m_i = max_{j <= i} s_j, and per count one Philox word w and t = (w 2^-32) a: "the smallest i with t < s_i" is at most
//                i exactly when t < m_i, so cum_i = #{counts : t < m_i} and the parts are the differences of cum (the last one x - cum).
//                An entry of ESPM_ATTRIB_HEAVY counts or more is drawn by its whole wave: mu_image_pass.hpp's for_each_heavy, with
//                a and m broadcast beside x and e and k - 1 counters summed.  The loop is WRITTEN OUT in assign_entry: through the
//                header's driver and a callable the widest 16-bit instance took two more vector and two more accumulation registers.
//
// No value is accumulated atomically.  The number of invalid entries of espm_assign_counts is a sum of integers (block_count_add, onto
// the zeroed counter).  Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry points as stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace attribk {

constexpr int BT = ESPM_ATTRIB_BLOCK;
constexpr int PC = ESPM_ATTRIB_PCHUNK;
constexpr int WALK = ESPM_ATTRIB_WALK;
constexpr uint32_t HEAVY = ESPM_ATTRIB_HEAVY;
constexpr int TP = BT + 1;   // lane stride of the transposing tile
static_assert(BT == 256, "four waves of 64 lanes");

static_assert(WALK % 256 == 0 && PC % 256 == 0, "whole rounds of the staged vectors");

struct Vec : espm::Vec {};   // the kernels' parameter type (its name is part of their symbols): the header's

// ---- expected attribution ---------------------------------------------------------------------------------------------------------
// PIXEL_SIDE: lane = pixel, grid (lane blocks), the whole walk; out = num_h (cs apart), scaled by the lane's vector; counts written.
// otherwise:  lane = channel, grid (pixel chunks, lane blocks); out = scratch + chunk * out_chunk, unscaled.
// TILE: the lane index runs across the rows of x (x[lane * ld + walk]) and x goes through the transposing tile.
template <int KP, typename XT, bool PIXEL_SIDE, bool TILE>
__global__ __launch_bounds__(BT) void expected_kernel(const XT* __restrict__ x, int64_t ld, int lanes, int walks, Vec lv, Vec wv, int k,
                                                      double log_shift, double* __restrict__ out, int64_t out_cs, int64_t out_chunk,
                                                      void* __restrict__ counts) {
  using CT = typename std::conditional<std::is_integral<XT>::value, int64_t, double>::type;
  constexpr int CH = stage_rows<KP>();
  __shared__ double ds[CH * KP];
  const int64_t l0 = (int64_t)(PIXEL_SIDE ? blockIdx.x : blockIdx.y) * BT;
  const int64_t l = l0 + threadIdx.x;
  const bool valid = l < lanes;
  const int64_t w_begin = PIXEL_SIDE ? 0 : (int64_t)blockIdx.x * PC;
  const int64_t w_end = PIXEL_SIDE ? (int64_t)walks : (w_begin + PC < walks ? w_begin + PC : (int64_t)walks);
  double a[KP], acc[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    a[j] = valid && j < k ? lv.ptr[(int64_t)j * lv.cs + l * lv.qs] : 0.0;
    acc[j] = 0.0;
  }
  CT cnt = 0;

  auto add = [&](XT xv, const double* __restrict__ g) {
    if (xv != XT(0)) {
      double y = 0.0;
#pragma unroll
      for (int j = 0; j < KP; ++j) y = fma(a[j], g[j], y);
      y = fmax(y, log_shift);
      const double w = (double)xv / y;
#pragma unroll
      for (int j = 0; j < KP; ++j) acc[j] = fma(w, g[j], acc[j]);
      cnt += (CT)xv;
    }
  };

  for (int64_t c0 = w_begin; c0 < w_end; c0 += CH) {
    const int cn = (int)(w_end - c0 < CH ? w_end - c0 : CH);
    __syncthreads();
    stage<KP, BT>(ds, wv, c0, cn, k);
    __syncthreads();
    if constexpr (!TILE) {
      const XT* xp = x + c0 * ld + l;
      for (int c = 0; c < cn; c += 8) {
        XT xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = (valid && c + u < cn) ? xp[(int64_t)(c + u) * ld] : XT(0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (c + u < cn) add(xv[u], ds + (c + u) * KP);
      }
    } else {
      constexpr int TS = tile_rows<XT>();
      __shared__ XT tile[TS * TP];
      for (int t0 = 0; t0 < cn; t0 += TS) {
        const int tn = cn - t0 < TS ? cn - t0 : TS;
        __syncthreads();   // (the tile's readers of the round before)
        fill_tile<XT, BT>(tile, x, ld, l0, lanes, c0 + t0, tn);
        __syncthreads();
        for (int c = 0; c < tn; ++c) add(valid ? tile[c * TP + threadIdx.x] : XT(0), ds + (t0 + c) * KP);
      }
    }
  }
  if (valid) {
    double* o = out + (PIXEL_SIDE ? 0 : (int64_t)blockIdx.x * out_chunk) + l;
#pragma unroll
    for (int j = 0; j < KP; ++j)
      if (j < k) o[(int64_t)j * out_cs] = PIXEL_SIDE ? a[j] * acc[j] : acc[j];
    if (PIXEL_SIDE) static_cast<CT*>(counts)[l] = cnt;
  }
}

// the chunks of every (component, channel) added in ascending order: the one order there is, whatever the grid did
__global__ __launch_bounds__(256) void reduce_kernel(const double* __restrict__ part, int n, int k, int n_chunks, double* __restrict__ ratio) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)k * n) return;
  const int j = (int)(i / n), c = (int)(i % n);
  double v = 0.0;
  for (int q = 0; q < n_chunks; ++q) v += part[((int64_t)q * k + j) * n + c];
  ratio[(int64_t)c * k + j] = v;
}

template <int KP, typename XT>
int launch_expected(const void* x, int layout, int64_t ld, int n, int p, const double* d, const double* h, int k, double log_shift, double* num_h,
                    void* counts, double* part, hipStream_t s) {
  const XT* xt = static_cast<const XT*>(x);
  const Vec hv = {h, (int64_t)p, 1}, dv = {d, 1, (int64_t)k};
  const dim3 block(BT);
  const dim3 pgrid((unsigned)(((int64_t)p + BT - 1) / BT));
  const dim3 cgrid((unsigned)(((int64_t)p + PC - 1) / PC), (unsigned)((n + BT - 1) / BT));
  const int64_t chunk = (int64_t)k * n;
  if (layout == ESPM_LAYOUT_CM) {
    hipLaunchKernelGGL((expected_kernel<KP, XT, true, false>), pgrid, block, 0, s, xt, ld, p, n, hv, dv, k, log_shift, num_h, (int64_t)p, (int64_t)0,
                       counts);
    hipLaunchKernelGGL((expected_kernel<KP, XT, false, true>), cgrid, block, 0, s, xt, ld, n, p, dv, hv, k, log_shift, part, (int64_t)n, chunk,
                       (void*)nullptr);
  } else {
    hipLaunchKernelGGL((expected_kernel<KP, XT, true, true>), pgrid, block, 0, s, xt, ld, p, n, hv, dv, k, log_shift, num_h, (int64_t)p, (int64_t)0,
                       counts);
    hipLaunchKernelGGL((expected_kernel<KP, XT, false, false>), cgrid, block, 0, s, xt, ld, n, p, dv, hv, k, log_shift, part, (int64_t)n, chunk,
                       (void*)nullptr);
  }
  return check_hip(hipGetLastError(), "expected attribution launch");
}

// ---- random attribution -----------------------------------------------------------------------------------------------------------
struct Rule {
  uint32_t key0, key1;
};

// the cumulative rates of one entry as their running maximum m_i = max_{j <= i} s_j, and a = s_{k - 1}: products and sums rounded one
// by one, components in ascending order (a contraction to a fused multiply-add would change the bits the rule is defined by)
template <int KP>
__device__ __forceinline__ double cuts(const double (&v)[KP], const double* __restrict__ g, int k, double (&m)[KP]) {
#pragma clang fp contract(off)
  double s = 0.0, top = 0.0, a = 0.0;
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    if (i < k) {   // (uniform)
      const double t = g[i] * v[i];
      s = i == 0 ? t : s + t;
      top = i == 0 ? s : fmax(top, s);
      a = s;
    }
    m[i] = top;
  }
  return a;
}

// cum_i += #{draws 4 b .. min(4 b + 3, x - 1) of element e with t < m_i}, i < k - 1 (4 b < x)
template <int KP>
__device__ __forceinline__ void block_of_four(uint32_t x, uint64_t e, uint32_t b, const Rule& r, const double (&m)[KP], double a, int k,
                                              uint32_t (&cum)[KP]) {
#pragma clang fp contract(off)
  uint32_t w[4];
  philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), 0x80000000u | b, 0u, r.key0, r.key1, w);
  const uint32_t left = x - 4u * b;   // draws from this block on: at least 1
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) {
    if (d < left) {
      const double u = (double)w[d] * 2.3283064365386963e-10;   // w 2^-32: exact
      const double t = u * a;
#pragma unroll
      for (int i = 0; i < KP - 1; ++i)
        if (i < k - 1) cum[i] += (uint32_t)(t < m[i]);
    }
  }
}

// the k parts of one entry per lane.  EVERY lane of the wave calls this together (a lane without an entry passes x = 0): the heavy
// entries of a 16-bit image are drawn by the whole wave.  Returns whether the entry is invalid.
template <int KP, typename XT>
__device__ __forceinline__ bool assign_entry(uint32_t x, uint64_t e, const Rule& r, const double (&v)[KP], const double* __restrict__ g, int k,
                                             uint32_t (&cnt)[KP]) {
  double m[KP];
  double a = 0.0;
  uint32_t cum[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) m[i] = 0.0, cum[i] = 0u;
  if (x) a = cuts<KP>(v, g, k, m);
  const bool ok = a > 0.0 && a <= 1.7976931348623157e308;   // finite and above 0
  const bool heavy = sizeof(XT) > 1 && x >= HEAVY && ok;
  if (x && ok && !heavy)
    for (uint32_t b = 0; 4u * b < x; ++b) block_of_four<KP>(x, e, b, r, m, a, k, cum);
  if constexpr (sizeof(XT) > 1) {   // (for_each_heavy's loop, written out: the file comment)
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(heavy);
    while (todo) {   // (wave-uniform)
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t xh = (uint32_t)__shfl((int)x, src, 64);
      const uint64_t eh = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(e >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)e, src, 64);
      const double ah = __shfl(a, src, 64);
      double mh[KP];
      uint32_t mine[KP];
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        mh[i] = i < k - 1 ? __shfl(m[i], src, 64) : 0.0;
        mine[i] = 0u;
      }
      for (uint32_t b = (uint32_t)lane; 4u * b < xh; b += 64u) block_of_four<KP>(xh, eh, b, r, mh, ah, k, mine);
#pragma unroll
      for (int i = 0; i < KP - 1; ++i)
        if (i < k - 1) {
          const uint32_t total = wave_sum_u32(mine[i]);
          if (lane == src) cum[i] = total;
        }
    }
  }
  // cum_i counts the draws that went to a component <= i; an invalid entry gives everything to component 0
  uint32_t prev = 0;
#pragma unroll
  for (int i = 0; i < KP; ++i) {
    const uint32_t upto = !ok || i >= k - 1 ? x : cum[i];
    cnt[i] = upto - prev;
    prev = upto;
  }
  return x && !ok;
}

// lane blocks on grid.x and walk chunks on grid.y for channel-major X, the other way round for pixel-major X (the long axis on x)
template <int KP, typename XT>
__global__ __launch_bounds__(BT) void assign_kernel(const XT* __restrict__ x, int64_t ld, int lanes, int walks, int pm, int64_t p_total, int64_t j0,
                                                    Rule rule, Vec lv, Vec wv, int k, XT* __restrict__ parts, int64_t part_stride, int64_t out_ld,
                                                    unsigned long long* __restrict__ counts) {
  constexpr int CH = stage_rows<KP>();
  __shared__ double ds[CH * KP];
  __shared__ uint32_t part_inv[1][BT / 64];
  const int64_t l = (int64_t)(pm ? blockIdx.y : blockIdx.x) * BT + threadIdx.x;
  const bool valid = l < lanes;
  const int64_t w_begin = (int64_t)(pm ? blockIdx.x : blockIdx.y) * WALK;
  const int64_t w_end = w_begin + WALK < walks ? w_begin + WALK : (int64_t)walks;
  double v[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) v[j] = valid && j < k ? lv.ptr[(int64_t)j * lv.cs + l * lv.qs] : 0.0;
  // e = c p_total + j0 + pixel: the lane's share and the walk's step
  const uint64_t e_lane = pm ? (uint64_t)l * (uint64_t)p_total + (uint64_t)j0 : (uint64_t)j0 + (uint64_t)l;
  const uint64_t e_step = pm ? 1ull : (uint64_t)p_total;
  uint32_t n_inv = 0;

  for (int64_t c0 = w_begin; c0 < w_end; c0 += CH) {
    const int cn = (int)(w_end - c0 < CH ? w_end - c0 : CH);
    __syncthreads();
    stage<KP, BT>(ds, wv, c0, cn, k);
    __syncthreads();
    const XT* xp = x + c0 * ld + l;
    XT* op = parts + c0 * out_ld + l;
    for (int c = 0; c < cn; c += 4) {
      XT xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = (valid && c + u < cn) ? xp[(int64_t)(c + u) * ld] : XT(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c + u < cn) {   // (uniform: every lane of the wave goes through assign_entry)
          uint32_t cnt[KP];
          const bool inv = assign_entry<KP, XT>((uint32_t)xv[u], e_lane + (uint64_t)(c0 + c + u) * e_step, rule, v, ds + (c + u) * KP, k, cnt);
          n_inv += (uint32_t)inv;
          if (valid) {
#pragma unroll
            for (int i = 0; i < KP; ++i)
              if (i < k) op[(int64_t)i * part_stride + (int64_t)(c + u) * out_ld] = (XT)cnt[i];
          }
        }
      }
    }
  }
  block_count_add<1>(part_inv, {n_inv}, counts);
}

template <int KP, typename XT>
int launch_assign(const void* x, int layout, int64_t ld, int n, int p, int64_t p_total, int64_t j0, const Rule& rule, const double* d, const double* h,
                  int k, void* parts, int64_t part_stride, int64_t out_ld, int64_t* counts, hipStream_t s) {
  const bool pm = layout == ESPM_LAYOUT_PM;
  const Vec hv = {h, (int64_t)p, 1}, dv = {d, 1, (int64_t)k};
  const int lanes = pm ? n : p, walks = pm ? p : n;
  const unsigned lane_blocks = (unsigned)(((int64_t)lanes + BT - 1) / BT), chunks = (unsigned)(((int64_t)walks + WALK - 1) / WALK);
  const dim3 grid(pm ? chunks : lane_blocks, pm ? lane_blocks : chunks), block(BT);
  hipLaunchKernelGGL((assign_kernel<KP, XT>), grid, block, 0, s, static_cast<const XT*>(x), ld, lanes, walks, (int)pm, p_total, j0, rule,
                     pm ? dv : hv, pm ? hv : dv, k, static_cast<XT*>(parts), part_stride, out_ld, reinterpret_cast<unsigned long long*>(counts));
  return check_hip(hipGetLastError(), "count assignment launch");
}

}  // namespace attribk
#endif

}  // namespace espm

using namespace espm;

#if ESPM_KP == 8
// what both entry points ask of the image and the model, before the device is touched
static int attrib_check(const char* who, const void* x, int x_dtype, int max_dtype, int x_layout, int64_t ld, int n, int p, const double* d,
                        const double* h, int k) {
  ESPM_REQUIRE(x && d && h, "%s: bad arguments (x %p, d %p, h %p)", who, x, (const void*)d, (const void*)h);
  ESPM_REQUIRE(n >= 1 && p >= 1, "%s: bad arguments (n=%d, p=%d)", who, n, p);
  ESPM_REQUIRE(k >= 1 && k <= ESPM_ATTRIB_MAX_K, "%s: k=%d (1..%d components)", who, k, ESPM_ATTRIB_MAX_K);
  if (int rc = check_image(who, x, x_dtype, max_dtype, x_layout, ld, n, p)) return rc;
  ESPM_REQUIRE((n + ESPM_ATTRIB_BLOCK - 1) / ESPM_ATTRIB_BLOCK <= 65535, "%s: n=%d (at most %d channels)", who, n, 65535 * ESPM_ATTRIB_BLOCK);
  return ESPM_OK;
}
#endif

extern "C" size_t espm_attribute_expected_scratch(int n, int p, int k) {
#if ESPM_KP != 8
  (void)n; (void)p; (void)k;
  return 0;
#else
  if (n < 1 || p < 1 || k < 1 || k > ESPM_ATTRIB_MAX_K) return 0;
  const size_t chunks = (size_t)(((int64_t)p + ESPM_ATTRIB_PCHUNK - 1) / ESPM_ATTRIB_PCHUNK);
  return chunks * (size_t)k * (size_t)n * sizeof(double);
#endif
}

extern "C" int espm_attribute_expected(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int k,
                                       double log_shift, double* num_h, double* ratio, void* counts, void* scratch, size_t scratch_bytes,
                                       espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "count attribution: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (int rc = attrib_check("expected attribution", x, x_dtype, ESPM_DIAG_X_F64, x_layout, ld, n, p, d, h, k)) return rc;
  ESPM_REQUIRE(num_h && ratio && counts && scratch, "expected attribution: bad arguments (num_h %p, ratio %p, counts %p, scratch %p)", (void*)num_h,
               (void*)ratio, counts, scratch);
  ESPM_REQUIRE(log_shift > 0, "expected attribution: log_shift=%g must be positive", log_shift);
  const size_t need = espm_attribute_expected_scratch(n, p, k);
  ESPM_REQUIRE(scratch_bytes >= need, "expected attribution: scratch of %zu bytes, %zu needed (espm_attribute_expected_scratch)", scratch_bytes,
               need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(scratch);
  const int rc = dispatch_kp(k, [&](auto kp) {
    return dispatch_xt<ESPM_DIAG_X_F64>(x_dtype, [&](auto xt) {
      return attribk::launch_expected<decltype(kp)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, d, h, k, log_shift, num_h, counts,
                                                                                         part, s);
    });
  });
  if (rc) return rc;
  const int n_chunks = (int)(((int64_t)p + ESPM_ATTRIB_PCHUNK - 1) / ESPM_ATTRIB_PCHUNK);
  const unsigned blocks = (unsigned)(((int64_t)k * n + 255) / 256);
  hipLaunchKernelGGL(attribk::reduce_kernel, dim3(blocks), dim3(256), 0, s, part, n, k, n_chunks, ratio);
  return check_hip(hipGetLastError(), "expected attribution reduction");
#endif
}

extern "C" int espm_assign_counts(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int64_t p_total, int64_t j0, const double* d,
                                  const double* h, int k, uint64_t seed, void* parts, int64_t part_stride, int64_t out_ld, int64_t* counts,
                                  espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "count attribution: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (int rc = attrib_check("assign counts", x, x_dtype, ESPM_DIAG_X_U16, x_layout, ld, n, p, d, h, k)) return rc;
  ESPM_REQUIRE(parts && counts, "assign counts: bad arguments (parts %p, counts %p)", parts, (void*)counts);
  const int row = x_layout == ESPM_LAYOUT_CM ? p : n, rows = x_layout == ESPM_LAYOUT_CM ? n : p;
  ESPM_REQUIRE(out_ld >= row, "assign counts: out_ld=%lld below the row length %d", (long long)out_ld, row);
  ESPM_REQUIRE(out_ld <= (INT64_MAX - row) / rows && part_stride >= (int64_t)(rows - 1) * out_ld + row,
               "assign counts: part_stride=%lld below one image (%d rows, out_ld=%lld apart)", (long long)part_stride, rows, (long long)out_ld);
  if (int rc = check_slab("assign counts", n, p, p_total, j0)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  attribk::Rule rule;
  rule.key0 = (uint32_t)seed, rule.key1 = (uint32_t)(seed >> 32);
  if (int rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t), s), "assign counts: zeroing the counter")) return rc;
  return dispatch_kp(k, [&](auto kp) {
    return dispatch_xt<ESPM_DIAG_X_U16>(x_dtype, [&](auto xt) {
      return attribk::launch_assign<decltype(kp)::value, typename decltype(xt)::type>(x, x_layout, ld, n, p, p_total, j0, rule, d, h, k, parts,
                                                                                       part_stride, out_ld, counts, s);
    });
  });
#endif
}
