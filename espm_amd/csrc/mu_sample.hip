// Parametric bootstrap (include/espm_mu.h, "Poisson sampling"): a count image drawn from a model d h on the device, and the deviance of
// such draws against the model that generated them, without storing them.
//
// The rule (the header has it in full).  Element (c, j) of the logical (n, p_total) channel-major image has the index e = c p_total + j.
// Its rate y = sum_i d[c, i] h[i, j] is formed in fp64 with every product and every sum rounded on its own (no fused multiply-add), so
// that a host loop gets the same bits.  m = floor(y), thr = floor((y - m) 2^32).  Block b of the element's random words is
// Philox4x32-10(counter = (e low, e high, b, replicate + 1), key = (seed low, seed high)).  N(w) = #{i < 12 : w >= T_i} turns a word into
// a Poisson(1) draw.  x = sum_{i < m} N(word i mod 4 of block 4 + i div 4) + #{i in 1 .. N(word 0 of block 0) : word i mod 4 of block
// i div 4 < thr}: m unit pieces and a Poisson(1) thinned to the fractional part.
//
//   sample_kernel:   a pixel per thread over mu_image_pass.hpp's walk (d staged padded to KP: a padded product is an exact +0 and y + 0
//                is y), pixel-major output through the tile, written where the other passes read it.
//   heavy entries (m >= ESPM_SAMPLE_HEAVY): the wave shares the unit pieces (for_each_heavy), lane l the blocks 4 + l, 4 + l + 64, ...
//   deviance_kernel: the same walk for replicate blockIdx.y (and every gridDim.y-th after it); each entry's x is drawn and its term
//                x ln(x / Y) - x + Y added in channel order in the pixel's own thread: two calls give the same bits.
//
// The sample values use no atomics.  The two counters of espm_poisson_sample are sums of integers (block_count_add, onto the zeroed
// pair).  Only the narrow build (ESPM_KP == 8) instantiates the kernels; the wide builds export the entry points as stubs.
#include <type_traits>

#include "mu_common.hpp"

namespace espm {

#if ESPM_KP == 8
#include "mu_image_pass.hpp"

namespace samplek {

constexpr int BT = ESPM_SAMPLE_BLOCK;
constexpr uint32_t HEAVY = ESPM_SAMPLE_HEAVY;
constexpr double MAX_RATE = (double)ESPM_SAMPLE_MAX_RATE;
static_assert(BT == 256, "four waves of 64 lanes");

// T_i = floor(2^32 sum_{j <= i} e^-1 / j!), i = 0 .. 11 (include/espm_mu.h)
constexpr uint32_t T0 = 0x5e2d58d8u, T1 = 0xbc5ab1b1u, T2 = 0xeb715e1du, T3 = 0xfb239797u, T4 = 0xff1025f5u, T5 = 0xffd90f3bu,
                   T6 = 0xfffa8b71u, T7 = 0xffff540cu, T8 = 0xffffed1fu, T9 = 0xfffffe21u, T10 = 0xffffffd4u, T11 = 0xfffffffcu;

struct Rule {
  uint32_t key0, key1, rep1;   // seed low, seed high, replicate + 1
};

__device__ __forceinline__ void block(uint64_t e, uint32_t b, const Rule& r, uint32_t (&w)[4]) {
  philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), b, r.rep1, r.key0, r.key1, w);
}

// N(w): a word as a Poisson(1) draw.  A word reaches T6 once in 12000: the last six comparisons stay behind a branch.
__device__ __forceinline__ uint32_t unit(uint32_t w) {
  uint32_t n = (uint32_t)(w >= T0) + (uint32_t)(w >= T1) + (uint32_t)(w >= T2) + (uint32_t)(w >= T3) + (uint32_t)(w >= T4) + (uint32_t)(w >= T5);
  if (w >= T6)
    n += 1u + (uint32_t)(w >= T7) + (uint32_t)(w >= T8) + (uint32_t)(w >= T9) + (uint32_t)(w >= T10) + (uint32_t)(w >= T11);
  return n;
}

// the unit pieces 4 b .. min(4 b + 3, m - 1) of element e (4 b < m): the words of block 4 + b
__device__ __forceinline__ uint32_t unit_block(uint32_t m, uint64_t e, uint32_t b, const Rule& r) {
  uint32_t w[4];
  block(e, 4u + b, r, w);
  const uint32_t left = m - 4u * b;   // pieces from this block on: at least 1
  uint32_t s = unit(w[0]);
  if (left > 1) s += unit(w[1]);
  if (left > 2) s += unit(w[2]);
  if (left > 3) s += unit(w[3]);
  return s;
}

// the fractional part: N0 = N(word 0 of block 0) counts, count i = 1 .. N0 kept iff word i mod 4 of block i div 4 < thr (N0 <= 12: blocks 0 .. 3)
__device__ __forceinline__ uint32_t remainder(uint32_t thr, uint64_t e, const Rule& r) {
  uint32_t w[4];
  block(e, 0u, r, w);
  const uint32_t n0 = unit(w[0]);
  uint32_t s = (uint32_t)(n0 >= 1 && w[1] < thr) + (uint32_t)(n0 >= 2 && w[2] < thr) + (uint32_t)(n0 >= 3 && w[3] < thr);
  for (uint32_t b = 1; 4u * b <= n0; ++b) {   // (one word in 53 asks for block 1)
    block(e, b, r, w);
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) s += (uint32_t)(4u * b + t <= n0 && w[t] < thr);
  }
  return s;
}

// one entry per lane, classified: m unit pieces and the threshold of the fractional part (both 0 where nothing is drawn)
struct Entry {
  uint32_t m, thr;
  bool invalid, saturated;
};

__device__ __forceinline__ Entry classify(double y) {
  Entry en;
  en.invalid = !(y >= 0.0 && y <= 1.7976931348623157e308);   // negative, NaN or infinite
  en.saturated = !en.invalid && y > MAX_RATE;
  en.m = en.invalid || en.saturated ? 0u : (uint32_t)y;           // (y >= 0: the conversion truncates to floor(y))
  en.thr = en.invalid || en.saturated ? 0u : (uint32_t)((y - (double)en.m) * 4294967296.0);   // (both operations exact)
  return en;
}

// x of one entry per lane.  EVERY lane of the wave calls this together (a lane without an entry passes m = thr = 0): the heavy entries
// are drawn by the whole wave.
__device__ __forceinline__ uint32_t draw(uint32_t m, uint32_t thr, uint64_t e, const Rule& r) {
  uint32_t x = 0;
  const bool heavy = m >= HEAVY;
  if (thr) x = remainder(thr, e, r);   // (thr == 0: no count of the fractional part is kept, whatever the words)
  if (m && !heavy)
    for (uint32_t b = 0; 4u * b < m; ++b) x += unit_block(m, e, b, r);
  for_each_heavy(heavy, m, e, [&](int src, uint32_t mh, uint64_t eh) {
    const uint32_t total = wave_blocks_sum(mh, [&](uint32_t b) { return unit_block(mh, eh, b, r); });
    if ((int)(threadIdx.x & 63) == src) x += total;
  });
  return x;
}

// the rate of one entry: products and sums rounded one by one, components in ascending order (a contraction to a fused multiply-add
// would change the bits the rule is defined by)
template <int KP>
__device__ __forceinline__ double rate(const double (&h)[KP], const double* __restrict__ g) {
#pragma clang fp contract(off)
  double y = 0.0;
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const double t = g[j] * h[j];
    y = y + t;
  }
  return y;
}

template <int KP, typename XT, bool PM>
__global__ __launch_bounds__(BT) void sample_kernel(const double* __restrict__ d, const double* __restrict__ h, int k, int n, int p, int64_t p_total,
                                                    int64_t j0, Rule rule, XT* __restrict__ x, int64_t ld, unsigned long long* __restrict__ counts) {
  constexpr int CH = stage_rows<KP>();   // channels of d per round
  constexpr uint32_t XMAX = sizeof(XT) == 1 ? 255u : 65535u;
  __shared__ double ds[CH * KP];
  __shared__ uint32_t part[2][BT / 64];
  const int64_t q0 = (int64_t)blockIdx.x * BT;
  const int64_t q = q0 + threadIdx.x;
  const bool valid = q < p;
  double hq[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) hq[j] = valid && j < k ? h[(size_t)j * p + q] : 0.0;
  const uint64_t ej = (uint64_t)(j0 + q);
  const Vec dv = {d, 1, (int64_t)(uint32_t)k};   // (k >= 1: the entry point checked it)
  uint32_t n_sat = 0, n_inv = 0;

  // one entry: its value as stored (every lane of the wave comes here together)
  auto entry = [&](int c, const double* g) -> XT {
    const Entry en = classify(rate<KP>(hq, g));
    const uint32_t xe = draw(valid ? en.m : 0u, valid ? en.thr : 0u, (uint64_t)c * (uint64_t)p_total + ej, rule);
    const bool sat = en.saturated || xe > XMAX;
    if (valid) n_sat += (uint32_t)sat, n_inv += (uint32_t)en.invalid;
    return (XT)(sat ? XMAX : xe);   // (an invalid entry drew nothing: 0)
  };

  for (int c0 = 0; c0 < n; c0 += CH) {
    const int cn = min(CH, n - c0);
    __syncthreads();
    stage<KP, BT>(ds, dv, c0, cn, k);
    __syncthreads();
    if constexpr (!PM) {
      XT* xp = x + (size_t)c0 * ld + q;
      for (int c = 0; c < cn; ++c) {
        const XT v = entry(c0 + c, ds + c * KP);
        if (valid) xp[(size_t)c * ld] = v;
      }
    } else {
      constexpr int TS = tile_rows<XT>();
      __shared__ XT tile[TS * (BT + 1)];
      for (int t0 = 0; t0 < cn; t0 += TS) {
        const int tn = min(TS, cn - t0);
        __syncthreads();   // (the tile's readers of the round before)
        for (int c = 0; c < tn; ++c) tile[c * (BT + 1) + threadIdx.x] = entry(c0 + t0 + c, ds + (t0 + c) * KP);
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < TS; ++i) {   // (fill_tile's pass, storing)
          int px, c;
          const int at = tile_slot<XT, BT>(i, px, c);
          if (q0 + px < p && c < tn) x[(size_t)(q0 + px) * ld + (c0 + t0 + c)] = tile[at];
        }
      }
    }
  }
  block_count_add<2>(part, {n_sat, n_inv}, counts);
}

template <int KP>
__global__ __launch_bounds__(BT) void deviance_kernel(const double* __restrict__ d, const double* __restrict__ h, int k, int n, int p, int64_t p_total,
                                                      int64_t j0, Rule rule, int n_rep, double log_shift, double* __restrict__ dev) {
  constexpr int CH = stage_rows<KP>();
  __shared__ double ds[CH * KP];
  const int64_t q = (int64_t)blockIdx.x * BT + threadIdx.x;
  const bool valid = q < p;
  double hq[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) hq[j] = valid && j < k ? h[(size_t)j * p + q] : 0.0;
  const uint64_t ej = (uint64_t)(j0 + q);
  const Vec dv = {d, 1, (int64_t)(uint32_t)k};   // (k >= 1: the entry point checked it)
  const uint32_t rep1 = rule.rep1;   // (replicate0 + 1)

  for (int rep = blockIdx.y; rep < n_rep; rep += gridDim.y) {   // (uniform over the workgroup)
    rule.rep1 = rep1 + (uint32_t)rep;
    double acc = 0.0;
    for (int c0 = 0; c0 < n; c0 += CH) {
      const int cn = min(CH, n - c0);
      __syncthreads();
      stage<KP, BT>(ds, dv, c0, cn, k);
      __syncthreads();
      for (int c = 0; c < cn; ++c) {   // (every lane walks: draw is the wave's)
        const double y = rate<KP>(hq, ds + c * KP);
        const Entry en = classify(y);
        uint32_t xe = draw(valid ? en.m : 0u, valid ? en.thr : 0u, (uint64_t)(c0 + c) * (uint64_t)p_total + ej, rule);
        if (en.saturated || xe > 65535u) xe = 65535u;   // (what the sampler stores at 16 bits; an invalid entry: 0)
        const double yy = y < log_shift ? log_shift : y;   // (a NaN rate stays NaN: it shows in the pixel's deviance)
        const double fx = (double)xe;
        double t = yy - fx;
        if (xe) t = fma(fx, log(fx / yy), t);
        acc += t;
      }
    }
    if (valid) dev[(size_t)rep * p + q] = 2.0 * acc;
  }
}

template <int KP, typename XT>
int launch_sample(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, const Rule& rule, void* x, int layout,
                  int64_t ld, int64_t* counts, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + BT - 1) / BT)), block(BT);
  XT* xt = static_cast<XT*>(x);
  unsigned long long* ct = reinterpret_cast<unsigned long long*>(counts);
  if (layout == ESPM_LAYOUT_PM)
    hipLaunchKernelGGL((sample_kernel<KP, XT, true>), grid, block, 0, s, d, h, k, n, p, p_total, j0, rule, xt, ld, ct);
  else
    hipLaunchKernelGGL((sample_kernel<KP, XT, false>), grid, block, 0, s, d, h, k, n, p, p_total, j0, rule, xt, ld, ct);
  return check_hip(hipGetLastError(), "poisson sample launch");
}

template <int KP>
int launch_deviance(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, const Rule& rule, int n_rep,
                    double log_shift, double* dev, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p + BT - 1) / BT), (unsigned)(n_rep < 65535 ? n_rep : 65535)), block(BT);
  hipLaunchKernelGGL((deviance_kernel<KP>), grid, block, 0, s, d, h, k, n, p, p_total, j0, rule, n_rep, log_shift, dev);
  return check_hip(hipGetLastError(), "sample deviance launch");
}

}  // namespace samplek
#endif

}  // namespace espm

using namespace espm;

#if ESPM_KP == 8
// what both entry points ask of the model and the slab, before the device is touched
static int sample_check(const char* who, const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, int64_t first_rep,
                        int64_t last_rep) {
  ESPM_REQUIRE(d && h, "%s: bad arguments (d %p, h %p)", who, (const void*)d, (const void*)h);
  ESPM_REQUIRE(k >= 1 && k <= ESPM_SAMPLE_MAX_K, "%s: k=%d (1..%d components)", who, k, ESPM_SAMPLE_MAX_K);
  ESPM_REQUIRE(n >= 1 && p >= 1, "%s: bad arguments (n=%d, p=%d)", who, n, p);
  if (int rc = check_slab(who, n, p, p_total, j0)) return rc;
  ESPM_REQUIRE(first_rep >= 0 && last_rep <= (int64_t)0xFFFFFFFEll, "%s: replicate=%lld .. %lld (0 .. 2^32 - 2)", who, (long long)first_rep,
               (long long)last_rep);
  return ESPM_OK;
}

static samplek::Rule sample_rule(uint64_t seed, int64_t replicate) {
  samplek::Rule r;
  r.key0 = (uint32_t)seed, r.key1 = (uint32_t)(seed >> 32), r.rep1 = (uint32_t)replicate + 1u;
  return r;
}
#endif

extern "C" int espm_poisson_sample(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, uint64_t seed,
                                   int64_t replicate, void* x, int x_dtype, int x_layout, int64_t ld, int64_t* counts, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "poisson sampling: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  if (int rc = sample_check("poisson sample", d, h, k, n, p, p_total, j0, replicate, replicate)) return rc;
  ESPM_REQUIRE(x && counts, "poisson sample: bad arguments (x %p, counts %p)", x, (void*)counts);
  if (int rc = check_image("poisson sample", x, x_dtype, ESPM_DIAG_X_U16, x_layout, ld, n, p)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const samplek::Rule rule = sample_rule(seed, replicate);
  if (int rc = check_hip(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s), "poisson sample: zeroing the counters")) return rc;
  return dispatch_kp(k, [&](auto kp) {
    return dispatch_xt<ESPM_DIAG_X_U16>(x_dtype, [&](auto xt) {
      return samplek::launch_sample<decltype(kp)::value, typename decltype(xt)::type>(d, h, k, n, p, p_total, j0, rule, x, x_layout, ld, counts, s);
    });
  });
#endif
}

extern "C" int espm_sample_deviance(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, uint64_t seed,
                                    int64_t replicate0, int n_rep, double log_shift, double* dev, espm_stream_t stream) {
#if ESPM_KP != 8
  return set_error(ESPM_EUNSUPPORTED, "poisson sampling: built into the 1..%d component library only", ESPM_DIAG_MAX_K);
#else
  ESPM_REQUIRE(n_rep >= 1, "sample deviance: n_rep=%d (at least one replicate)", n_rep);
  const int64_t last = replicate0 > (int64_t)0xFFFFFFFEll ? replicate0 : replicate0 + n_rep - 1;   // (no overflow of the sum)
  if (int rc = sample_check("sample deviance", d, h, k, n, p, p_total, j0, replicate0, last)) return rc;
  ESPM_REQUIRE(dev, "sample deviance: bad arguments (dev is null)");
  ESPM_REQUIRE(log_shift > 0, "sample deviance: log_shift=%g must be positive", log_shift);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const samplek::Rule rule = sample_rule(seed, replicate0);
  return dispatch_kp(k, [&](auto kp) {
    return samplek::launch_deviance<decltype(kp)::value>(d, h, k, n, p, p_total, j0, rule, n_rep, log_shift, dev, s);
  });
#endif
}
