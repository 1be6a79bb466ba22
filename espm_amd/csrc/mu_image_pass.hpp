// What the passes over a count image share (mu_diag.hip, mu_diag_chan.hip, mu_split.hip, mu_sample.hip, mu_attrib.hip, mu_marginals.hip, mu_residual.hip): the pieces of
// the rules of include/espm_mu.h that are defined bit for bit, the walk of "a lane owns one index, a thread walks the other", and the
// host side's checks and dispatch.  ONE copy of each: a changed Philox constant, a wrong broadcast of e's high word or a tile index off
// by one still gives plausible counts.  DESIGN.md ("the image-pass header") lists what lives here and what deliberately does not.
//
// Included INSIDE namespace espm, behind the unit's `#if ESPM_KP == 8`, after mu_common.hpp and <type_traits>.
#pragma once

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
  return v;
}

// The heavy entries of a wave, one after the other.  EVERY lane of the wave comes here together with its own entry (heavy, x, e); for
// each lane that holds a heavy one, in ascending lane order, its x and its 64-bit e are broadcast and f(src, xh, eh) runs wave-uniformly:
// the wave shares that entry's draws and lane src keeps the result.  (attribk::assign_entry has this loop written out: its file comment.)
template <typename F>
__device__ __forceinline__ void for_each_heavy(bool heavy, uint32_t x, uint64_t e, F f) {
  unsigned long long todo = __ballot(heavy);
  while (todo) {   // (wave-uniform)
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t xh = (uint32_t)__shfl((int)x, src, 64);
    const uint64_t eh = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(e >> 32), src, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)e, src, 64);
    f(src, xh, eh);
  }
}

// sum over the wave of f(b) for the blocks of four b with 4 b < n: lane l takes b = l, l + 64, ... (integers: any order gives the same sum)
template <typename F>
__device__ __forceinline__ uint32_t wave_blocks_sum(uint32_t n, F f) {
  const int lane = threadIdx.x & 63;
  uint32_t mine = 0;
  for (uint32_t b = (uint32_t)lane; 4u * b < n; b += 64u) mine += f(b);
  return wave_sum_u32(mine);
}

// component i of the k-vector of index q: ptr[i * cs + q * qs] (h: cs = p, qs = 1; d: cs = 1, qs = k)
struct Vec {
  const double* ptr;
  int64_t cs, qs;
};

template <int KP>
constexpr int stage_rows() { return KP <= 8 ? 256 : 2048 / KP; }   // walk indices per round: at most 16 KB of LDS

// the vectors of the walk indices w0 .. w0 + wn - 1, padded with zeros to KP columns, into LDS (a padded product is an exact zero);
// IT: the caller's index type (int or int64_t) - the index is formed as the caller formed it
template <int KP, int BT, typename IT>
__device__ __forceinline__ void stage(double* ds, const Vec& v, IT w0, int wn, int k) {
  for (int i = threadIdx.x; i < wn * KP; i += BT) {
    const int w = i / KP, j = i % KP;
    ds[i] = j < k ? v.ptr[(int64_t)(w0 + w) * v.qs + (int64_t)j * v.cs] : 0.0;
  }
}

// a round of BT walk indices, every thread its OWN index w0 + threadIdx.x: that index's vector into ds[threadIdx.x * KP ..], zeros beyond
// k and beyond wn.  The KP loads of a thread are independent and, where qs == 1 (h, or weights that run along the walk), those of one
// component are consecutive over the threads - where `stage` would walk such a vector KP rows at a time.  Returns whether any component
// of the thread's vector is not 0 (margk: the walk indices that carry a weight).
template <int KP, int BT, typename IT>
__device__ __forceinline__ bool stage_own(double* ds, const Vec& v, IT w0, int wn, int k) {
  const bool in = (int)threadIdx.x < wn;
  double c[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) c[j] = in && j < k ? v.ptr[(int64_t)(w0 + threadIdx.x) * v.qs + (int64_t)j * v.cs] : 0.0;
  bool any = false;
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    ds[threadIdx.x * KP + j] = c[j];
    any |= c[j] != 0.0;
  }
  return any;
}

// The transposing tile of the layout whose rows run along the walk: tile_rows<XT>() walk indices of BT lanes (u8: 16 KB, the others
// 33 KB), lanes BT + 1 apart.  Element i * BT + tid of a pass over it is lane el / TS, walk index el % TS: consecutive threads touch
// consecutive entries of one row of x, and a thread reads back (or has written) its own lane's column.
template <typename XT>
constexpr int tile_rows() { return sizeof(XT) <= 2 ? 64 : sizeof(XT) == 4 ? 32 : 16; }

template <typename XT, int BT>
__device__ __forceinline__ int tile_slot(int i, int& li, int& w) {
  constexpr int TS = tile_rows<XT>();
  const int el = i * BT + threadIdx.x;
  li = el / TS, w = el % TS;
  return w * (BT + 1) + li;
}

// tile <- x[(l0 + lane) * ld + w0 + walk], walk < tn, zeros beyond `lanes` and tn (the caller's barriers stand around it): diagk and
// attribk.  splitk::deviance_kernel writes the same loop out over tile_slot (its file comment), samplek::sample_kernel runs it storing.
template <typename XT, int BT, typename IT>
__device__ __forceinline__ void fill_tile(XT* tile, const XT* __restrict__ x, int64_t ld, IT l0, int lanes, IT w0, int tn) {
#pragma unroll 8
  for (int i = 0; i < tile_rows<XT>(); ++i) {
    int li, w;
    const int at = tile_slot<XT, BT>(i, li, w);
    XT v = XT(0);
    if (l0 + li < lanes && w < tn) v = x[(size_t)(l0 + li) * ld + (w0 + w)];
    tile[at] = v;
  }
}

// N counters of a workgroup of NW waves: the threads' values summed over the wave, the waves' over the workgroup through `part`, then
// one 64-bit integer atomic per counter that is not 0 (sums of integers: exact, and the same from call to call)
template <int N, int NW>
__device__ __forceinline__ void block_count_add(uint32_t (&part)[N][NW], const uint32_t (&v)[N], unsigned long long* __restrict__ counts) {
  uint32_t t[N];
#pragma unroll
  for (int i = 0; i < N; ++i) t[i] = wave_sum_u32(v[i]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) part[i][threadIdx.x >> 6] = t[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned long long s = 0;
    for (int w = 0; w < NW; ++w) s += part[threadIdx.x][w];
    if (s) atomicAdd(counts + threadIdx.x, s);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// what every entry point asks of the image before the device is touched; max_dtype ESPM_DIAG_X_U16: counts only
inline int check_image(const char* who, const void* x, int x_dtype, int max_dtype, int x_layout, int64_t ld, int n, int p) {
  ESPM_REQUIRE(x && n >= 1 && p >= 1, "%s: bad arguments (x %p, n=%d, p=%d)", who, x, n, p);
  ESPM_REQUIRE(x_layout == ESPM_LAYOUT_CM || x_layout == ESPM_LAYOUT_PM, "%s: x_layout %d", who, x_layout);
  ESPM_REQUIRE(x_dtype >= ESPM_DIAG_X_U8 && x_dtype <= max_dtype, "%s: x_dtype %d%s", who, x_dtype,
               max_dtype == ESPM_DIAG_X_U16 ? " (counts: u8 or u16)" : "");
  const int row = x_layout == ESPM_LAYOUT_CM ? p : n;
  ESPM_REQUIRE(ld >= row, "%s: ld=%lld below the row length %d", who, (long long)ld, row);
  return ESPM_OK;
}

// the slab of pixels j0 .. j0 + p of the logical (n, p_total) image, and its 64-bit element index
inline int check_slab(const char* who, int n, int p, int64_t p_total, int64_t j0) {
  ESPM_REQUIRE(j0 >= 0 && p_total >= p && j0 <= p_total - p, "%s: pixels j0=%lld .. j0 + p=%lld of p_total=%lld", who, (long long)j0,
               (long long)j0 + p, (long long)p_total);
  ESPM_REQUIRE(p_total <= INT64_MAX / n, "%s: n=%d x p_total=%lld elements (a 64-bit index)", who, n, (long long)p_total);
  return ESPM_OK;
}

// f(std::integral_constant<int, KP>) for the padded stride KP = 4, 8, 16 or 32 that holds k components
template <typename F>
int dispatch_kp(int k, F&& f) {
  if (k <= 4) return f(std::integral_constant<int, 4>{});
  if (k <= 8) return f(std::integral_constant<int, 8>{});
  if (k <= 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 32>{});
}

// f(std::integral_constant<int, K>) for the exact K = k of this build (1 .. 8); no other k reaches it
template <typename F>
int dispatch_k_exact(int k, F&& f) {
  switch (k) {
#define ESPM_K_EXACT_CASE(KK) \
  case KK: return f(std::integral_constant<int, KK>{});
    ESPM_K_CASES(ESPM_K_EXACT_CASE)
#undef ESPM_K_EXACT_CASE
  }
  return ESPM_OK;
}

// f(type_tag<XT>) for the element type of a checked x_dtype <= MAX_DTYPE (ESPM_DIAG_X_U16: u8 and u16 only are instantiated)
template <typename T>
struct type_tag { using type = T; };

template <int MAX_DTYPE, typename F>
int dispatch_xt(int x_dtype, F&& f) {
  if (x_dtype == ESPM_DIAG_X_U8) return f(type_tag<uint8_t>{});
  if constexpr (MAX_DTYPE == ESPM_DIAG_X_U16) return f(type_tag<uint16_t>{});
  else {
    if (x_dtype == ESPM_DIAG_X_U16) return f(type_tag<uint16_t>{});
    if (x_dtype == ESPM_DIAG_X_F32) return f(type_tag<float>{});
    return f(type_tag<double>{});
  }
}
