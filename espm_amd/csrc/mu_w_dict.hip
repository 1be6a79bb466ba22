// The W step behind the slab reduction with a dictionary G (the W step as a whole: mu_w_parts.hpp), as many-workgroup launches,
// sharded or not; what these do not apply to keeps the one-workgroup finish (mu_w_finish.hip).
#include <atomic>

#include "mu_w_parts.hpp"

namespace espm {

// ---- W finish with a dictionary G (n x m, few columns) as TWO launches (C5: 1980 x 17, k = 8) ----------------------------------
// The one-workgroup finish spends its 24-36 us on one CU: the m k dot products G^T A over the n channels (butterfly sums across a
// wave) and the rows of G W'.  The W update needs nothing global but the row sums of H' (no simplex over W here), so:
//   w_gfinish_update_kernel  one workgroup per entry (row of G, component): G^T A over the channels from the transposed copy of G
//                            (coalesced), a fixed-order block sum, W' = max(W (G^T A) / (colsum(G) rowsum(H')), eps), fixed_W
//                            (updates.py:58-60, :70-76)
//   w_gfinish_gw_kernel      256 channels per workgroup: W' (m k floats) into LDS, the rows of G W' (a thread per channel: m k
//                            multiply-adds from LDS, its row of G requested with W'); workgroup 0 forms the column sums of G W' as
//                            colsum(G)^T W' (round 4: per-workgroup partials + a ticket before), mean(W') and rel_W (base.py:323)
// ESPM_W_GSPLIT=0 keeps the one-workgroup finish (A/B).
__global__ __launch_bounds__(256) void w_gfinish_update_kernel(const WFinishArgs a) {
  __shared__ float s_wave[4];
  const int e = blockIdx.x, mm = e / a.k, kk = e - mm * a.k;
  const float* gt = a.g_t + (size_t)mm * a.n_pad;
  const float* av = a.a + (size_t)kk * a.n_pad;
  float s = 0.f;
  for (int c0 = threadIdx.x; c0 < a.n; c0 += 8 * 256) {   // eight channels per thread requested together (a loop of single loads waits for each)
    float gv[8], vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + u * 256;
      gv[u] = c < a.n ? gt[c] : 0.f;
      vv[u] = c < a.n ? av[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s = fmaf(gv[u], vv[u], s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float gta = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    const float num = a.w_old[e] * gta;
    const float den = a.colsum_g[mm] * (float)a.hstat[ESPM_HS_ROWSUM + kk];
    float wn = fmaxf(num / den, a.log_shift);
    if (a.fixed_w && a.fixed_w[e] >= 0.f) wn = a.fixed_w[e];
    a.w_new[e] = wn;
  }
}

// workgroup b: channels 256 b .. 256 b + 255, one per thread; partial column sums -> scratch; the workgroup that finishes last adds
// them in workgroup order (the same bits whoever is last) and forms mean(W') and rel_W
__global__ __launch_bounds__(256) void w_gfinish_gw_kernel(const WFinishArgs a) {
  extern __shared__ float s_w[];   // [m * k] the new W
  __shared__ double scratch[(256 / 64 + 1) * 2 * KP];
  const int tid = threadIdx.x, mk = a.m * a.k, k = a.k;
  // Round 4: ONE trip to memory.  The rows of G do not depend on W': they are requested together with it.  And the column sums of
  // G W' - the denominator of the next H update, updates.py:132 - are sum_m colsum(G)[m] W'[m, k] (fp64, workgroup 0, from the copy of
  // W' it holds anyway) instead of the sum of the rows over the channels, which took per-workgroup partials, a drain, a ticket and
  // the last workgroup's agent-scope loads: four more dependent round trips in a launch that is nothing but latency (14.3 us for 8
  // workgroups at BASELINE configuration 5, profiles/r03l_ks_c5_128rows_kernel_stats.csv).  The two sums agree to the rounding of
  // the fp32 rows (~1e-7 relative; an entry below gw_floor counts as itself, not as the floor: < 1e-30 each).
  // The LAST workgroup has no rows: it forms the column sums, mean(W') and rel_W - two block reductions behind loads of their own (W',
  // W, colsum(G), all requested at its start) - next to the row workgroups instead of behind workgroup 0's rows.
  if (blockIdx.x == gridDim.x - 1) {
    float wo[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wo[u] = (tid + 256 * u < mk && a.hist_slot) ? a.w_old[tid + 256 * u] : 1.f;   // (up to 1024 entries requested with W'; beyond that in the loop)
    for (int e = tid; e < mk; e += 256) s_w[e] = a.w_new[e];
    __syncthreads();
    if (tid < KP) {
      double v = 0.0;
      if (tid < k)
        for (int mm = 0; mm < a.m; ++mm) v += (double)a.colsum_g[mm] * (double)s_w[mm * k + tid];
      a.colsum_gw[tid] = v;
    }
    if (a.hist_slot) {   // mean(W') and rel_W (base.py:323) over the m k entries
      double sum_l = 0.0;
      for (int e = tid; e < mk; e += 256) sum_l += (double)s_w[e];
      const double mean_w = block_sum1(sum_l, scratch) / (double)mk;
      double rel_l = 0.0;
      for (int e = tid, u = 0; e < mk; e += 256, ++u) {
        const double wn = s_w[e], wov = u < 4 ? wo[u] : a.w_old[e];
        rel_l = fmax(rel_l, fabs(wn - wov) / (wn + (double)a.rel_tol * mean_w));
      }
      const double rel_w = block_max1(rel_l, scratch);
      if (tid == 0) a.hist_slot[ESPM_HI_REL_W] = rel_w;
    }
    return;
  }
  const int c = blockIdx.x * 256 + tid;
  constexpr int GM = 32;   // entries of a row of G requested together (a dictionary has a few tens of columns)
  float gv[GM];
  const float* gc = a.g_t + (c < a.n ? c : 0);   // (the transposed copy: the lanes of a wave read neighbouring channels of one column of G)
#pragma unroll
  for (int u = 0; u < GM; ++u) gv[u] = (c < a.n && u < a.m) ? gc[(size_t)u * a.n_pad] : 0.f;
  for (int e = tid; e < mk; e += 256) s_w[e] = a.w_new[e];
  __syncthreads();
  // GW = G W' (updates.py:107 of the next half step), stored / xscale with a positive floor
  const float inv_scale = 1.f / a.xscale;
  if (c < a.n_pad) {
    float row[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) row[kk] = (kk < k && c >= a.n) ? 1.f : 0.f;   // padding channels: X = 0 there, any positive value keeps X / Y = 0
    if (c < a.n) {
      for (int m0 = 0; m0 < a.m; m0 += GM) {
        if (m0 > 0) {   // (more than GM columns: the further ones in batches of their own)
#pragma unroll
          for (int u = 0; u < GM; ++u) gv[u] = m0 + u < a.m ? gc[(size_t)(m0 + u) * a.n_pad] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < GM; ++u)
          if (m0 + u < a.m) {
#pragma unroll
            for (int kk = 0; kk < KP; ++kk)
              if (kk < k) row[kk] = fmaf(gv[u], s_w[(m0 + u) * k + kk], row[kk]);
          }
      }
#pragma unroll
      for (int kk = 0; kk < KP; ++kk)
        if (kk < k) row[kk] = fmaxf(row[kk], a.gw_floor) * inv_scale;
    }
    store_row_kp(a.gw_s + (size_t)c * KP, row);
  }
}

// ---- the same on a SHARDED image: what crosses the links is G^T A (m k values), not A (k n) -------------------------------------
// G^T (sum over the ranks of A_r) = sum over the ranks of G^T A_r: every rank contracts its OWN A with G (the update kernel's dot
// products), sends the m k results - one granule each, with the statistics and the boundary rows as in w_exchange_update_kernel -
// and adds the ranks' values in rank order: the same W' on every rank.  For C5 a rank ships 136 granules instead of a 63 KB record,
// and the sharded W step is three launches behind the accumulation (slab reduction + record reduction, this kernel, the rows of
// G W') instead of seven (reduce + pack, post, wait, combine, and the finish).
// grid: workgroup 0 = the extra workgroup (boundary rows, statistics, their flag), workgroup 1 + e = entry e = (row of G, component).
struct WGxchgArgs {
  WFinishArgs f;
  const double* hstat_local;   // this rank's statistics of the new H (the slab reduction's finalize left them in its own record)
  double* hstat_out;           // the global ones
  unsigned char* mbox[16];
  int world, rank, nfl, with_halo;
  size_t rec_bytes, slot_base, wgflags_off, gran_off, err_off, top_off, bot_off;
  unsigned int seq;
  long long max_ticks;
  int release;
  const float* halo_h;
  int halo_k, halo_nx, halo_ny, halo_ppad;
};

__global__ __launch_bounds__(256) void w_gxchg_update_kernel(const WGxchgArgs x) {
  const WFinishArgs& a = x.f;
  __shared__ float s_wave[4];
  const int mk = a.m * a.k;
  auto record = [&](int dst, int src_rank) { return x.mbox[dst] + x.slot_base + (size_t)src_rank * x.rec_bytes; };
  auto flag = [&](int dst, int src_rank) {   // (the extra workgroup's flag: index nfl - 1 of a rank's flags)
    return reinterpret_cast<unsigned int*>(x.mbox[dst] + x.wgflags_off + ((size_t)src_rank * x.nfl + (x.nfl - 1)) * sizeof(unsigned int));
  };
  const size_t GRAN = (size_t)34 * x.nfl + 2 * ESPM_HS_STRIDE;
  auto gran = [&](int dst, int src_rank, int g) {
    return reinterpret_cast<unsigned long long*>(x.mbox[dst] + x.gran_off) + (size_t)src_rank * GRAN + g;
  };
  unsigned int* err = reinterpret_cast<unsigned int*>(x.mbox[x.rank] + x.err_off);
  if (blockIdx.x == 0) {   // boundary rows (16-byte write-through stores), statistics as granules, the rows' flag
    if (x.with_halo) {
      for (int d = -1; d <= 1; ++d) {
        const int r = x.rank + d;
        if (r < 0 || r >= x.world) continue;
        float* top = reinterpret_cast<float*>(record(r, x.rank) + x.top_off);
        float* bot = reinterpret_cast<float*>(record(r, x.rank) + x.bot_off);
        if ((x.halo_ny & 3) == 0) {
          typedef float xf4 __attribute__((ext_vector_type(4)));
          for (int e = 4 * threadIdx.x; e < x.halo_k * x.halo_ny; e += 4 * 256) {
            const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
            const xf4 vt = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + j);
            const xf4 vb = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j);
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(top + e), "v"(vt) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(bot + e), "v"(vb) : "memory");
          }
        } else {
          for (int e = threadIdx.x; e < x.halo_k * x.halo_ny; e += 256) {
            const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
            __hip_atomic_store(top + e, x.halo_h[(size_t)kk * x.halo_ppad + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(bot + e, x.halo_h[(size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
      }
    }
    for (int i = threadIdx.x; i < x.world * 2 * ESPM_HS_STRIDE; i += 256) {
      const int r = i / (2 * ESPM_HS_STRIDE), j = i - r * 2 * ESPM_HS_STRIDE;
      const unsigned long long bits = __builtin_bit_cast(unsigned long long, x.hstat_local[j >> 1]);
      const unsigned int half = (j & 1) ? (unsigned int)(bits >> 32) : (unsigned int)bits;
      __hip_atomic_store(gran(r, x.rank, 34 * x.nfl + j), ((unsigned long long)x.seq << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((int)threadIdx.x < x.world) xchg_store_flag(flag(threadIdx.x, x.rank), x.seq, x.release);
    return;
  }
  const int e = (int)blockIdx.x - 1, mm = e / a.k, kk = e - mm * a.k;
  const float* gt = a.g_t + (size_t)mm * a.n_pad;
  const float* av = a.a + (size_t)kk * a.n_pad;
  const float wo = a.w_old[e];
  const float fx = a.fixed_w ? a.fixed_w[e] : -1.f;
  float s = 0.f;
  for (int c0 = threadIdx.x; c0 < a.n; c0 += 8 * 256) {
    float gv[8], vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = c0 + u * 256;
      gv[u] = c < a.n ? gt[c] : 0.f;
      vv[u] = c < a.n ? av[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s = fmaf(gv[u], vv[u], s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const float gta_mine = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
  if (lane < x.world)   // this rank's value of entry e, to every rank
    __hip_atomic_store(gran(lane, x.rank, e), ((unsigned long long)x.seq << 32) | __float_as_uint(gta_mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // lanes 0..15: rank r's value of entry e; 16..31 / 32..47: the low / high half of rank r's row sum kk of its new H block
  const int r_of = lane & 15, what = lane >> 4;
  const bool polls = what < 3 && r_of < x.world;
  const int g_idx = what == 0 ? e : 34 * x.nfl + 2 * (ESPM_HS_ROWSUM + kk) + (what - 1);
  unsigned int got = 0;
  {
    const long long t0 = wall_clock64();
    for (;;) {
      const unsigned long long v = polls ? __hip_atomic_load(gran(x.rank, r_of, g_idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ((unsigned long long)x.seq << 32);
      const bool ok = (unsigned int)(v >> 32) == x.seq;
      got = (unsigned int)v;
      if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
      if (wall_clock64() - t0 > x.max_ticks) {
        if (!ok) atomicAdd(err, 1u);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  float gta = 0.f;
  double rs = 0.0;
  for (int r = 0; r < x.world; ++r) {   // rank order: the same sums on every rank
    gta += __uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)got, r));
    const unsigned long long lo = (unsigned int)__builtin_amdgcn_readlane((int)got, 16 + r), hi = (unsigned int)__builtin_amdgcn_readlane((int)got, 32 + r);
    rs += __builtin_bit_cast(double, (hi << 32) | lo);
  }
  if (lane == 0) {   // updates.py:58-60, :70-76
    const float num = wo * gta, den = a.colsum_g[mm] * (float)rs;
    float wn = fmaxf(num / den, a.log_shift);
    if (fx >= 0.f) wn = fx;
    a.w_new[e] = wn;
  }
  if (e == 0) {   // the global statistics of the new H (the NEXT launch reads them) and the neighbours' boundary rows' flag
    for (int hl = lane; hl < ((2 * ESPM_HS_STRIDE + 63) & ~63); hl += 64) {   // (64 halves of statistics per pass: two passes in the widest build)
    const bool p2 = hl < 2 * ESPM_HS_STRIDE;
    unsigned int hv[16];
    const long long t0 = wall_clock64();
    for (;;) {
      unsigned long long v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        v[r] = (p2 && r < x.world) ? __hip_atomic_load(gran(x.rank, r, 34 * x.nfl + hl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                   : ((unsigned long long)x.seq << 32);
      bool all = true;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        all = all && (unsigned int)(v[r] >> 32) == x.seq;
        hv[r] = (unsigned int)v[r];
      }
      if (__builtin_amdgcn_ballot_w64(!all) == 0) break;
      if (wall_clock64() - t0 > x.max_ticks) {
        if (!all) atomicAdd(err, 1u);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r < x.world) {
        const unsigned int other = (unsigned int)__shfl_xor((int)hv[r], 1, 64);
        const unsigned long long bits = (lane & 1) ? (((unsigned long long)hv[r] << 32) | other) : (((unsigned long long)other << 32) | hv[r]);
        const double v2 = __builtin_bit_cast(double, bits);
        g = (hl >> 1) < ESPM_HS_MAX ? g + v2 : fmax(g, v2);
      }
    if (p2 && !(lane & 1)) x.hstat_out[hl >> 1] = g;
    }
    if (lane < x.world) xchg_wait_flag(flag(x.rank, lane), x.seq, x.max_ticks, err);
  }
}

// ---- the dictionary-G W step by COLUMNS: one launch behind the slab reduction (round 5) ------------------------------------------------
// With a dictionary of few columns (C5: G 1980 x 17, k = 8) component kk of the whole W update is small enough for ONE workgroup:
//   G^T A[:, kk]   m dot products over the n channels (a thread holds its 1 or 2 channels' rows of G^T in registers, and A[kk, :] once for all m),
//   (sharded) the m values cross the links as granules and come back summed in rank order, with the ranks' row sums of H'[kk, :],
//   W'[:, kk] = max(W (G^T A) / (colsum(G) rowsum(H')), eps), fixed_W                                        (updates.py:58-60, :70-76)
//   G W'[:, kk]    from the SAME registers of G^T: the column of the table the next H update gathers from, its sum as colsum(G)^T W'[:, kk].
// Nothing a workgroup needs comes from another workgroup of the launch, so what were two launches with a boundary between them - the update
// per entry of W (m k workgroups, each loading a row of A and a row of G^T for ONE dot product) and the rows of G W' (which need all of W') -
// is one: configuration 5's W step is two launches behind the fused one instead of three.  What IS global - mean(W') for
// rel_W (base.py:323) - is formed by one extra wave (the finisher) from the columns' sums, which arrive as 8-byte granules {launch nonce,
// fp32 sum}: value and "it is there" in one store, no counter to reset, stale content of the scratch never matches (the nonce is the
// process's launch count).  The entries of W' the finisher compares are stored write-through (sc1) and drained before the granule, and read
// with sc1 loads behind it (MI355X_MICROARCH.md, valid forms: data-tagged granules; sc1 payload drained before the flag, sc1 loads).
// Built for m <= GC_MMAX columns and n_pad <= GC_CPT * GC_THREADS channels; anything else keeps the launches above.
// (GC_THREADS, GC_CPT, GC_MMAX: mu_w_plan.hpp, with the predicate of this form)

// the extra workgroup of a sharded exchange launch: boundary rows of H' (16-byte write-through stores), this rank's statistics as granules, the rows' flag
__device__ __forceinline__ void gxchg_extra_role(const WGxchgArgs& x, int nthreads) {
  auto record = [&](int dst, int src_rank) { return x.mbox[dst] + x.slot_base + (size_t)src_rank * x.rec_bytes; };
  auto flag = [&](int dst, int src_rank) {
    return reinterpret_cast<unsigned int*>(x.mbox[dst] + x.wgflags_off + ((size_t)src_rank * x.nfl + (x.nfl - 1)) * sizeof(unsigned int));
  };
  const size_t GRAN = (size_t)34 * x.nfl + 2 * ESPM_HS_STRIDE;
  auto gran = [&](int dst, int src_rank, int g) {
    return reinterpret_cast<unsigned long long*>(x.mbox[dst] + x.gran_off) + (size_t)src_rank * GRAN + g;
  };
  if (x.with_halo) {
    for (int d = -1; d <= 1; ++d) {
      const int r = x.rank + d;
      if (r < 0 || r >= x.world) continue;
      float* top = reinterpret_cast<float*>(record(r, x.rank) + x.top_off);
      float* bot = reinterpret_cast<float*>(record(r, x.rank) + x.bot_off);
      if ((x.halo_ny & 3) == 0) {
        typedef float xf4 __attribute__((ext_vector_type(4)));
        for (int e = 4 * threadIdx.x; e < x.halo_k * x.halo_ny; e += 4 * nthreads) {
          const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
          const xf4 vt = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + j);
          const xf4 vb = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j);
          asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(top + e), "v"(vt) : "memory");
          asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(bot + e), "v"(vb) : "memory");
        }
      } else {
        for (int e = threadIdx.x; e < x.halo_k * x.halo_ny; e += nthreads) {
          const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
          __hip_atomic_store(top + e, x.halo_h[(size_t)kk * x.halo_ppad + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(bot + e, x.halo_h[(size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
    }
  }
  for (int i = threadIdx.x; i < x.world * 2 * ESPM_HS_STRIDE; i += nthreads) {
    const int r = i / (2 * ESPM_HS_STRIDE), j = i - r * 2 * ESPM_HS_STRIDE;
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, x.hstat_local[j >> 1]);
    const unsigned int half = (j & 1) ? (unsigned int)(bits >> 32) : (unsigned int)bits;
    __hip_atomic_store(gran(r, x.rank, 34 * x.nfl + j), ((unsigned long long)x.seq << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if ((int)threadIdx.x < x.world) xchg_store_flag(flag(threadIdx.x, x.rank), x.seq, x.release);
}

// one wave: the global statistics of the new H from the ranks' granules (the NEXT launch reads them), then the neighbours' boundary rows' flag
__device__ __forceinline__ void gxchg_global_stats_role(const WGxchgArgs& x, int lane) {
  auto flag = [&](int dst, int src_rank) {
    return reinterpret_cast<unsigned int*>(x.mbox[dst] + x.wgflags_off + ((size_t)src_rank * x.nfl + (x.nfl - 1)) * sizeof(unsigned int));
  };
  const size_t GRAN = (size_t)34 * x.nfl + 2 * ESPM_HS_STRIDE;
  auto gran = [&](int dst, int src_rank, int g) {
    return reinterpret_cast<unsigned long long*>(x.mbox[dst] + x.gran_off) + (size_t)src_rank * GRAN + g;
  };
  unsigned int* err = reinterpret_cast<unsigned int*>(x.mbox[x.rank] + x.err_off);
  for (int hl = lane; hl < ((2 * ESPM_HS_STRIDE + 63) & ~63); hl += 64) {   // (64 halves of statistics per pass: two passes in the widest build)
  const bool p2 = hl < 2 * ESPM_HS_STRIDE;
  unsigned int hv[16];
  const long long t0 = wall_clock64();
  for (;;) {
    unsigned long long v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
      v[r] = (p2 && r < x.world) ? __hip_atomic_load(gran(x.rank, r, 34 * x.nfl + hl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                 : ((unsigned long long)x.seq << 32);
    bool all = true;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      all = all && (unsigned int)(v[r] >> 32) == x.seq;
      hv[r] = (unsigned int)v[r];
    }
    if (__builtin_amdgcn_ballot_w64(!all) == 0) break;
    if (wall_clock64() - t0 > x.max_ticks) {
      if (!all) atomicAdd(err, 1u);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  double g = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r < x.world) {
      const unsigned int other = (unsigned int)__shfl_xor((int)hv[r], 1, 64);
      const unsigned long long bits = (lane & 1) ? (((unsigned long long)hv[r] << 32) | other) : (((unsigned long long)other << 32) | hv[r]);
      const double v2 = __builtin_bit_cast(double, bits);
      g = (hl >> 1) < ESPM_HS_MAX ? g + v2 : fmax(g, v2);
    }
  if (p2 && !(lane & 1)) x.hstat_out[hl >> 1] = g;
  }
  if (lane < x.world) xchg_wait_flag(flag(x.rank, lane), x.seq, x.max_ticks, err);
}

// grid: [XCHG: workgroup 0 = the exchange's extra workgroup] k column workgroups, then the finisher (one wave does the work)
template <bool XCHG>
__global__ __launch_bounds__(GC_THREADS) void w_gcol_kernel(const WGxchgArgs x, unsigned int nonce) {
  const WFinishArgs& a = x.f;
  __shared__ float s_red[GC_THREADS / 64][GC_MMAX];
  __shared__ unsigned int s_got[GC_MMAX + 2][16];
  __shared__ float s_w[GC_MMAX], s_csg[GC_MMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.m, k = a.k, mk = m * k;
  const int first = XCHG ? 1 : 0;
  unsigned long long* colgran = reinterpret_cast<unsigned long long*>(a.scratch);   // [k] {nonce, fp32 sum of W'[:, kk]}
  if (XCHG && blockIdx.x == 0) {
    gxchg_extra_role(x, GC_THREADS);
    return;
  }
  if ((int)blockIdx.x == first + k) {   // ---- the finisher: mean(W'), rel_W (base.py:323); sharded: the global statistics of H'
    if (tid >= 64) return;
    if (XCHG) gxchg_global_stats_role(x, lane);
    if (lane < KP - k) a.colsum_gw[k + lane] = 0.0;
    if (!a.hist_slot) return;
    float sw = 0.f;
    const long long t0 = wall_clock64();
    for (;;) {
      const unsigned long long v = lane < k ? __hip_atomic_load(colgran + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((unsigned long long)nonce << 32);
      const bool ok = (unsigned int)(v >> 32) == nonce;
      sw = __uint_as_float((unsigned int)v);
      if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
      if (wall_clock64() - t0 > 4 * x.max_ticks) break;   // (every column workgroup reaches its granule: its own waits are bounded)
      __builtin_amdgcn_s_sleep(1);
    }
    double sum = 0.0;
    for (int kk = 0; kk < k; ++kk) sum += (double)__uint_as_float((unsigned int)__builtin_amdgcn_readlane((int)__float_as_uint(sw), kk));
    const double shift = (double)a.rel_tol * (sum / (double)mk);
    double rel = 0.0;
    for (int e = lane; e < mk; e += 64) {
      const double wn = (double)__hip_atomic_load(a.w_new + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), wov = (double)a.w_old[e];
      rel = fmax(rel, fabs(wn - wov) / (wn + shift));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rel = fmax(rel, __shfl_xor(rel, off, 64));
    if (lane == 0) a.hist_slot[ESPM_HI_REL_W] = rel;
    return;
  }
  // ---- column kk ----
  const int kk = (int)blockIdx.x - first;
  float av[GC_CPT], gv[GC_MMAX][GC_CPT];
#pragma unroll
  for (int u = 0; u < GC_CPT; ++u) {
    const int c = tid + GC_THREADS * u;
    av[u] = c < a.n ? a.a[(size_t)kk * a.n_pad + c] : 0.f;
#pragma unroll
    for (int mm = 0; mm < GC_MMAX; ++mm) gv[mm][u] = (c < a.n && mm < m) ? a.g_t[(size_t)mm * a.n_pad + c] : 0.f;
  }
  float wo = 1.f, fx = -1.f;
  if (tid < m) {
    wo = a.w_old[tid * k + kk];
    if (a.fixed_w) fx = a.fixed_w[tid * k + kk];
    s_csg[tid] = a.colsum_g[tid];
  }
#pragma unroll
  for (int mm = 0; mm < GC_MMAX; ++mm) {
    if (mm < m) {   // (uniform)
      float part = gv[mm][0] * av[0];
#pragma unroll
      for (int u = 1; u < GC_CPT; ++u) part = fmaf(gv[mm][u], av[u], part);
      part = wave_sum(part);
      if (lane == 0) s_red[wave][mm] = part;
    }
  }
  __syncthreads();
  float gta = 0.f;
  if (tid < m) {
#pragma unroll
    for (int w = 0; w < GC_THREADS / 64; ++w) gta += s_red[w][tid];   // wave order
  }
  double rs;
  if constexpr (XCHG) {
    const size_t GRAN = (size_t)34 * x.nfl + 2 * ESPM_HS_STRIDE;
    auto gran = [&](int dst, int src_rank, int g) {
      return reinterpret_cast<unsigned long long*>(x.mbox[dst] + x.gran_off) + (size_t)src_rank * GRAN + g;
    };
    unsigned int* err = reinterpret_cast<unsigned int*>(x.mbox[x.rank] + x.err_off);
    if (tid < m) {   // this rank's value of entry (tid, kk), to every rank
      const unsigned long long g = ((unsigned long long)x.seq << 32) | __float_as_uint(gta);
      for (int r = 0; r < x.world; ++r) __hip_atomic_store(gran(r, x.rank, tid * k + kk), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // thread (row, r): rank r's value of entry row (< m), or (rows m, m + 1) the low / high half of rank r's row sum kk of its new H block
    const int row = tid >> 4, r_of = tid & 15;
    if (row < m + 2) {   // (whole waves: 16 threads per row, 4 rows per wave)
      const bool polls = r_of < x.world;
      const int g_idx = row < m ? row * k + kk : 34 * x.nfl + 2 * (ESPM_HS_ROWSUM + kk) + (row - m);
      unsigned int got = 0;
      const long long t0 = wall_clock64();
      for (;;) {
        const unsigned long long v = polls ? __hip_atomic_load(gran(x.rank, r_of, g_idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ((unsigned long long)x.seq << 32);
        const bool ok = (unsigned int)(v >> 32) == x.seq;
        got = (unsigned int)v;
        if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
        if (wall_clock64() - t0 > x.max_ticks) {
          if (!ok) atomicAdd(err, 1u);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      s_got[row][r_of] = got;
    }
    __syncthreads();
    gta = 0.f;
    rs = 0.0;
    for (int r = 0; r < x.world; ++r) {   // rank order: the same sums on every rank
      if (tid < m) gta += __uint_as_float(s_got[tid][r]);
      rs += __builtin_bit_cast(double, ((unsigned long long)s_got[m + 1][r] << 32) | s_got[m][r]);
    }
  } else {
    rs = a.hstat[ESPM_HS_ROWSUM + kk];
  }
  if (tid < m) {   // updates.py:58-60, :70-76
    const float num = wo * gta, den = s_csg[tid] * (float)rs;
    float wn = fmaxf(num / den, a.log_shift);
    if (fx >= 0.f) wn = fx;
    __hip_atomic_store(a.w_new + tid * k + kk, wn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (sc1: the finisher reads it in this launch)
    s_w[tid] = wn;
  }
  __syncthreads();
  // the column of G W' (updates.py:107 of the next half step), stored / xscale with a positive floor; padding channels: X = 0 there
  const float inv_scale = 1.f / a.xscale;
#pragma unroll
  for (int u = 0; u < GC_CPT; ++u) {
    const int c = tid + GC_THREADS * u;
    if (c < a.n_pad) {
      float v = 1.f;
      if (c < a.n) {
        float row = 0.f;
#pragma unroll
        for (int mm = 0; mm < GC_MMAX; ++mm)
          if (mm < m) row = fmaf(gv[mm][u], s_w[mm], row);
        v = fmaxf(row, a.gw_floor) * inv_scale;
      }
      a.gw_s[(size_t)c * KP + kk] = v;
    }
  }
  if (wave == 0) {   // (the threads that stored W'[:, kk] are this wave's: its drain covers them)
    double cs = 0.0;
    float swf = 0.f;
    if (lane == 0) {
      for (int mm = 0; mm < m; ++mm) {
        cs += (double)s_csg[mm] * (double)s_w[mm];   // colsum(G W')[kk] = colsum(G)^T W'[:, kk] (round 4: DESIGN.md section 2)
        swf += s_w[mm];
      }
      a.colsum_gw[kk] = cs;
    }
    if (a.hist_slot) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(colgran + kk, ((unsigned long long)nonce << 32) | __float_as_uint(swf), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// the two-launch form applies: nothing global in W' but the row sums of H'
// (scratch: w_scratch's 2 m k floats must hold the second launch's partial column sums and its ticket - zero between launches)
bool w_gsplit_applies(const WFinishArgs& args) {
  const long mk = (long)args.m * args.k;
  const int nwg_b = (args.n_pad + 255) / 256;
  if (!(args.g && args.g_t && args.m > 0 && args.update_w && !args.simplex_w && args.pg_gamma_w <= 0.f && !args.breg_sr && mk <= 8192 && args.scratch &&
        (size_t)2 * mk * sizeof(float) >= (size_t)nwg_b * KP * sizeof(double) + 16))
    return false;
  static const bool enabled = w_env_knob("ESPM_W_GSPLIT", true);
  return enabled;
}
static unsigned int w_gcol_nonce() {
  static std::atomic<unsigned int> count{0};
  unsigned int v = ++count;
  if (v == 0) v = ++count;   // (0 is what a zeroed scratch holds)
  return v;
}
int launch_w_gcol(const WFinishArgs& f, hipStream_t stream) {
  WGxchgArgs x = {};
  x.f = f;
  x.world = 1;
  x.max_ticks = W_WAIT_MAX_TICKS;
  hipLaunchKernelGGL(w_gcol_kernel<false>, dim3(f.k + 1), dim3(GC_THREADS), 0, stream, x, w_gcol_nonce());
  return check_hip(hipGetLastError(), "w_finish (dictionary G, by columns)");
}

int launch_w_gfinish_gw(const WFinishArgs& args, hipStream_t stream) {
  const int nwg_b = (args.n_pad + 255) / 256;
  hipLaunchKernelGGL(w_gfinish_gw_kernel, dim3(nwg_b + 1), dim3(256), (size_t)args.m * args.k * sizeof(float), stream, args);
  return check_hip(hipGetLastError(), "w_finish (dictionary G: rows of G W')");
}

int launch_w_gxchg_update(const WFinishArgs& f, const espm_xchg* xc, unsigned int seq, const double* hstat_local, double* hstat_out,
                          const float* h_new, int nx, int ny, int p_pad, int with_halo, hipStream_t stream) {
  WGxchgArgs x;
  x.f = f;
  const int mk = f.m * f.k;
  ESPM_REQUIRE((size_t)mk <= (size_t)34 * xc->wgflags, "exchange: %d entries of G^T A, the mailbox holds granules for %d", mk, 34 * xc->wgflags);
  if (int rc = fill_w_mailbox_args(x, xc, seq, f, h_new, nx, ny, p_pad, with_halo)) return rc;
  x.hstat_local = hstat_local;
  x.hstat_out = hstat_out;
  if (w_gcol_applies(f)) {   // one launch: G^T A by columns, the exchange, W', the columns of G W' (w_gcol_kernel)
    hipLaunchKernelGGL(w_gcol_kernel<true>, dim3(f.k + 2), dim3(GC_THREADS), 0, stream, x, w_gcol_nonce());
    return check_hip(hipGetLastError(), "w_gcol (exchange) launch");
  }
  hipLaunchKernelGGL(w_gxchg_update_kernel, dim3(mk + 1), dim3(256), 0, stream, x);
  if (int rc = check_hip(hipGetLastError(), "w_gxchg_update launch")) return rc;
  return launch_w_gfinish_gw(f, stream);
}

// launch_w_finish's: the form that plan_w_dict chose
int launch_w_dict_finish(const WFinishArgs& args, int form, hipStream_t stream) {
  if (form == ESPM_W_FORM_DICT_COLUMNS) return launch_w_gcol(args, stream);
  hipLaunchKernelGGL(w_gfinish_update_kernel, dim3((unsigned)args.m * args.k), dim3(256), 0, stream, args);
  if (int rc = check_hip(hipGetLastError(), "w_finish (dictionary G: update)")) return rc;
  return launch_w_gfinish_gw(args, stream);
}

}  // namespace espm
