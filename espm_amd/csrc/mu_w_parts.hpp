// W update of the SmoothNMF multiplicative rule.
//
// espm/estimators/updates.py:38-76 computes  W' = max( W * (G^T (X / (GWH)) H^T) / (colsum(G) rowsum(H)^T + nu), eps ).
// Here the (n, p) ratio R = X / (GW H) is never stored and the association is G^T (R H^T):
//   w_accum : A_b = sum_{j in pixel block b} R[:, j] H[:, j]^T      lanes <-> channels, X pixel-major,
//             one 16-byte coalesced load per lane and pixel, H[:, j] wave-uniform (scalar cache),
//             the contraction over pixels accumulates in registers - no cross-lane traffic.
//   w_reduce: A = sum_b A_b in fixed order (bit-reproducible, unlike float atomics).
//   w_finish: numerator / denominator, optional simplex over the columns of W with the reference's
//             global-stop bisection (dicotomy.py:111-173), clamp, fixed_W, then GW = G W for the
//             next half step, its column sums, and rel_W (base.py:323).
//
// The units: mu_w_accum.hip (w_accum on the dense stores), mu_w_reduce.hip (w_reduce and the many-workgroup updates of W with
// G = identity), mu_w_exchange.hip (the same inside a sharded image's record exchange), mu_w_finish.hip (the one-workgroup w_finish),
// mu_w_dict.hip (a dictionary G, sharded or not).  This header holds what more than one of them needs; mu_common.hpp declares their launchers.
#pragma once
#include <stdlib.h>

#include "mu_common.hpp"
#include "mu_w_plan.hpp"
#include "mu_xchg.hpp"

namespace espm {

// The arguments of a many-workgroup update of W with G = identity (mu_w_reduce.hip, mu_w_exchange.hip): the head comment of
// w_reduce_update_kernel says what the sources and the records are.
struct WUpdateArgs {
  const unsigned char* src;
  size_t src_stride;
  int nsrc, n, n_pad, k, nbk;
  float* a_out;
  const double* hpart;          // slab mode: H-step records (field-major), nblk_h of them
  const double* hstat_rs;       // slab mode without a riding finalize: the statistics of the new H are already reduced
  int nblk_h;
  size_t rec_hstat_off;         // records mode (hpart == null): byte offset of the 16 statistics inside a record
  double* hstat_out;            // records mode: global row sums / maxima of the new H
  const float* w_old;
  float* w_new;
  const float* fixed_w;
  const float* breg_sr;         // Bregman variant (updates.py:40-48): per-channel sums of the stored X, else null
  float pg_gamma_w;             // > 0: projected-gradient step (updates.py:353-370)
  int pg_track;                 // its linesearch term goes to parts[2 nwg + workgroup]
  float* gw_s;
  double* parts;                // [2][k * nbk]: partial column sum of G W' (component of the workgroup), partial sum of W'
  float log_shift, gw_floor, xscale;
  int fuse_finalize;
  HFinalizeArgs fin;
};

// The update of the 32 entries of W (component kk, channels c of the lanes that own one) from their summed A and the row
// sum rs of the new H, by wave 0 of a reduction workgroup; the per-workgroup partials of what is global go to a.parts.
__device__ __forceinline__ void w_update_preload(const WUpdateArgs& a, int kk, int c, bool mine, float& wo, float& fx) {
  wo = 1.f;
  fx = -1.f;
  if (mine && c < a.n) {
    wo = a.w_old[(size_t)c * a.k + kk];
    if (a.fixed_w) fx = a.fixed_w[(size_t)c * a.k + kk];
  }
}
// wo_pre / fx_pre: the entry's old value and fixed value (negative: none), requested by the caller at its start - here they would
// be one more trip to memory at the end of a kernel that is nothing but latency.
__device__ __forceinline__ void w_update_entries(const WUpdateArgs& a, int kk, int c, int e, bool owns, float t, double rs, int nwg, int wg,   // wg: index of the reduction workgroup (its slot of the partials)
                                                 float wo_pre, float fx_pre) {
  double cs = 0.0, sw = 0.0, qw = 0.0;
  if (owns) {
    a.a_out[e] = t;
    if (c < a.n) {
      const float wo = wo_pre;
      float v;
      if (a.pg_gamma_w > 0.f) {  // W - grad / gamma with grad = rowsum(H) - (X / GWH) H^T (G = I), updates.py:353-362
        v = fmaxf(wo - ((float)rs - t) / a.pg_gamma_w, a.log_shift);
        const double dw = (double)v - (double)wo;   // (fixed_W is not part of a projected-gradient fit, smooth_nmf.py:430-437)
        qw = dw * (double)((float)rs - t) + (double)a.pg_gamma_w * dw * dw;
      } else if (a.breg_sr) {  // W' = sR W / ((rowsum(H) - (X / GWH) H^T) W + sR), updates.py:41-48
        const float sr = a.xscale * a.breg_sr[c];
        v = fmaxf((sr * wo) / (((float)rs - t) * wo + sr), a.log_shift);
      } else {
        v = fmaxf((wo * t) / (float)rs, a.log_shift);   // updates.py:59-60, :70-72 (G = I: colsum(G) = 1)
      }
      if (fx_pre >= 0.f) v = fx_pre;                        // updates.py:75-76
      a.w_new[(size_t)c * a.k + kk] = v;
      const float gv = fmaxf(v, a.gw_floor);
      a.gw_s[(size_t)c * KP + kk] = gv * (1.f / a.xscale);
      cs = (double)gv;
      sw = (double)v;
    } else {
      a.gw_s[(size_t)c * KP + kk] = 1.f;  // padding channels: X = 0 there
    }
  }
  cs = wave_sum(cs);
  sw = wave_sum(sw);
  if (a.pg_track) qw = wave_sum(qw);
  if (threadIdx.x == 0) {
    a.parts[wg] = cs;
    a.parts[nwg + wg] = sw;
    if (a.pg_track) a.parts[2 * nwg + wg] = qw;
  }
}

// What every launcher of such an update takes from the W finish's arguments: no sources, no H-step records and no riding record
// reduction yet - the launcher sets the ones it has.
static inline WUpdateArgs make_w_update_args(const WFinishArgs& f) {
  WUpdateArgs a = {};
  a.n = f.n;
  a.n_pad = f.n_pad;
  a.k = f.k;
  a.nbk = (f.n_pad + 31) / 32;
  a.w_old = f.w_old;
  a.w_new = f.w_new;
  a.fixed_w = f.fixed_w;
  a.breg_sr = f.breg_sr;
  a.pg_gamma_w = f.pg_gamma_w;
  a.pg_track = f.pg_q != nullptr;
  a.gw_s = f.gw_s;
  a.parts = reinterpret_cast<double*>(f.scratch);
  a.log_shift = f.log_shift;
  a.gw_floor = f.gw_floor;
  a.xscale = f.xscale;
  return a;
}

// The flag behind a record's stores (the ordering contract: mu_xchg.hip).  Default: a relaxed system-scope store - the data stores were
// write-through, every storing wave drained them (s_waitcnt vmcnt(0)) and the workgroup's barrier lies in between.  release != 0
// (ESPM_XCHG_ORDER=release, espm_xchg_set_order): the same store with release order at system scope - the compiler's full recipe
// (write back this XCD's L2, wait, store), by the flag-storing lanes only.
__device__ __forceinline__ void xchg_store_flag(unsigned int* flag, unsigned int seq, int release) {
  if (release) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  else __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void xchg_wait_flag(const unsigned int* flag, unsigned int seq, long long max_ticks, unsigned int* err) {
  const long long t0 = wall_clock64();
  while ((int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {   // (polling with acquire loads would invalidate the caches per poll)
    if (wall_clock64() - t0 > max_ticks) {
      atomicAdd(err, 1u);
      break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

constexpr long long W_WAIT_MAX_TICKS = 200000000LL;   // the bound of every wait inside a launch: 2 s of the 100 MHz wall clock

// The mailbox view of an in-launch exchange, for WExchangeArgs (mu_w_exchange.hip) or WGxchgArgs (mu_w_dict.hip): the two structs
// name these fields alike and keep them in their own order.  A record is the A block (k n_pad floats), the statistics of the new H
// and its two boundary rows; slot and granules are those of the sequence number's parity (mu_xchg.hpp).
template <typename Args>
static int fill_w_mailbox_args(Args& x, const espm_xchg* xc, unsigned int seq, const WFinishArgs& f, const float* h_new, int nx, int ny,
                               int p_pad, int with_halo) {
  for (int r = 0; r < 16; ++r) x.mbox[r] = r < xc->world ? xc->peers[r] : nullptr;
  for (int r = 0; r < xc->world; ++r) ESPM_REQUIRE(x.mbox[r], "exchange: rank %d is not connected (espm_xchg_connect)", r);
  x.world = xc->world;
  x.rank = xc->rank;
  x.nfl = xc->wgflags;
  x.with_halo = with_halo;
  x.rec_bytes = xc->record_bytes;
  x.slot_base = (size_t)(seq & 1u) * xc->world * xc->record_bytes;
  x.wgflags_off = xc->off_wgflags;
  x.gran_off = xc->off_gran + (size_t)(seq & 1u) * xc->world * ((size_t)34 * xc->wgflags + 2 * ESPM_HS_STRIDE) * sizeof(unsigned long long);
  x.err_off = xc->off_err;
  x.top_off = (size_t)f.k * f.n_pad * 4 + ESPM_HS_STRIDE * 8;
  x.bot_off = x.top_off + (size_t)f.k * (ny > 0 ? ny : 0) * 4;
  x.seq = seq;
  x.max_ticks = W_WAIT_MAX_TICKS;
  x.release = xc->order;
  x.halo_h = h_new;
  x.halo_k = f.k;
  x.halo_nx = nx;
  x.halo_ny = ny;
  x.halo_ppad = p_pad;
  return 0;
}

__device__ __forceinline__ double block_sum1(double v, double* scratch) {
  double a[1] = {v};
  block_reduce<1, 1>(a, scratch);
  __shared__ double bc;
  if (threadIdx.x == 0) bc = a[0];
  __syncthreads();
  return bc;
}
__device__ __forceinline__ double block_max1(double v, double* scratch) {
  double a[1] = {v};
  block_reduce<1, 0>(a, scratch);
  __shared__ double bc;
  if (threadIdx.x == 0) bc = a[0];
  __syncthreads();
  return bc;
}

#pragma GCC visibility push(hidden)   // between the units: not part of the library's interface
// mu_w_reduce.hip: the tail of a many-workgroup update, handed to the caller (it rides in a later launch) or launched here; the launches' status as `what`
int w_tail_defer_or_launch(const WFinishArgs& f, WTailArgs* defer_tail, hipStream_t stream, const char* what);
// mu_w_dict.hip: the W finish of a dictionary G as the many-workgroup form that plan_w_dict chose (mu_w_plan.hpp)
int launch_w_dict_finish(const WFinishArgs& args, int form, hipStream_t stream);
#pragma GCC visibility pop

}  // namespace espm
