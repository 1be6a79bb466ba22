// What lies where in a workgroup's LDS for the three launches of the sparse count store - the H-step (mu_ell.hip), its chained form
// (mu_h_chain.hip) and the fused half-steps (mu_fused.hip) - and for the fused launch which instance runs: the host arithmetic of
// those launchers in one place, in the manner of mu_w_plan.hpp.  No kernel and no HIP call in the plans: the launchers compute a
// plan, copy it into the argument block, grant the LDS (allow_lds below, the one HIP call of this header) and launch; the predicates
// (ell_chain_fits, fused_ell_lds_bytes and through it espm_mu_fused_applies) and the size query of include/espm_mu.h
// (espm_mu_ell_h_lds_bytes, which espm_amd/ell.py and the store choice ask) read the same plans, so what admits a launch cannot
// drift from what lays it out.  tests/test_ell_plan_cpu.py runs the launchers against a stubbed runtime and pins every field.
// The sizes of the kernels' own structures - FusedGeom<K>::S / S_MAX / PROWS, FixTab<K>::bytes / MAX_ROWS, EllTab<K>::FLOATS - stay
// with the kernels; the plans are templates on K for that reason ("LDS of the sparse store's launches").
#pragma once
#include <stdio.h>

#include "mu_fused_kernel.hpp"

// the full geometry: the block's permutations in LDS (mu_fused_kernel.hpp) when they fit next to the tables.  Measured: no
// gain at the headline (150.1 against 146.9-150.2 us per iteration, profiles/r03a_variant_ab_512.log: with four waves per SIMD
// a unit's start - 4 of them per wave and walk - is covered by the other waves) - off.
#ifndef ESPM_FUSED_FULL_PERM_LDS
#define ESPM_FUSED_FULL_PERM_LDS 0
#endif
#ifndef ESPM_FUSED_PLAIN   // the lean instance of the common case (mu_fused_plain.hip); ESPM_FUSED_PLAIN=0 in the environment keeps the generic one (A/B)
#define ESPM_FUSED_PLAIN 1
#endif

namespace espm {

// dynamic LDS above 64 KB has to be granted per kernel (once); ESPM_ELL_LDS_MAX is a workgroup's LDS on gfx950
template <typename KernelT>
static int allow_lds(KernelT kern, size_t bytes, const char* what) {
  if (bytes <= 64 * 1024) return ESPM_OK;
  if (bytes > ESPM_ELL_LDS_MAX) return set_error(ESPM_EUNSUPPORTED, "%s: %zu bytes of LDS exceed %d", what, bytes, ESPM_ELL_LDS_MAX);
  return check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), what);
}

// ---- the sparse H-step (h_step_ell_kernel) and its chained instance ---------------------------------------------------------------
// In order: the G W table (n_pad rows of EllTab<K>::FLOATS floats, address 0); one region for the partial numerators, which the
// record reduction and then the extra workgroup's scratch (the tail of the W update; chained: the finalize) reuse; then
//   plain:   the workgroup's copy of colsum(GW') where cs_parts is given - KP doubles behind the region or, where table and region
//            take the LDS to the last byte (16 components at 2048 channels: 128 + 32 KB), cs_lds_off = 0: the table's first bytes
//            once the walk is over and the table dead (the kernel: cs_late);
//   chained: the 8 k doubles of the row sums and maxima the workgroup reduces from the previous launch's records (chain_lds_off).
//            The chained launch carries no tail of a W update: cs_parts is not looked at and cs_lds_off stays the caller's.
inline size_t chain_scr_bytes(int k) { return (size_t)8 * k * sizeof(double); }   // (the dense stores' chained H-step puts the same behind its LDS: mu_h_chain.hip)
struct EllHPlan {
  size_t bytes;        // dynamic LDS of the launch
  int cs_lds_off;      // plain with cs_parts: HStepArgs::cs_lds_off (0: cs_late); else -1, the argument block keeps its value
  int chain_lds_off;   // chained: HStepArgs::chain_lds_off, chain_scr_bytes(K) from there to the end; else -1
  bool fits;           // bytes <= ESPM_ELL_LDS_MAX
};
template <int K>
inline EllHPlan plan_h_ell(int n_pad, int tile_px, bool cs_parts, bool chained) {
  const size_t red = (size_t)(ESPM_ELL_TILE / 64 + 1) * (ESPM_HP_NSCALAR + 2 * K + 1) * sizeof(double);
  // [nsplit][K][tile_px]: K * 512 floats whatever the split; two such sets when the groups of a 512-pixel window are walked in pairs
  size_t part = (size_t)K * ESPM_ELL_TILE * sizeof(float) * ((K <= ESPM_ELL_PAIR_MAX_K && tile_px == ESPM_ELL_TILE) ? 2 : 1);
  if (red > part) part = red;
  // the extra workgroup's scratch, at the start of the region: the W update's tail, or the chain's finalize
  const size_t extra = chained ? (size_t)4 * H_FINALIZE_NV * sizeof(double) : (size_t)((ESPM_ELL_TILE / 64 + 1) * (KP + 1) + 1) * sizeof(double);
  if (extra > part) part = extra;
  EllHPlan pl = {(size_t)n_pad * EllTab<K>::FLOATS * sizeof(float) + part, -1, -1, false};
  if (chained) {
    pl.chain_lds_off = (int)pl.bytes;
    pl.bytes += chain_scr_bytes(K);
  } else if (cs_parts) {
    if (pl.bytes + KP * sizeof(double) <= ESPM_ELL_LDS_MAX) {
      pl.cs_lds_off = (int)pl.bytes;
      pl.bytes += KP * sizeof(double);
    } else {
      pl.cs_lds_off = 0;
    }
  }
  pl.fits = pl.bytes <= ESPM_ELL_LDS_MAX;
  return pl;
}

// ---- the fused half-steps (mu_fused_ell_kernel) --------------------------------------------------------------------------------------
// In order: the table region (FixTab<K>::bytes of max(n_pad, pb) rows: G W for the H walk, then H' of the block's pb pixels for
// the W walk); the numerators' region (h_segs partial sets of PROWS x pb floats, at least the record reduction's and the shared
// tail's scratch; from the epilogue's barrier on the block's slab of k n_pad floats where slab_lds); the two unit counters and the
// units' KL sums (cnt_lds_off); the block's list offsets (meta_lds_off); below the full geometry the block's pix_perm and chan_perm
// (perm_lds_off, perm_lds); the scratch of the one-barrier record reduction (red_lds_off) - in the part of the table region that is
// dead by then (behind the H' table's pb rows) where the segment search asked for that and the region is long enough, else behind
// the permutations where the 160 KB still hold it, else none (< 0: the numerators' region after a barrier of its own); and the
// workgroup's copy of colsum(GW') and of the sums of W' where cs_parts is given (cs_lds_off: always behind, 2 KP doubles).
enum FusedInstance {   // which instance runs: one of the three kinds, | FUSED_FULL (blocks of ESPM_ELL_PB pixels) | FUSED_LOSS
  FUSED_GENERIC = 0,        // mu_fused_ell_kernel as mu_fused.hip instantiates it
  FUSED_PLAIN = 1,          // the lean instance of the common case (mu_fused_plain.hip)
  FUSED_PLAIN_STREAM = 2,   // ... that loads the lists without allocating in the last-level cache (mu_fused_stream.hip; the full geometry only)
  FUSED_KIND = 3,
  FUSED_FULL = 4,
  FUSED_LOSS = 8
};
struct FusedPlan {
  int refusal;      // ESPM_OK, or the status the launch returns with `why` as its text
  char why[192];
  size_t bytes;     // dynamic LDS of the launch
  int instance;     // FusedInstance
  // FusedArgs' fields of the same names, and h.cs_lds_off / h.tail_on
  int cnt_lds_off, meta_lds_off, perm_lds_off, red_lds_off, perm_lds, h_segs, w_split, slab_lds, cs_lds_off, tail_on;
  void apply(FusedArgs& a) const {
    a.cnt_lds_off = cnt_lds_off, a.meta_lds_off = meta_lds_off, a.perm_lds_off = perm_lds_off, a.red_lds_off = red_lds_off;
    a.perm_lds = perm_lds, a.h_segs = h_segs, a.w_split = w_split, a.slab_lds = slab_lds, a.h.cs_lds_off = cs_lds_off, a.h.tail_on = tail_on;
  }
};
#define ESPM_PLAN_REFUSE(pl, code, ...) \
  return (pl).refusal = (code), snprintf((pl).why, sizeof((pl).why), __VA_ARGS__), (pl)

// segments per list group of the H walk at the least: below the full geometry 1024 / pb (16 units), at the full geometry FusedGeom<K>::S
template <int K>
inline int fused_floor_segs(int pb) { return pb == ESPM_ELL_PB ? FusedGeom<K>::S : ESPM_ELL_PB / pb; }
// the numerators' region for `segs` segments
template <int K>
inline size_t fused_part(int segs, int pb) {
  const size_t red = (size_t)(ESPM_ELL_WTHREADS / 64 + 1) * (ESPM_HP_NSCALAR + 2 * K + 1) * sizeof(double);
  const size_t tail_scratch = (size_t)((ESPM_ELL_WTHREADS / 64 + 1) * (KP + 1) + 1) * sizeof(double);
  size_t part = (size_t)segs * FusedGeom<K>::PROWS * pb * sizeof(float);
  if (red > part) part = red;
  if (tail_scratch > part) part = tail_scratch;
  return part;
}
// the workgroup's LDS with `part` bytes for the numerators' region: sets the offsets of `pl`, returns the bytes.  red_in_table: the
// scratch of the record reduction in the part of the table region that is dead by then - the G W table is read by the H walk only,
// the H' table of the W walk occupies the first pb rows' worth of it (mu_fused_kernel.hpp) - where the region is long enough;
// otherwise (and by default) behind the permutations.  red_scratch = false: without that scratch (the floor, fused_floor_bytes).
template <int K>
inline size_t fused_layout(FusedPlan& pl, int pb, int tab_rows, int n_cg, bool cs_parts, size_t part, bool red_in_table, bool red_scratch = true) {
  const size_t red_own = (size_t)(ESPM_ELL_WTHREADS / 64) * (ESPM_HP_NSCALAR + 2 * K + 1) * sizeof(double);   // the one-barrier record reduction's scratch
  const size_t tab_bytes = FixTab<K>::bytes(tab_rows);   // (float4 parts from address 0, components 4.. from ESPM_TAB2_BASE: mu_h_kernel.hpp)
  size_t bytes = tab_bytes + part;
  pl.cnt_lds_off = (int)bytes;   // the two unit counters, then the units' KL sums
  bytes += 16 + ESPM_FUSED_MAX_UNITS * sizeof(float);
  pl.meta_lds_off = (int)bytes;  // the block's list offsets
  bytes += (size_t)(3 * (pb / 64) + 2 * n_cg + 1 + 3) / 4 * 16;
  pl.perm_lds_off = (int)bytes;  // below the full geometry: the block's pix_perm and chan_perm
  const size_t perm_bytes = (size_t)(pb + 64 * n_cg) * sizeof(int);
  // (the full geometry: the copies are an extra where the workgroup's 160 KB still hold them)
  pl.perm_lds = pb != ESPM_ELL_PB || (ESPM_FUSED_FULL_PERM_LDS && bytes + perm_bytes + KP * sizeof(double) <= ESPM_ELL_LDS_MAX);
  if (pl.perm_lds) bytes += perm_bytes;
  pl.red_lds_off = -1;
  const size_t hp_tab = FixTab<K>::bytes(pb);   // (the end of the H' table's last part: what lies behind it up to tab_bytes held rows pb.. of G W)
  if (ESPM_FUSED_RED_ONE_BARRIER && red_scratch && red_in_table && hp_tab + red_own <= tab_bytes) {
    pl.red_lds_off = (int)hp_tab;
  } else if (ESPM_FUSED_RED_ONE_BARRIER && red_scratch && bytes + red_own + 2 * KP * sizeof(double) <= ESPM_ELL_LDS_MAX) {
    bytes = (bytes + 7) / 8 * 8;
    pl.red_lds_off = (int)bytes;
    bytes += red_own;
  }
  if (cs_parts) {   // the workgroup's own copy of colsum(GW'): k doubles behind the numerators (and, for the shared tail, the sums of W')
    bytes = (bytes + 7) / 8 * 8;
    pl.cs_lds_off = (int)bytes;
    bytes += 2 * KP * sizeof(double);
  }
  return bytes;
}

// What launch_fused_k lays out and runs for these arguments.  env_plain, env_small_segs: the A/B switches of the environment
// (ESPM_FUSED_PLAIN, ESPM_FUSED_SMALL_SEGS), which the launcher reads once per process.
template <int K>
inline FusedPlan plan_fused(const FusedArgs& args, bool env_plain, int env_small_segs) {
  FusedPlan pl = {};
  pl.cs_lds_off = args.h.cs_lds_off, pl.tail_on = args.h.tail_on;
  const int pb = args.w.pb;
  const int tab_rows = args.h.n_pad > pb ? args.h.n_pad : pb;
  const bool full = pb == ESPM_ELL_PB;
  if (!(K <= 4 || tab_rows <= FixTab<K>::MAX_ROWS))
    ESPM_PLAN_REFUSE(pl, ESPM_EINVAL, "fused half-steps: a table of %d rows, at most %d from 5 components on", tab_rows, FixTab<K>::MAX_ROWS);
  size_t bytes = 0;
  auto layout = [&](size_t part, bool red_in_table) { bytes = fused_layout<K>(pl, pb, tab_rows, args.w.n_cg, args.h.cs_parts != nullptr, part, red_in_table); };
  // segments per list group of the H walk: below the full geometry 1024 / pb (16 units); at the full geometry as many as fit, S_MAX down to S
  pl.h_segs = fused_floor_segs<K>(pb);
  size_t part0 = fused_part<K>(pl.h_segs, pb);
  bool red_in_table = false;
  if (full) {
    for (int segs = FusedGeom<K>::S_MAX; segs > FusedGeom<K>::S; --segs) {
      bool ok = false;
      for (int rit = 0; rit < 2 && !ok; ++rit) {
        layout(fused_part<K>(segs, pb), rit != 0);
        ok = bytes <= ESPM_ELL_LDS_MAX && pl.red_lds_off >= 0;
        if (ok) red_in_table = rit != 0;
      }
      if (ok) {
        pl.h_segs = segs;
        part0 = fused_part<K>(segs, pb);
        break;
      }
    }
  }
  // the slab of the block collected in the numerators' region (mu_fused_kernel.hpp, ESPM_FUSED_SLAB_LDS): needs that region to itself from
  // the epilogue's barrier on (the record reduction's scratch elsewhere) and k n_pad floats of it - below the full geometry the
  // region is grown to that where the workgroup's LDS allows
  const size_t slab = (size_t)K * args.w.n_pad * sizeof(float);
  pl.slab_lds = 0;
  layout(part0, red_in_table);
  pl.w_split = 0;
  if (ESPM_FUSED_SLAB_LDS && args.w.n_pad % 4 == 0) {
    if (slab > part0) {
      layout(slab, false);
      if (bytes > ESPM_ELL_LDS_MAX || pl.red_lds_off < 0) {
        layout(part0, red_in_table);
      } else {
        pl.slab_lds = 1;
        // the region grown for the slab holds more partial sets than 1024 / pb: more (group, segment) units than waves, so that the
        // units handed out last level the waves (ESPM_FUSED_SMALL_SEGS: A/B; 0 keeps 1024 / pb)
        const int want = env_small_segs;
        const int fit = (int)(slab / ((size_t)FusedGeom<K>::PROWS * pb * sizeof(float)));
        int segs = want > 0 ? want : pl.h_segs;
        if (segs > fit) segs = fit;
        if (segs > ESPM_FUSED_MAX_SEGS) segs = ESPM_FUSED_MAX_SEGS;
        if (segs > pl.h_segs) pl.h_segs = segs;
      }
    } else {
      pl.slab_lds = pl.red_lds_off >= 0;
      // the full geometry: two copies of the slab where the region holds them - the W walk then hands out half channel groups
      pl.w_split = ESPM_FUSED_W_SPLIT && pl.slab_lds && pb == ESPM_ELL_PB && 2 * slab <= part0;
    }
  }
  // the tail of the previous W update is shared by the launch's own workgroups (mu_fused_kernel.hpp) unless it carries the
  // projected gradient's quadratic term, which only the extra workgroup sums
  if (pl.tail_on && !args.h.tail.pg_q) pl.tail_on = 2;
  pl.bytes = bytes;
  if (bytes > ESPM_ELL_LDS_MAX) ESPM_PLAN_REFUSE(pl, ESPM_EUNSUPPORTED, "fused half-steps: %zu bytes of LDS exceed %d", bytes, ESPM_ELL_LDS_MAX);
  // the common case as its own, leaner instance (mu_fused_kernel.hpp: PLAIN; instantiated in mu_fused_plain.hip): every fact the
  // kernel takes for granted is checked here
  const int NT = ESPM_ELL_WTHREADS;
  const int n_perm = pl.perm_lds ? pb + 64 * args.w.n_cg : 0, n_woff = 2 * args.w.n_cg + 1;
  const bool staged_ok = args.h.n_pad <= 4 * NT && n_perm <= 4 * NT && n_woff <= NT && args.h.cs_nbk <= 64 && 2 * K <= NT / 64;
  const bool plain = ESPM_FUSED_PLAIN && env_plain && !args.h.fixed_h && !args.h.fill_num && !args.h.breg_sr && !args.h.l2_m &&
                     args.h.simplex_h && args.h.lambda_l != 0.f && args.h.grid_mode && args.h.have_prev && args.h.write_h && args.h.h_rule == 0 &&
                     pl.tail_on != 1 && !args.static_units && pl.slab_lds && !pl.w_split && pl.red_lds_off >= 0 && staged_ok &&
                     (pl.perm_lds != 0) == (pb != ESPM_ELL_PB) && ESPM_FUSED_SMALL_THREADS == ESPM_ELL_WTHREADS;
  if (plain && !(!(EllImplicit<K>::ON && args.h.compute_loss) || args.h.ell_blk_cnt))
    ESPM_PLAN_REFUSE(pl, ESPM_EINVAL, "fused half-steps at %d components with the loss: espm_mu_state.ell_blk_cnt is missing (espm_mu_ell_block_counts)", K);
  // (the lists too large for the last-level cache, the caller says: the instance that loads them without allocating there)
  pl.instance = (plain ? (args.stream_lists && pb == ESPM_ELL_PB ? FUSED_PLAIN_STREAM : FUSED_PLAIN) : FUSED_GENERIC) | (full ? FUSED_FULL : 0) |
                (args.h.compute_loss ? FUSED_LOSS : 0);
  return pl;
}

// The least LDS a fused launch of (n_pad, k, pb) takes, which fused_ell_lds_bytes answers (mu_fused.hip): the layout at the floor -
// fused_floor_segs segments, cs_parts given, no reduction scratch of its own, the permutations in LDS below the full geometry -
// for the most channel groups an n of this n_pad has.  (size_t)-1 where the launch is refused whatever the rest.
// FUSED_FLOOR_SLACK: fused_ell_lds_bytes has always allowed 8 bytes for an alignment the layout never needs (every term is a
// multiple of 8); they stay, so that no (n_pad, k, pb) starts to fuse that did not before.
constexpr size_t FUSED_FLOOR_SLACK = 8;
template <int K>
inline size_t fused_floor_bytes(int n_pad, int pb) {
  const int tab_rows = n_pad > pb ? n_pad : pb;
  if (!(K <= 4 || tab_rows <= FixTab<K>::MAX_ROWS)) return (size_t)-1;
  FusedPlan pl = {};
  return fused_layout<K>(pl, pb, tab_rows, (n_pad + 63) / 64, true, fused_part<K>(fused_floor_segs<K>(pb), pb), false, false) + FUSED_FLOOR_SLACK;
}

}  // namespace espm
