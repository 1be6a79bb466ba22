// Launcher of the fused half-steps of the sparse count store (mu_fused_kernel.hpp).
#include <stdlib.h>

#include "mu_ell_plan.hpp"

#ifndef ESPM_ELL_UNR_H
#define ESPM_ELL_UNR_H 4
#endif
#ifndef ESPM_FUSED_SMALL_UNR_H   // list dwords per batch in the run-time-sized instance (shards, small images): A/B knob (code size against rows in flight)
#define ESPM_FUSED_SMALL_UNR_H ESPM_ELL_UNR_H
#endif
#ifndef ESPM_FUSED_SMALL_UNR_W
#define ESPM_FUSED_SMALL_UNR_W ESPM_ELL_UNR_W
#endif
#ifndef ESPM_ELL_UNR_W
#define ESPM_ELL_UNR_W 4
#endif

#ifndef ESPM_FUSED_SMALL_SEGS_DEFAULT       // below the full geometry: segments per list group where the LDS holds them (0: 1024 / pb)
#define ESPM_FUSED_SMALL_SEGS_DEFAULT 0
#endif

namespace espm {

// The A/B switches of the environment, read ONCE per process (a lookup per launch sat inside espm_mu_iterate's loop, raced
// with a setenv from another thread and could change the kernel instance in the middle of a fit).
static bool fused_env_plain() {
  static const bool on = [] {
    const char* env = getenv("ESPM_FUSED_PLAIN");
    return !(env && env[0] == '0');
  }();
  return on;
}
static int fused_env_small_segs() {
  static const int want = [] {
    const char* env = getenv("ESPM_FUSED_SMALL_SEGS");
    return env ? atoi(env) : ESPM_FUSED_SMALL_SEGS_DEFAULT;
  }();
  return want;
}

int launch_fused_plain(const FusedArgs& args, int k, bool loss, bool full, int nblk, size_t lds_bytes, hipStream_t stream);   // mu_fused_plain.hip
int launch_fused_plain_stream(const FusedArgs& args, int k, bool loss, bool full, int nblk, size_t lds_bytes, hipStream_t stream);   // mu_fused_stream.hip
#ifdef ESPM_PHASE_CLOCK
int phase_buffer_plain(unsigned long long* p);
int phase_buffer_plain_stream(unsigned long long* p);
#endif

#if ESPM_MIN_K <= 8
// compute the plan (mu_ell_plan.hpp), copy it into the arguments, grant the LDS, switch on the instance
template <int K>
static int launch_fused_k(const FusedArgs& args_in, int nblk, hipStream_t stream) {
  const FusedPlan pl = plan_fused<K>(args_in, fused_env_plain(), fused_env_small_segs());
  if (pl.refusal) return set_error(pl.refusal, "%s", pl.why);
  FusedArgs args = args_in;
  pl.apply(args);
  const bool loss = pl.instance & FUSED_LOSS, full = pl.instance & FUSED_FULL;
  switch (pl.instance & FUSED_KIND) {
    case FUSED_PLAIN_STREAM: return launch_fused_plain_stream(args, K, loss, true, nblk, pl.bytes, stream);
    case FUSED_PLAIN: return launch_fused_plain(args, K, loss, full, nblk, pl.bytes, stream);
  }
  auto go = [&](auto kern, int threads) -> int {
    if (int rc = allow_lds(kern, pl.bytes, "fused half-steps")) return rc;
    hipLaunchKernelGGL(kern, dim3(nblk + (args.h.tail_on == 1 ? 1 : 0)), dim3(threads), pl.bytes, stream, args);
    return check_hip(hipGetLastError(), "fused half-steps launch");
  };
  if (full)   // the full geometry: 16 waves, sizes known at compile time
    return loss ? go(mu_fused_ell_kernel<K, true, ESPM_ELL_UNR_H, ESPM_ELL_UNR_W, ESPM_ELL_WTHREADS, true>, ESPM_ELL_WTHREADS)
                : go(mu_fused_ell_kernel<K, false, ESPM_ELL_UNR_H, ESPM_ELL_UNR_W, ESPM_ELL_WTHREADS, true>, ESPM_ELL_WTHREADS);
  return loss ? go(mu_fused_ell_kernel<K, true, ESPM_FUSED_SMALL_UNR_H, ESPM_FUSED_SMALL_UNR_W, ESPM_FUSED_SMALL_THREADS, false>, ESPM_FUSED_SMALL_THREADS)
              : go(mu_fused_ell_kernel<K, false, ESPM_FUSED_SMALL_UNR_H, ESPM_FUSED_SMALL_UNR_W, ESPM_FUSED_SMALL_THREADS, false>, ESPM_FUSED_SMALL_THREADS);
}
#endif

// LDS the fused kernel needs for (n_pad, k, pb) at the least (mu_ell_plan.hpp: fused_floor_bytes): the caller decides with it whether
// the fused path applies.  (size_t)-1: never, or k is not one of this build's
size_t fused_ell_lds_bytes(int n_pad, int k, int pb) {
  if (pb < 128 || pb > ESPM_ELL_PB || (pb & (pb - 1))) return (size_t)-1;
  switch (k) {
#define ESPM_X(KK) case KK: return fused_floor_bytes<KK>(n_pad, pb);
    ESPM_K_CASES(ESPM_X)
#undef ESPM_X
  }
  return (size_t)-1;
}

int launch_fused_ell(const HStepArgs& h, const WAccumArgs& w, int nblk, hipStream_t stream, int static_units, int stream_lists) {
  ESPM_REQUIRE(h.ell && h.ell_off && h.ell_klc && h.ell_pix && w.ell && w.ell_off && w.chan_perm, "fused half-steps: the sparse store's lists are missing");
  ESPM_REQUIRE(w.pb >= 128 && w.pb <= ESPM_ELL_PB && (w.pb & (w.pb - 1)) == 0 && 2 * h.ell_tp == w.pb && h.h_rule == 0 && h.write_h && !h.l2_m,
               "fused half-steps: blocks of two H tiles (tile_px=%d, ell_pb=%d), the default H rule, write_h", h.ell_tp, w.pb);
  ESPM_REQUIRE(nblk == (h.p + w.pb - 1) / w.pb && w.n_cg >= 1, "fused half-steps: nblk_w=%d must be ceil(p / %d)", nblk, w.pb);
  FusedArgs fa;
  fa.h = h;
  fa.w = w;
  fa.static_units = static_units;
  // stream_lists: espm_mu_state.ell_stream in bit 0 and, with it, the kept part of the streamed lists - ell_keep_h in bits 8..15, ell_keep_w in
  // bits 16..23 (list groups per tile, channel groups per block: checked by the caller, mu_api.hip); 0: plain loads, 1: every row non-temporal
  ESPM_REQUIRE(stream_lists >= 0 && stream_lists < (1 << 24) && ((stream_lists & 1) || stream_lists == 0), "fused half-steps: stream_lists=%d", stream_lists);
  fa.stream_lists = (unsigned char)(stream_lists & 1);
  fa.keep_h = (unsigned char)((stream_lists >> 8) & 255);
  fa.keep_w = (unsigned char)((stream_lists >> 16) & 255);
  fa.keep_pad = 0;
  switch (h.k) {
#if ESPM_MIN_K <= 8
#define ESPM_X(KK) case KK: return launch_fused_k<KK>(fa, nblk, stream);
    ESPM_K_CASES(ESPM_X)
#undef ESPM_X
#endif
  }
  return set_error(ESPM_EUNSUPPORTED, "fused half-steps: k=%d not built", h.k);
}

}  // namespace espm

#ifdef ESPM_PHASE_CLOCK
// debug build only (tools/analysis/phase_clock.py): where the fused kernel's workgroups write their phase stamps (8 x uint64 per workgroup)
extern "C" int espm_debug_phase_buffer(void* dev_ptr) {
  unsigned long long* p = static_cast<unsigned long long*>(dev_ptr);
  if (int rc = espm::phase_buffer_plain(p)) return rc;
  if (int rc = espm::phase_buffer_plain_stream(p)) return rc;
  return espm::check_hip(hipMemcpyToSymbol(HIP_SYMBOL(espm::espm_phase_buf), &p, sizeof(p)), "phase buffer");
}
#endif
