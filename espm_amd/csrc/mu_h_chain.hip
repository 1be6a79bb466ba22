// Launchers of the CHAIN instances of the H-step kernels (mu_h_chain.hpp): the H-only iteration of espm_mu_iterate_h as one launch
// per iteration.  Built for the kernels an H-only iteration of the default rule runs by default: h_step_ell_kernel (sparse store; the
// pixels of heavy elements need launches of their own around it and keep the general path) and the vector h_step_kernel of the 8-bit,
// bf16 and fp32 stores below ESPM_H_CHAIN_MAX_K components (from there on the dense stores run the matrix-core H-step, which is not
// chained; neither is the 17..32 build).  Only the instances WITH the loss terms: espm_mu_iterate_h fills history rows.
// The build may compile this file ESPM_CHAIN_PARTS times, part ESPM_CHAIN_PART instantiating every ESPM_CHAIN_PARTS-th component count.
#include "mu_ell_plan.hpp"

#ifndef ESPM_H_CHAIN_MAX_K
#define ESPM_H_CHAIN_MAX_K 12   // = ESPM_H_MFMA_MIN_K - 1 (mu_h_step.hip)
#endif
#ifndef ESPM_ELL_UNR_H
#define ESPM_ELL_UNR_H 4
#endif
#ifndef ESPM_CHAIN_PARTS
#define ESPM_CHAIN_PARTS 1
#define ESPM_CHAIN_PART 0
#endif
#define ESPM_CAT2(a, b) a##b
#define ESPM_CAT(a, b) ESPM_CAT2(a, b)

namespace espm {

#if ESPM_KP <= 16

template <int K>
static int launch_chain_k(const HStepArgs& args_in, int x_dtype, int tile_px, int nblk, hipStream_t stream) {
  HStepArgs args = args_in;
  args.tail_on = args.chain_fin_on ? 1 : 0;   // (the extra workgroup is not a record: h_epilogue)
  const dim3 grid(nblk + args.tail_on);
  auto go = [&](auto kern, int threads, size_t bytes, const char* what) -> int {   // bytes: the kernel's own LDS; the chain's scratch goes behind
    args.chain_lds_off = (int)bytes;
    bytes += chain_scr_bytes(K);
    if (int rc = allow_lds(kern, bytes, what)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(threads), bytes, stream, args);
    return check_hip(hipGetLastError(), what);
  };
  if (x_dtype == ESPM_X_ELL) {
    constexpr int UNR = K > 8 ? 2 : ESPM_ELL_UNR_H;
    return go(h_step_ell_kernel<K, true, UNR, 0, true>, ESPM_ELL_TILE, plan_h_ell<K>(args.n_pad, args.ell_tp, false, true).chain_lds_off, "h_step (ell, chained)");
  }
  if constexpr (K <= ESPM_H_CHAIN_MAX_K) {
    auto dense = [&](auto k256, auto k128) -> int {
      const int px = tile_px == 256 ? 4 : 2, nw = tile_px == 256 ? 4 : 8;
      const size_t lds = (size_t)nw * K * 64 * px * sizeof(float);   // (>= the reduction's scratch and the extra workgroup's)
      if (tile_px == 256) return go(k256, 256, lds, "h_step (chained)");
      if (tile_px == 128) return go(k128, 512, lds, "h_step (chained)");
      return set_error(ESPM_EINVAL, "h_step (chained): tile_px %d not available", tile_px);
    };
    if (x_dtype == ESPM_X_U8) return dense(h_step_kernel<K, uint8_t, 4, 4, true, 8, 0, false, 0, true>, h_step_kernel<K, uint8_t, 2, 8, true, 8, 2, false, 0, true>);
    if (x_dtype == ESPM_X_BF16) return dense(h_step_kernel<K, bf16_t, 4, 4, true, 8, 0, false, 0, true>, h_step_kernel<K, bf16_t, 2, 8, true, 8, 2, false, 0, true>);
    return dense(h_step_kernel<K, float, 4, 4, true, 8, 0, false, 0, true>, h_step_kernel<K, float, 2, 8, true, 8, 2, false, 0, true>);
  }
  return set_error(ESPM_EUNSUPPORTED, "h_step (chained): %d components on a dense store are not built", K);
}

template <int KK>
static int launch_chain_part_k(const HStepArgs& args, int x_dtype, int tile_px, int nblk, hipStream_t stream) {
  if constexpr ((KK - ESPM_MIN_K) % ESPM_CHAIN_PARTS == ESPM_CHAIN_PART) return launch_chain_k<KK>(args, x_dtype, tile_px, nblk, stream);
  else return set_error(ESPM_EUNSUPPORTED, "h_step (chained): k=%d belongs to another part of the build", KK);
}

int ESPM_CAT(launch_h_chain_part, ESPM_CHAIN_PART)(const HStepArgs& args, int x_dtype, int tile_px, int nblk, hipStream_t stream) {
  switch (args.k) {
#define ESPM_X(KK) case KK: return launch_chain_part_k<KK>(args, x_dtype, tile_px, nblk, stream);
    ESPM_K_CASES(ESPM_X)
#undef ESPM_X
  }
  return set_error(ESPM_EUNSUPPORTED, "h_step (chained): k=%d not built", args.k);
}

#endif   // ESPM_KP <= 16

#if ESPM_CHAIN_PART == 0
#if ESPM_KP <= 16
int launch_h_chain_part1(const HStepArgs& args, int x_dtype, int tile_px, int nblk, hipStream_t stream);

template <int K>
static bool ell_chain_fits(int n_pad, int tile_px) { return plan_h_ell<K>(n_pad, tile_px, false, true).fits; }
#endif

bool h_chain_built(const espm_mu_state* st) {
#if ESPM_KP <= 16
  if (st->h_rule != 0 || st->breg_sr_px || !st->compute_loss || st->k < ESPM_MIN_K || st->k > ESPM_MAX_K) return false;
  if (st->x_dtype == ESPM_X_ELL) {
    if (st->ell_hv_n > 0) return false;
    switch (st->k) {
#define ESPM_X(KK) case KK: return ell_chain_fits<KK>(st->n_pad, st->tile_px);
      ESPM_K_CASES(ESPM_X)
#undef ESPM_X
    }
    return false;
  }
  return st->k <= ESPM_H_CHAIN_MAX_K && (st->tile_px == 256 || st->tile_px == 128);
#else
  (void)st;
  return false;
#endif
}

int launch_h_chain(const HStepArgs& args, int x_dtype, int tile_px, int nblk, hipStream_t stream) {
#if ESPM_KP <= 16
  static_assert(ESPM_CHAIN_PARTS == 1 || ESPM_CHAIN_PARTS == 2, "ESPM_CHAIN_PARTS: 1 or 2");
#if ESPM_CHAIN_PARTS > 1
  if ((args.k - ESPM_MIN_K) % ESPM_CHAIN_PARTS == 1) return launch_h_chain_part1(args, x_dtype, tile_px, nblk, stream);
#endif
  return launch_h_chain_part0(args, x_dtype, tile_px, nblk, stream);
#else
  (void)args; (void)x_dtype; (void)tile_px; (void)nblk; (void)stream;
  return set_error(ESPM_EUNSUPPORTED, "h_step (chained): not built for 17..32 components");
#endif
}
#endif

}  // namespace espm
