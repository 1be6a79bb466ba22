// Which form finishes W, and for the register-resident finish which instance: the host arithmetic of the W update's dispatch in
// one place (the W step as a whole: mu_w_parts.hpp).  Host code only, no kernel: launch_w_finish (mu_w_finish.hip) and
// launch_w_dict_finish (mu_w_dict.hip) switch on the plan and espm_mu_w_update_form (mu_api.hip) returns it - all three from this
// header, so the query needs nothing of the kernels' units and its answer cannot drift from the launch.
#pragma once
#include <stdlib.h>

#include "mu_common.hpp"

namespace espm {

// ---- the sizes the kernels are built for --------------------------------------------------------------------------------------
// the one-workgroup W finish (mu_w_finish.hip)
constexpr int WF_THREADS = 1024;
#ifndef ESPM_WF_FEW_THREADS
#define ESPM_WF_FEW_THREADS 512
#endif
constexpr int WF_FEW_THREADS = ESPM_WF_FEW_THREADS;   // threads of the register-resident W finish for G = identity, k <= WF_HALF_MAX_K (A/B: 256)
#ifndef ESPM_WF_HALF_MAX_K
#define ESPM_WF_HALF_MAX_K 8
#endif
constexpr int WF_HALF_MAX_K = ESPM_WF_HALF_MAX_K;   // component counts up to which the register-resident W finish also exists with 512 threads
constexpr int WF_GTA_MAX = 8192;   // M * k up to which the register-resident finish takes a dictionary G
constexpr int WF_GTA_PAR = 512;    // M * k up to which G^T A uses the all-threads path (16 x M k floats of LDS)
// the dictionary-G W step by columns (mu_w_dict.hip: w_gcol_kernel): threads, channels per thread, columns of G
constexpr int GC_THREADS = 1024, GC_CPT = 2, GC_MMAX = 32;

// An on / off knob of the environment (README.md: ESPM_W_GCOL, ESPM_W_GSPLIT, ESPM_W_FINISH_GENERAL): `dflt` unless the variable is
// set and begins with the other value's digit.  Its user keeps the answer in a function-local static: read once per process.
static inline bool w_env_knob(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? (dflt ? e[0] != '0' : e[0] == '1') : dflt;
}

// ---- a dictionary G as many-workgroup launches ----------------------------------------------------------------------------------
// (w_gsplit_applies - the two-launch form applies - is mu_w_dict.hip's, declared in mu_common.hpp: the sharded half-step asks it too)
// the column form applies where the two-launch form does, the dictionary has at most GC_MMAX columns and a thread holds its channels
inline bool w_gcol_applies(const WFinishArgs& args) {
  if (!(w_gsplit_applies(args) && args.m <= GC_MMAX && args.n_pad <= GC_CPT * GC_THREADS && args.k <= KP && (size_t)2 * args.m * args.k * sizeof(float) >= (size_t)args.k * 8))
    return false;
  static const bool enabled = w_env_knob("ESPM_W_GCOL", true);
  return enabled;
}
// the column form, else the two launches, else 0 (the one-workgroup finish)
inline int plan_w_dict(const WFinishArgs& args) {
  if (w_gcol_applies(args)) return ESPM_W_FORM_DICT_COLUMNS;
  return w_gsplit_applies(args) ? ESPM_W_FORM_DICT_TWO_LAUNCH : 0;
}

// ---- what launch_w_finish runs for these arguments (WFinishPlan: mu_common.hpp) ---------------------------------------------------
inline WFinishPlan plan_w_finish(const WFinishArgs& args) {
  WFinishPlan pl;
  if ((pl.form = plan_w_dict(args)) != 0) return pl;   // a dictionary G one of the many-workgroup forms applies to
  const int M = args.m > 0 ? args.m : args.n;
  const long mk = (long)M * args.k;
  const int span = M > args.n_cm ? M : args.n_cm;
  // G = identity, up to 8 components (the narrow build), up to 2048 rows: 8 waves with 256 registers each (with the simplex
  // over W at the headline size 49 -> 37 us at k = 5, iteration 278 -> 248 us at k = 8); a dictionary G keeps the 16 waves
  // (its loops over the rows of G want them: C5 141 vs 151 us)
  const int nt = (!args.g && args.k <= WF_HALF_MAX_K && span <= 4 * 512) ? WF_FEW_THREADS : WF_THREADS;
  const int crows = (span + nt - 1) / nt;               // channels (or, with G = identity, rows of W) per thread
  const int rows = args.g ? (M + nt - 1) / nt : crows;   // rows of W per thread
  // G given: [M][k rounded up to 4] new W, [M k] G^T A, and the per-wave partials of the all-threads G^T A (within the 64 KB a
  // kernel gets without asking)
  const size_t lds = args.g ? ((size_t)M * ((args.k + 3) / 4 * 4) + (size_t)mk * (1 + (args.g_t && mk <= WF_GTA_PAR ? WF_THREADS / 64 : 0))) * sizeof(float) : 0;
  // (the widest build - 17..32 components - has the general one-workgroup finish only: the register-resident ones are not built there;
  //  ESPM_W_FINISH_GENERAL=1 sends the other builds there too - tests: images small enough for the register-resident kernels never reach it)
  static const bool general_only = w_env_knob("ESPM_W_FINISH_GENERAL", false);
  // (nt == 256: only in the A/B build with -DESPM_WF_FEW_THREADS=256, which holds up to 8 rows per thread; the product has 512 and 1024)
  if (!(KP <= 16 && !general_only && crows <= (nt == 256 ? 8 : 4) && rows <= (nt == 256 ? 8 : 4) && (!args.g || (mk <= WF_GTA_MAX && lds <= 64 * 1024)))) {
    pl.form = ESPM_W_FORM_ONE_WG_GENERAL;
    return pl;
  }
  pl.form = ESPM_W_FORM_ONE_WG_REGISTERS;
  pl.nt = nt;
  pl.lds = lds;
  // the instances are built for 1, 2 and 4 (nt == 256: and 8) per thread: the next one up
  auto built = [nt](int v) { return v <= 1 ? 1 : v <= 2 ? 2 : (v <= 4 || nt != 256) ? 4 : 8; };
  if (crows > rows && rows <= 1) {   // dictionary G with at most nt rows: one row of W per thread, 2 or 4 channels in its G^T A
    pl.rows = 1;
    pl.crows = crows <= 2 ? 2 : 4;
  } else {
    pl.rows = pl.crows = built(crows > rows ? crows : rows);
  }
  // (w_finish_fast_kernel's own test: the packed sum of the all-threads G^T A is laid out for 4 rows x 8 components)
  pl.gta_all = (args.k <= 8 && args.g && args.g_t && mk <= WF_GTA_PAR) ? 1 : 0;
  return pl;
}

}  // namespace espm
