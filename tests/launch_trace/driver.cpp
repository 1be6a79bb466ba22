// Launch trace of mu_api.hip on the CPU: calls the entry points of the extern "C" surface that sequence launches, on states whose
// pointers are fake addresses, against the stubs of stubs.hip, and prints which launches each call issued with which arguments, what
// it returned and what it left in the state.  tests/test_launch_trace_cpu.py compares the output with tests/golden/launch_trace.txt.
//
// Output: per configuration (build / store / W update) one line with the count and the FNV-1a hash of its trace lines - written
// out, the table is 78000 lines - then the source-view checks in full, which show the format: per case "case <name>", the launches,
// and "-> rc ..." with the state left behind.  `driver --full` prints every configuration like that: run it on two versions of
// mu_api.hip and diff to see what a changed hash stands for.
#include <string.h>

#include <functional>

#include "espm_mu.h"
#include "mu_xchg.hpp"
#include "trace.hpp"

namespace lt {
void reset_events();
}
using lt::fmt;
using lt::line;

#if ESPM_MIN_K <= 8
static const char* BUILD = "narrow";
static const int K = 3;
#else
static const char* BUILD = "wide";
static const int K = 12;
#endif
static const int N = 64, P = 2048, NX = 32, NY = 64, HIST_LEN = 16, M_DICT = 12;

// one fake address per pointer of the state, and those of the calls' own arguments
#define PTRS(F)                                                                                                                          \
  F(x_cm) F(x_pm) F(g) F(colsum_g) F(w0) F(w1) F(gw_s) F(colsum_gw) F(h0) F(h1) F(h_t) F(mu) F(hpart) F(hstat0) F(hstat1) F(a_slab) F(a) \
  F(w_scratch) F(hist) F(ell_h) F(ell_h_off) F(ell_klc) F(ell_w) F(ell_w_off) F(chan_perm) F(pix_perm) F(g_t) F(pg_q) F(ell_fill_px)    \
  F(ell_fill_num) F(ell_hv_px) F(ell_hv_px_off) F(ell_hv_pm) F(ell_hv_klc) F(ell_hv_kl) F(ell_hv_grp) F(ell_hv_grp_off) F(ell_hv_wm)    \
  F(hpart_alt) F(stream) F(mailbox) F(staging) F(records) F(record) F(src) F(out_a) F(out_b) F(out_c)
struct Ptrs {
#define F(name) void* name;
  PTRS(F)
#undef F
} A;

struct Store {
  const char* name;
  int x_dtype, tile_px;
  bool fill, hv;
  int no_fused, ell_stream;
  size_t fused_lds;   // what the stubbed fused_ell_lds_bytes answers
};
struct WUpdate {
  const char* name;
  int m, simplex_w;
  bool pg;
};

static espm_mu_state make_state(const Store& s, const WUpdate& w) {
  espm_mu_state st;
  memset(&st, 0, sizeof(st));
  st.struct_size = sizeof(st);
  st.abi_version = ESPM_MU_ABI_VERSION;
  st.n = N, st.m = w.m, st.k = K, st.p = P, st.nx = NX, st.ny = NY, st.n_pad = N, st.p_pad = P, st.p_total = P;
  st.x_dtype = s.x_dtype, st.tile_px = st.x_tile = s.tile_px, st.n_cm = N;
  st.simplex_h = 1, st.simplex_w = w.simplex_w, st.grid_mode = 1, st.compute_loss = 1;
  st.lambda_l = 1.f, st.sigma_l = 8.f, st.eps_reg = 1.f, st.log_shift = 1e-14f, st.dicotomy_tol = 1e-5f, st.rel_tol = 1e-4f;
  st.xscale = 1.f, st.gw_floor = 1e-30f;
  st.w[0] = (float*)A.w0, st.w[1] = (float*)A.w1, st.h[0] = (float*)A.h0, st.h[1] = (float*)A.h1;
  st.gw_s = (float*)A.gw_s, st.colsum_gw = (double*)A.colsum_gw, st.h_t = (float*)A.h_t, st.mu = (const float*)A.mu;
  st.hpart = (double*)A.hpart, st.hstat[0] = (double*)A.hstat0, st.hstat[1] = (double*)A.hstat1;
  st.a_slab = (float*)A.a_slab, st.a = (float*)A.a, st.w_scratch = (float*)A.w_scratch;
  st.hist = (double*)A.hist, st.hist_len = HIST_LEN, st.cur = 0, st.it = 2;
  if (w.m > 0) st.g = (const float*)A.g, st.colsum_g = (const float*)A.colsum_g, st.g_t = (const float*)A.g_t;
  if (w.pg) st.pg_q = (double*)A.pg_q, st.pg_gamma_w = 0.5f;
  if (s.x_dtype == ESPM_X_ELL) {
    st.ell_h = (const uint32_t*)A.ell_h, st.ell_h_off = (const int32_t*)A.ell_h_off, st.ell_klc = (const float*)A.ell_klc;
    st.ell_w = (const uint32_t*)A.ell_w, st.ell_w_off = (const int32_t*)A.ell_w_off, st.chan_perm = (const int32_t*)A.chan_perm;
    st.pix_perm = (const int32_t*)A.pix_perm, st.ell_cbits = 6, st.n_cg = 1;
    st.ell_pb = 2 * s.tile_px, st.nblk_w = (P + st.ell_pb - 1) / st.ell_pb;
    if (s.fill) st.ell_fill_px = (const int32_t*)A.ell_fill_px, st.ell_fill_n = 5;
    if (s.fill || s.hv) st.ell_fill_num = (float*)A.ell_fill_num;
    if (s.hv) {
      st.ell_hv_n = 9, st.ell_hv_npx = 4, st.ell_hv_ngrp = 7;
      st.ell_hv_px = (const int32_t*)A.ell_hv_px, st.ell_hv_px_off = (const int32_t*)A.ell_hv_px_off, st.ell_hv_pm = (const int32_t*)A.ell_hv_pm;
      st.ell_hv_klc = (const float*)A.ell_hv_klc, st.ell_hv_kl = (double*)A.ell_hv_kl, st.ell_hv_grp = (const int32_t*)A.ell_hv_grp;
      st.ell_hv_grp_off = (const int32_t*)A.ell_hv_grp_off, st.ell_hv_wm = (const int32_t*)A.ell_hv_wm;
    }
  } else {
    st.x_cm = A.x_cm, st.x_pm = A.x_pm, st.nblk_w = 8;
  }
  st.no_fused = s.no_fused, st.ell_stream = s.ell_stream;
  return st;
}

static uint32_t fnv(uint32_t h, const std::string& s) {
  for (unsigned char c : s) h = (h ^ c) * 16777619u;
  return (h ^ '\n') * 16777619u;
}

static espm_stream_t S;

// one case: the call on a copy of the state, then what it returned and left behind
static void run(const std::string& name, espm_mu_state st, const std::function<int(espm_mu_state&)>& fn) {
  lt::reset_events();
  line("case " + name);
  const int rc = fn(st);
  line(fmt("-> rc=%d cur=%d it=%d tail_mode=%d halo_top=%s halo_bot=%s%s%s", rc, st.cur, st.it, st.tail_mode, lt::pname(st.halo_top).c_str(),
           lt::pname(st.halo_bot).c_str(), rc ? " error: " : "", rc ? espm_mu_last_error() : ""));
}

static void run_config(const Store& s, const WUpdate& w, bool show) {
  lt::g_lines.clear();
  lt::reset_defs();
  const espm_mu_state base = make_state(s, w);
  lt::g_answers = lt::Answers{s.fused_lds, false, false, (base.n_pad + 31) / 32};
  auto with = [&](std::function<void(espm_mu_state&)> edit) {
    espm_mu_state st = base;
    edit(st);
    return st;
  };
  auto tm = [&](int mode) { return with([&](espm_mu_state& st) { st.tail_mode = mode; }); };
  espm_xchg x;
  memset(&x, 0, sizeof(x));
  x.world = 3, x.rank = 1, x.record_bytes = espm_mu_shard_record_bytes(&base), x.wgflags = 1 << 20;
  x.mailbox = (unsigned char*)A.mailbox, x.staging = (unsigned char*)A.staging;

  for (int mode : {0, ESPM_TAIL_RIDE}) {
    const std::string t = fmt(" tail_mode=%d", mode);
    run("step_h" + t, tm(mode), [](espm_mu_state& st) { return espm_mu_step_h(&st, st.cur, 1, S); });
    run("step_hw" + t, tm(mode), [](espm_mu_state& st) { return espm_mu_step_hw(&st, st.cur, S); });
    run("loss_only" + t, tm(mode), [](espm_mu_state& st) { return espm_mu_loss_only(&st, st.cur, st.it, S); });
  }
  run("step_h src=1 write_h=0", base, [](espm_mu_state& st) { return espm_mu_step_h(&st, 1, 0, S); });
  run("w_accum", base, [](espm_mu_state& st) { return espm_mu_w_accum(&st, S); });
  for (int wf : {0, 1})
    for (int mode : {0, ESPM_TAIL_DEFER})
      run(fmt("w_reduce_finish with_finalize=%d tail_mode=%d", wf, mode), tm(mode),
          [wf](espm_mu_state& st) { return espm_mu_w_reduce_finish(&st, st.cur, st.it, wf, S); });
  for (int mode : {0, ESPM_TAIL_DEFER})
    run(fmt("shard_combine_finish tail_mode=%d", mode), tm(mode),
        [](espm_mu_state& st) { return espm_mu_shard_combine_finish(&st, A.records, 3, st.cur, st.it, S); });
  // (its four branches follow from the W update, no_fused and what the stubbed w_gsplit_applies answers)
  for (int gsplit : {0, 1})
    for (int mode : {0, ESPM_TAIL_DEFER})
      run(fmt("shard_exchange_finish gsplit=%d tail_mode=%d", gsplit, mode), tm(mode), [&, gsplit](espm_mu_state& st) {
        lt::g_answers.w_gsplit = gsplit != 0;
        const int rc = espm_mu_shard_exchange_finish(&st, &x, 7, st.cur, st.it, S);
        lt::g_answers.w_gsplit = false;
        return rc;
      });
  run("shard_exchange_finish lambda_l=0", with([](espm_mu_state& st) { st.lambda_l = 0.f; }),
      [&](espm_mu_state& st) { return espm_mu_shard_exchange_finish(&st, &x, 8, st.cur, st.it, S); });
  for (int n_iter : {0, 3})
    for (int fl : {0, 1})
      run(fmt("iterate n_iter=%d final_loss=%d", n_iter, fl), base, [=](espm_mu_state& st) { return espm_mu_iterate(&st, n_iter, fl, S); });
  run("iterate from it=0 cur=1", with([](espm_mu_state& st) { st.it = 0, st.cur = 1; }),
      [](espm_mu_state& st) { return espm_mu_iterate(&st, 2, 1, S); });
  run("iterate_timed n_iter=2", base, [](espm_mu_state& st) {
    float first[2], rest[2];
    return espm_mu_iterate_timed(&st, 2, first, rest, S);
  });
  for (int chain : {0, 1})
    for (int fl : {0, 1})
      run(fmt("iterate_h chain=%d final_loss=%d", chain, fl), with([&](espm_mu_state& st) { st.hpart_alt = chain ? (double*)A.hpart_alt : nullptr; }),
          [&, chain, fl](espm_mu_state& st) {
            lt::g_answers.h_chain_built = chain != 0;
            const int rc = espm_mu_iterate_h(&st, 3, fl, S);
            lt::g_answers.h_chain_built = false;
            return rc;
          });
  run("iterate_h n_iter=0", base, [](espm_mu_state& st) { return espm_mu_iterate_h(&st, 0, 1, S); });
  for (float lam : {1.f, 0.f})
    for (int fl : {0, 1})
      run(fmt("iterate_sharded halo=%d final_loss=%d", lam != 0.f, fl), with([=](espm_mu_state& st) { st.lambda_l = lam; }), [&, fl](espm_mu_state& st) {
        uint32_t seq = 4;
        const int rc = espm_mu_iterate_sharded(&st, &x, &seq, 3, fl, S);
        line(fmt("seq=%u", seq));
        return rc;
      });
  run("iterate_sharded n_iter=0", base, [&](espm_mu_state& st) {
    uint32_t seq = 4;
    return espm_mu_iterate_sharded(&st, &x, &seq, 0, 1, S);
  });
  run("w_update_tail", base, [](espm_mu_state& st) { return espm_mu_w_update_tail(&st, st.cur, st.it, S); });
  // the other calls that take a history slot or build the same argument blocks
  run("build_gw", base, [](espm_mu_state& st) { return espm_mu_build_gw(&st, 1, S); });
  run("h_finalize", base, [](espm_mu_state& st) { return espm_mu_h_finalize(&st, st.cur, st.it, S); });
  run("w_reduce", base, [](espm_mu_state& st) { return espm_mu_w_reduce(&st, S); });
  run("w_reduce_finalize", base, [](espm_mu_state& st) { return espm_mu_w_reduce_finalize(&st, st.cur, st.it, S); });
  run("w_finish", base, [](espm_mu_state& st) { return espm_mu_w_finish(&st, st.cur, 1 - st.cur, st.it + 1, S); });
  run("w_finish slot=-1", base, [](espm_mu_state& st) { return espm_mu_w_finish(&st, st.cur, st.cur, -1, S); });
  run("w_reduce_pack", base, [](espm_mu_state& st) { return espm_mu_w_reduce_pack(&st, st.cur, st.it, A.record, S); });
  run("shard_pack", base, [](espm_mu_state& st) { return espm_mu_shard_pack(&st, 1, A.record, S); });
  run("shard_combine", base, [](espm_mu_state& st) { return espm_mu_shard_combine(&st, A.records, 3, 1, S); });

  // ---- refusals ---------------------------------------------------------------------------------------------------------------------
  const int last = HIST_LEN - 1;   // (a slot that exists, but slot + 1 does not)
  run("refused slot: h_finalize", base, [](espm_mu_state& st) { return espm_mu_h_finalize(&st, 0, HIST_LEN, S); });
  run("refused slot: loss_only", base, [](espm_mu_state& st) { return espm_mu_loss_only(&st, 0, -1, S); });
  run("refused slot: w_reduce_finalize", base, [](espm_mu_state& st) { return espm_mu_w_reduce_finalize(&st, 0, HIST_LEN, S); });
  run("refused slot: w_finish", base, [](espm_mu_state& st) { return espm_mu_w_finish(&st, 0, 1, HIST_LEN, S); });
  run("refused slot: w_reduce_pack", base, [](espm_mu_state& st) { return espm_mu_w_reduce_pack(&st, 0, HIST_LEN, A.record, S); });
  run("refused slot: w_reduce_finish", base, [=](espm_mu_state& st) { return espm_mu_w_reduce_finish(&st, 0, last, 1, S); });
  run("refused slot: shard_combine_finish", base, [=](espm_mu_state& st) { return espm_mu_shard_combine_finish(&st, A.records, 3, 0, last, S); });
  run("refused slot: shard_exchange_finish", base, [&](espm_mu_state& st) { return espm_mu_shard_exchange_finish(&st, &x, 7, 0, -1, S); });
  run("refused slot: w_update_tail", base, [=](espm_mu_state& st) { return espm_mu_w_update_tail(&st, 0, last, S); });
  run("refused history: iterate", base, [](espm_mu_state& st) { return espm_mu_iterate(&st, HIST_LEN - 2, 0, S); });
  run("refused history: iterate_h", base, [](espm_mu_state& st) { return espm_mu_iterate_h(&st, HIST_LEN - 2, 0, S); });
  run("refused history: iterate_sharded", base, [&](espm_mu_state& st) {
    uint32_t seq = 4;
    return espm_mu_iterate_sharded(&st, &x, &seq, HIST_LEN - 2, 0, S);
  });
  run("refused n_iter: iterate", base, [](espm_mu_state& st) { return espm_mu_iterate(&st, -1, 0, S); });
  run("refused n_iter: iterate_timed", base, [](espm_mu_state& st) {
    float ms[1];
    return espm_mu_iterate_timed(&st, 0, ms, ms, S);
  });
  run("refused src: step_h", base, [](espm_mu_state& st) { return espm_mu_step_h(&st, 2, 1, S); });
  run("refused src: step_hw", base, [](espm_mu_state& st) { return espm_mu_step_hw(&st, -1, S); });
  run("refused src: h_finalize", base, [](espm_mu_state& st) { return espm_mu_h_finalize(&st, 2, 0, S); });
  run("refused src: w_reduce_finalize", base, [](espm_mu_state& st) { return espm_mu_w_reduce_finalize(&st, 2, 0, S); });
  run("refused src: w_finish", base, [](espm_mu_state& st) { return espm_mu_w_finish(&st, 0, 2, 0, S); });
  run("refused src: w_reduce_finish", base, [](espm_mu_state& st) { return espm_mu_w_reduce_finish(&st, 2, 0, 1, S); });
  run("refused src: shard_combine_finish", base, [](espm_mu_state& st) { return espm_mu_shard_combine_finish(&st, A.records, 3, 2, 0, S); });
  run("refused src: shard_exchange_finish", base, [&](espm_mu_state& st) { return espm_mu_shard_exchange_finish(&st, &x, 7, 2, 0, S); });
  run("refused src: w_update_tail", base, [](espm_mu_state& st) { return espm_mu_w_update_tail(&st, 2, 0, S); });
  run("refused src: w_reduce_pack", base, [](espm_mu_state& st) { return espm_mu_w_reduce_pack(&st, 2, 0, A.record, S); });
  run("refused tail: step_h rides at it=0", with([](espm_mu_state& st) { st.it = 0, st.tail_mode = ESPM_TAIL_RIDE; }),
      [](espm_mu_state& st) { return espm_mu_step_h(&st, st.cur, 1, S); });
  run("refused tail: step_hw rides at it=0", with([](espm_mu_state& st) { st.it = 0, st.tail_mode = ESPM_TAIL_RIDE; }),
      [](espm_mu_state& st) { return espm_mu_step_hw(&st, st.cur, S); });
  {
    espm_xchg y = x;
    y.record_bytes += 16;
    run("refused record bytes: shard_exchange_finish", base, [&](espm_mu_state& st) { return espm_mu_shard_exchange_finish(&st, &y, 7, 0, 2, S); });
    run("refused record bytes: iterate_sharded", base, [&](espm_mu_state& st) {
      uint32_t seq = 4;
      return espm_mu_iterate_sharded(&st, &y, &seq, 1, 0, S);
    });
  }
  // n * log_shift >= 1 (k * log_shift < 1: the state itself passes)
  const espm_mu_state shifted = with([](espm_mu_state& st) { st.log_shift = 0.02f; });
  run("log_shift=0.02: w_finish", shifted, [](espm_mu_state& st) { return espm_mu_w_finish(&st, st.cur, 1 - st.cur, st.it + 1, S); });
  run("log_shift=0.02: w_reduce_finish", shifted, [](espm_mu_state& st) { return espm_mu_w_reduce_finish(&st, st.cur, st.it, 1, S); });
  run("log_shift=0.02: shard_combine_finish", shifted, [](espm_mu_state& st) { return espm_mu_shard_combine_finish(&st, A.records, 3, st.cur, st.it, S); });
  run("log_shift=0.02: shard_exchange_finish", shifted, [&](espm_mu_state& st) { return espm_mu_shard_exchange_finish(&st, &x, 7, st.cur, st.it, S); });
  run("log_shift=0.02: iterate", shifted, [](espm_mu_state& st) { return espm_mu_iterate(&st, 2, 1, S); });
  run("log_shift=0.02: iterate_sharded", shifted, [&](espm_mu_state& st) {
    uint32_t seq = 4;
    return espm_mu_iterate_sharded(&st, &x, &seq, 2, 1, S);
  });
  run("log_shift=0.02 simplex_rows: w_finish", with([](espm_mu_state& st) { st.log_shift = 0.02f, st.simplex_rows = (const int32_t*)A.out_c; }),
      [](espm_mu_state& st) { return espm_mu_w_finish(&st, st.cur, 1 - st.cur, st.it + 1, S); });

  uint32_t h = 2166136261u;
  for (const std::string& l : lt::g_lines) h = fnv(h, l);
  printf("config %s/%s/%s lines=%zu fnv1a=%08x\n", BUILD, s.name, w.name, lt::g_lines.size(), h);
  if (show)
    for (const std::string& l : lt::g_lines) printf("  %s\n", l.c_str());
}

// the argument checks of the calls that read the caller's image (no W update, no store variants: once per build)
static void run_source_checks() {
  lt::g_lines.clear();
  lt::reset_defs();
  const Store ell = {"ell", ESPM_X_ELL, 512, false, false, 0, 0, 0};
  const WUpdate local = {"local", 0, 0, false};
  const espm_mu_state st0 = make_state(ell, local);
  struct View {
    const char* name;
    int dtype, layout;
    int64_t ld;
  };
  const View views[] = {{"f32 cm", ESPM_SRC_F32, ESPM_LAYOUT_CM, P},       {"f64 pm", ESPM_SRC_F64, ESPM_LAYOUT_PM, N + 3},
                        {"bad dtype", 2, ESPM_LAYOUT_CM, P},               {"bad layout", ESPM_SRC_F32, 2, P},
                        {"cm ld too small", ESPM_SRC_F32, ESPM_LAYOUT_CM, P - 1}, {"pm ld too small", ESPM_SRC_F64, ESPM_LAYOUT_PM, N - 1}};
  for (const View& v : views) {
    run(fmt("pack_x %s", v.name), st0, [&](espm_mu_state& st) {
      return espm_mu_pack_x(A.src, v.dtype, v.layout, v.ld, N, P, A.x_cm, A.x_pm, ESPM_X_U8, st.n_pad, st.p_pad, 512, st.n_cm, S);
    });
    run(fmt("ell_heavy_count %s", v.name), st0, [&](espm_mu_state& st) {
      return espm_mu_ell_heavy_count(&st, A.src, v.dtype, v.layout, v.ld, (uint8_t*)A.out_a, (uint8_t*)A.out_b, (int32_t*)A.out_c, S);
    });
    run(fmt("ell_heavy_fill %s", v.name), st0, [&](espm_mu_state& st) {
      return espm_mu_ell_heavy_fill(&st, A.src, v.dtype, v.layout, v.ld, (const int32_t*)A.out_a, (int32_t*)A.out_b, S);
    });
  }
  printf("config %s/source views\n", BUILD);
  for (const std::string& l : lt::g_lines) printf("  %s\n", l.c_str());
}

int main(int argc, char** argv) {
  const bool full = argc > 1 && !strcmp(argv[1], "--full");
#define F(name) A.name = lt::fake(#name);
  PTRS(F)
#undef F
  lt::g_ev_base = static_cast<char*>(lt::fake("ev"));
  S = A.stream;
  const size_t fits = 1024, too_big = ESPM_ELL_LDS_MAX + 1;
  // sparse store: with and without fill pixels and heavy elements, no_fused 0..3, streamed lists; 64-pixel tiles (blocks of 128 pixels,
  // 16 of them) are below the fused launch's thresholds, so only no_fused = 3 fuses there; a table that does not fit LDS never fuses
  const Store stores[] = {{"f32", ESPM_X_F32, 128, false, false, 0, 0, fits},
                          {"u8", ESPM_X_U8, 128, false, false, 0, 0, fits},
                          {"ell", ESPM_X_ELL, 512, false, false, 0, 0, fits},
                          {"ell+fill", ESPM_X_ELL, 512, true, false, 0, 0, fits},
                          {"ell+heavy", ESPM_X_ELL, 512, false, true, 0, 0, fits},
                          {"ell+fill+heavy", ESPM_X_ELL, 512, true, true, 0, 0, fits},
                          {"ell no_fused=1", ESPM_X_ELL, 512, false, false, 1, 0, fits},
                          {"ell+fill+heavy no_fused=1", ESPM_X_ELL, 512, true, true, 1, 0, fits},
                          {"ell no_fused=2", ESPM_X_ELL, 512, false, false, 2, 0, fits},
                          {"ell no_fused=2 stream", ESPM_X_ELL, 512, false, false, 2, 1, fits},
                          {"ell stream", ESPM_X_ELL, 512, false, false, 0, 1, fits},
                          {"ell+fill+heavy stream", ESPM_X_ELL, 512, true, true, 0, 1, fits},
                          {"ell tile=64", ESPM_X_ELL, 64, false, false, 0, 0, fits},
                          {"ell tile=64 no_fused=3", ESPM_X_ELL, 64, false, false, 3, 0, fits},
                          {"ell+heavy tile=64 no_fused=3 stream", ESPM_X_ELL, 64, false, true, 3, 1, fits},
                          {"ell table too big", ESPM_X_ELL, 512, false, false, 0, 0, too_big}};
  const WUpdate updates[] = {{"local", 0, 0, false},
                             {"simplex split", 0, 1, false},
                             {"dictionary", M_DICT, 0, false},
                             {"dictionary+simplex", M_DICT, 1, false},
                             {"projected gradient", 0, 0, true}};
  for (const Store& s : stores)
    for (const WUpdate& w : updates) run_config(s, w, full);
  run_source_checks();
  return 0;
}
