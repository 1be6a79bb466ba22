// Every function mu_api.hip calls outside itself - the launchers and predicates of the kernel units, the exchange's three calls and the
// HIP runtime - as a stub.  Each one that stands for a launch or a runtime call appends one line to the trace: its name and its
// arguments, pointers by the name of the state field they equal (trace.hpp).  Nothing here launches, allocates on or opens a device; the program links without the HIP runtime library.
#include "mu_common.hpp"
#include "mu_xchg.hpp"
#include "trace.hpp"

using lt::Args;
using lt::call;

namespace {

std::string fin_id(const espm::HFinalizeArgs& a) {
  Args t;
  t.p(a.hpart).p(a.colsum_gw).p(a.hstat_in).p(a.hstat_out).p(a.hist_slot).i(a.nblk).i(a.k).i(a.compute_loss).i(a.have_prev).f(a.xscale).p(a.pg_q);
  return lt::intern('F', t.s);
}
std::string fin_id(const espm::HFinalizeArgs* a) { return a ? fin_id(*a) : "null"; }

std::string tail_id(const espm::WTailArgs& a) {
  Args t;
  t.p(a.parts).p(a.w_old).p(a.w_new).p(a.colsum_gw).p(a.hist_slot).p(a.pg_q).i(a.n).i(a.k).i(a.nbk).f(a.rel_tol);
  return lt::intern('T', t.s);
}

std::string h_id(const espm::HStepArgs& a) {
  Args t;
  t.p(a.x_cm).p(a.x_pm).i(a.mfma).p(a.gw_s).p(a.colsum_gw).p(a.h_in).p(a.h_out).p(a.h_t).p(a.mu).p(a.fixed_h).p(a.halo_top).p(a.halo_bot);
  t.p(a.hstat_in).p(a.hpart).i(a.n).i(a.k).i(a.p).i(a.nx).i(a.ny).i(a.p_pad).i(a.x_tile).i(a.n_cm).p(a.gw_a).p(a.gw_p);
  t.i(a.simplex_h).i(a.grid_mode).i(a.compute_loss).i(a.write_h).i(a.have_prev);
  t.f(a.lambda_l).f(a.sigma_l).f(a.eps_reg).f(a.log_shift).f(a.tol).f(a.xscale).f(a.rel_tol).f(a.inv_count);
  t.p(a.ell).p(a.ell_off).p(a.ell_klc).p(a.ell_pix).i(a.ell_bits).i(a.n_pad).i(a.ell_tp).p(a.l2_m).p(a.breg_sr).i(a.h_rule).p(a.fill_num).i(a.fill_n);
  t.p(a.cs_parts).i(a.cs_nbk).i(a.cs_lds_off).i(a.tail_on).t(a.tail_on ? tail_id(a.tail) : "-").i(a.rec_nb);   // (tail: set only where tail_on)
  t.p(a.chain_prev).i(a.chain_nb).i(a.chain_lds_off).i(a.chain_fin_on).t(fin_id(a.chain_fin));
  return lt::intern('H', t.s);
}

std::string w_id(const espm::WAccumArgs& a) {
  Args t;
  t.p(a.x_pm).p(a.x_cm).i(a.x_tile).i(a.n_cm).i(a.p_pad).i(a.mfma).p(a.gw_s).p(a.h_t).p(a.a_slab).i(a.n_pad).i(a.p).i(a.ppb);
  t.p(a.ell).p(a.ell_off).p(a.chan_perm).i(a.n_cg).i(a.pb).i(a.pbits).i(a.l2);
  return lt::intern('A', t.s);
}

std::string f_id(const espm::WFinishArgs& a) {
  Args t;
  t.p(a.g).p(a.g_t).p(a.colsum_g).p(a.w_old).p(a.w_new).p(a.a).p(a.hstat).p(a.fixed_w).p(a.simplex_rows).p(a.scratch).p(a.breg_sr);
  t.f(a.pg_gamma_w).p(a.pg_q).p(a.gw_s).p(a.colsum_gw).p(a.gw_a).p(a.gw_p).p(a.hist_slot);
  t.i(a.n).i(a.m).i(a.k).i(a.n_pad).i(a.n_cm).i(a.simplex_w).i(a.update_w).f(a.log_shift).f(a.tol).f(a.rel_tol).f(a.xscale).f(a.gw_floor);
  return lt::intern('W', t.s);
}

std::string x_id(const espm_xchg* x) {
  if (!x) return "null";
  Args t;
  t.i(x->world).i(x->rank).u(x->record_bytes).p(x->mailbox).p(x->staging);
  return lt::intern('X', t.s);
}

// the launchers that form the tail hand it to the caller instead of launching it when the caller asks (mu_w_reduce.hip)
std::string hand_tail(const espm::WFinishArgs& f, espm::WTailArgs* defer_tail) {
  if (!defer_tail) return "tail launched";
  *defer_tail = espm::make_w_tail_args(f);
  return "tail deferred";
}

int g_events = 0;

}  // namespace

namespace lt {
void reset_events() { g_events = 0; }
}

namespace espm {

bool h_chain_built(const espm_mu_state*) { return lt::g_answers.h_chain_built; }
// (the predicates and make_w_tail_args launch nothing and leave no line: how often mu_api.hip asks them is not part of its behaviour)
size_t fused_ell_lds_bytes(int, int, int) { return lt::g_answers.fused_lds_bytes; }
bool w_gsplit_applies(const WFinishArgs&) { return lt::g_answers.w_gsplit; }
WTailArgs make_w_tail_args(const WFinishArgs& f) {
  WTailArgs t;
  t.parts = reinterpret_cast<const double*>(f.scratch);
  t.w_old = f.w_old;
  t.w_new = f.w_new;
  t.colsum_gw = f.colsum_gw;
  t.hist_slot = f.hist_slot;
  t.pg_q = f.pg_q;
  t.n = f.n;
  t.k = f.k;
  t.nbk = lt::g_answers.tail_nbk;
  t.rel_tol = f.rel_tol;
  return t;
}

int dispatch_h_step(const HStepArgs& a, int x_dtype, int tile_px, int nblk, hipStream_t s) {
  call("dispatch_h_step", Args().t(h_id(a)).i(x_dtype).i(tile_px).i(nblk).p(s));
  return 0;
}
int launch_h_chain(const HStepArgs& a, int x_dtype, int tile_px, int nblk, hipStream_t s) {
  call("launch_h_chain", Args().t(h_id(a)).i(x_dtype).i(tile_px).i(nblk).p(s));
  return 0;
}
int launch_h_finalize(const HFinalizeArgs& a, hipStream_t s) {
  call("launch_h_finalize", Args().t(fin_id(a)).p(s));
  return 0;
}
int launch_h_ell(const HStepArgs& a, int nblk, hipStream_t s) {
  call("launch_h_ell", Args().t(h_id(a)).i(nblk).p(s));
  return 0;
}
int launch_fused_ell(const HStepArgs& h, const WAccumArgs& w, int nblk, hipStream_t s, int static_units, int stream_lists) {
  call("launch_fused_ell", Args().t(h_id(h)).t(w_id(w)).i(nblk).p(s).i(static_units).i(stream_lists));
  return 0;
}
int launch_ell_count(const uint8_t* x_pm, int n, int n_pad, int p, int p_pad, int cbits, int n_cg, int nblk, int pb, int32_t* cnt_px,
                     int32_t* cnt_bc, float* klc, hipStream_t s, uint8_t* bkt_px, uint8_t* bkt_bc) {
  call("launch_ell_count", Args().p(x_pm).i(n).i(n_pad).i(p).i(p_pad).i(cbits).i(n_cg).i(nblk).i(pb).p(cnt_px).p(cnt_bc).p(klc).p(s).p(bkt_px).p(bkt_bc));
  return 0;
}
int launch_ell_plan(const int32_t* cnt_px, const int32_t* cnt_bc, int n, int n_cg, int nblk, int p_pad, int win, int32_t* chan_perm,
                    int32_t* pix_perm, int32_t* h_off, int32_t* w_off, long long* rows, hipStream_t s) {
  call("launch_ell_plan", Args().p(cnt_px).p(cnt_bc).i(n).i(n_cg).i(nblk).i(p_pad).i(win).p(chan_perm).p(pix_perm).p(h_off).p(w_off).p(rows).p(s));
  return 0;
}
int launch_ell_fill(const uint8_t* x_pm, int n, int n_pad, int p, int p_pad, int cbits, int n_cg, int nblk, int win, int pb,
                    const int32_t* chan_perm, const int32_t* pix_perm, const int32_t* h_off, const int32_t* w_off, uint32_t* ell_h,
                    uint32_t* ell_w, hipStream_t s, const uint8_t* x_cm, int n_cm, const uint8_t* bkt_px, const uint8_t* bkt_bc) {
  call("launch_ell_fill", Args().p(x_pm).i(n).i(n_pad).i(p).i(p_pad).i(cbits).i(n_cg).i(nblk).i(win).i(pb).p(chan_perm).p(pix_perm).p(h_off).p(w_off)
                              .p(ell_h).p(ell_w).p(s).p(x_cm).i(n_cm).p(bkt_px).p(bkt_bc));
  return 0;
}
int launch_w_ell(const WAccumArgs& a, int k, int nblk, hipStream_t s) {
  call("launch_w_ell", Args().t(w_id(a)).i(k).i(nblk).p(s));
  return 0;
}
int launch_ell_fill_num(const float* gw_s, const float* h_in, const int32_t* fill_px, int fill_n, int n, int k, int p_pad, float fill,
                        float* fill_num, hipStream_t s, int ld) {
  call("launch_ell_fill_num", Args().p(gw_s).p(h_in).p(fill_px).i(fill_n).i(n).i(k).i(p_pad).f(fill).p(fill_num).p(s).i(ld));
  return 0;
}
int launch_ell_hv_count(const void* x, int src_dtype, int layout, int64_t ld, int n, int p, int n_pad, int n_cm, uint8_t* x8, uint8_t* x8c,
                        int32_t* cnt_px, hipStream_t s) {
  call("launch_ell_hv_count", Args().p(x).i(src_dtype).i(layout).i(ld).i(n).i(p).i(n_pad).i(n_cm).p(x8).p(x8c).p(cnt_px).p(s));
  return 0;
}
int launch_ell_hv_fill(const void* x, int src_dtype, int layout, int64_t ld, int n, int p, const int32_t* px_off, int32_t* hv_pm, hipStream_t s) {
  call("launch_ell_hv_fill", Args().p(x).i(src_dtype).i(layout).i(ld).i(n).i(p).p(px_off).p(hv_pm).p(s));
  return 0;
}
int launch_ell_hv_h(const espm_mu_state*, int src, int ld, hipStream_t s) {
  call("launch_ell_hv_h", Args().i(src).i(ld).p(s));
  return 0;
}
int launch_ell_hv_post(const espm_mu_state*, const float* h, size_t hs_k, size_t hs_p, bool w, bool loss, hipStream_t s) {
  call("launch_ell_hv_post", Args().p(h).u(hs_k).u(hs_p).i(w).i(loss).p(s));
  return 0;
}
int dispatch_w_accum(const WAccumArgs& a, int k, int x_dtype, int nblk, hipStream_t s) {
  call("dispatch_w_accum", Args().t(w_id(a)).i(k).i(x_dtype).i(nblk).p(s));
  return 0;
}
int launch_w_reduce(const float* slab, float* out, int nblk, int total, const HFinalizeArgs* fin, hipStream_t s, const float* bw_old,
                    double* bparts, int n, int k, int n_pad) {
  call("launch_w_reduce", Args().p(slab).p(out).i(nblk).i(total).t(fin_id(fin)).p(s).p(bw_old).p(bparts).i(n).i(k).i(n_pad));
  return 0;
}
int launch_w_simplex_update(const WFinishArgs& f, float* a_inout, const double* bparts, double tol, hipStream_t s, WTailArgs* defer_tail) {
  call("launch_w_simplex_update", Args().t(f_id(f)).p(a_inout).p(bparts).f(tol).p(s).t(hand_tail(f, defer_tail)));
  return 0;
}
int launch_w_reduce_pack(const float* slab, int nblk, int k, int n_pad, const HFinalizeArgs& fin, const float* h_new, int nx, int ny, int p_pad,
                         int with_halo, void* rec, hipStream_t s) {
  call("launch_w_reduce_pack", Args().p(slab).i(nblk).i(k).i(n_pad).t(fin_id(fin)).p(h_new).i(nx).i(ny).i(p_pad).i(with_halo).p(rec).p(s));
  return 0;
}
int launch_w_finish(const WFinishArgs& a, hipStream_t s) {
  call("launch_w_finish", Args().t(f_id(a)).p(s));
  return 0;
}
int launch_gram(const float* m, int rows, int k, double* part, int part_cap, float* out, hipStream_t s) {
  call("launch_gram", Args().p(m).i(rows).i(k).p(part).i(part_cap).p(out).p(s));
  return 0;
}
int launch_w_finish_l2(const float* a, int n, int n_pad, int m, int k, const float* g, const float* gtg, const float* hh, const float* w_old,
                       float* w_new, const float* fixed_w, float log_shift, hipStream_t s) {
  call("launch_w_finish_l2", Args().p(a).i(n).i(n_pad).i(m).i(k).p(g).p(gtg).p(hh).p(w_old).p(w_new).p(fixed_w).f(log_shift).p(s));
  return 0;
}
int launch_w_reduce_update(const WFinishArgs& f, const void* src, size_t src_stride, int nsrc, float* a_out, const double* hpart, int nblk_h,
                           const double* hstat_rs, size_t rec_hstat_off, double* hstat_out, const HFinalizeArgs* fin, hipStream_t s,
                           WTailArgs* defer_tail) {
  call("launch_w_reduce_update", Args().t(f_id(f)).p(src).u(src_stride).i(nsrc).p(a_out).p(hpart).i(nblk_h).p(hstat_rs).u(rec_hstat_off).p(hstat_out)
                                     .t(fin_id(fin)).p(s).t(hand_tail(f, defer_tail)));
  return 0;
}
int launch_w_update_tail(const WTailArgs& t, hipStream_t s) {
  call("launch_w_update_tail", Args().t(tail_id(t)).p(s));
  return 0;
}
int launch_w_exchange_update(const WFinishArgs& f, const void* slabs, size_t slab_stride, int nslab, float* a_out, double* hstat_out,
                             const HFinalizeArgs& fin, const struct ::espm_xchg* xc, unsigned int seq, const float* h_new, int nx, int ny,
                             int p_pad, int with_halo, hipStream_t s, WTailArgs* defer_tail, double* simplex_bparts) {
  // (with the bracket's partials the simplex update follows and forms the tail: this launch then has none, mu_w_exchange.hip)
  call("launch_w_exchange_update", Args().t(f_id(f)).p(slabs).u(slab_stride).i(nslab).p(a_out).p(hstat_out).t(fin_id(fin)).t(x_id(xc)).u(seq).p(h_new)
                                       .i(nx).i(ny).i(p_pad).i(with_halo).p(s).t(simplex_bparts ? (defer_tail ? "tail given" : "no tail") : hand_tail(f, defer_tail))
                                       .p(simplex_bparts));
  return 0;
}
int launch_w_gxchg_update(const WFinishArgs& f, const struct ::espm_xchg* xc, unsigned int seq, const double* hstat_local, double* hstat_out,
                          const float* h_new, int nx, int ny, int p_pad, int with_halo, hipStream_t s) {
  call("launch_w_gxchg_update", Args().t(f_id(f)).t(x_id(xc)).u(seq).p(hstat_local).p(hstat_out).p(h_new).i(nx).i(ny).i(p_pad).i(with_halo).p(s));
  return 0;
}
int launch_pack_x(const void* src, int src_dtype, int src_layout, int64_t ld, int n, int p, void* x_cm, void* x_pm, int x_dtype, int n_pad,
                  int p_pad, int x_tile, int n_cm, hipStream_t s) {
  call("launch_pack_x", Args().p(src).i(src_dtype).i(src_layout).i(ld).i(n).i(p).p(x_cm).p(x_pm).i(x_dtype).i(n_pad).i(p_pad).i(x_tile).i(n_cm).p(s));
  return 0;
}
int launch_hstat(const float* h, int k, int p, int p_pad, double* out, hipStream_t s) {
  call("launch_hstat", Args().p(h).i(k).i(p).i(p_pad).p(out).p(s));
  return 0;
}
int launch_dichotomy(const double* num, const double* den, int k, int p, int den_cols, double eps, double tol, int maxit, double* nu_out,
                     int32_t* status, hipStream_t s) {
  call("launch_dichotomy", Args().p(num).p(den).i(k).i(p).i(den_cols).f(eps).f(tol).i(maxit).p(nu_out).p(status).p(s));
  return 0;
}
int launch_shard_pack(const float* a, const double* hstat, const float* h_new, int k, int n_pad, int nx, int ny, int p_pad, int with_halo,
                      void* rec, hipStream_t s) {
  call("launch_shard_pack", Args().p(a).p(hstat).p(h_new).i(k).i(n_pad).i(nx).i(ny).i(p_pad).i(with_halo).p(rec).p(s));
  return 0;
}
int launch_shard_combine(const void* recs, int world, size_t stride, int na, float* a_out, double* hstat_out, hipStream_t s, const float* bw_old,
                         double* bparts, int n, int k, int n_pad) {
  call("launch_shard_combine", Args().p(recs).i(world).u(stride).i(na).p(a_out).p(hstat_out).p(s).p(bw_old).p(bparts).i(n).i(k).i(n_pad));
  return 0;
}
int launch_simplex_root_f32(const float* num, const float* den, int k, int p, float eps, float tol, int maxit, int fast_exit, float* delta_out,
                            float* e_out, int32_t* status, hipStream_t s) {
  call("launch_simplex_root_f32", Args().p(num).p(den).i(k).i(p).f(eps).f(tol).i(maxit).i(fast_exit).p(delta_out).p(e_out).p(status).p(s));
  return 0;
}
int launch_dichotomy_acc(double a, const double* b, const double* c, int k, int p, int b_cols, double eps, double tol, int maxit, double* nu_out,
                         int32_t* status, hipStream_t s) {
  call("launch_dichotomy_acc", Args().f(a).p(b).p(c).i(k).i(p).i(b_cols).f(eps).f(tol).i(maxit).p(nu_out).p(status).p(s));
  return 0;
}
int launch_dichotomy_pg(const double* a, int k, int p, double eps, double tol, int maxit, double* nu_out, hipStream_t s) {
  call("launch_dichotomy_pg", Args().p(a).i(k).i(p).f(eps).f(tol).i(maxit).p(nu_out).p(s));
  return 0;
}
int launch_laplacian(const float* h, int k, int nx, int ny, int64_t ld, float* out, hipStream_t s) {
  call("launch_laplacian", Args().p(h).i(k).i(nx).i(ny).i(ld).p(out).p(s));
  return 0;
}
int launch_linesearch_terms(const float* h_old, const float* h_new, int k, int p, int p_pad, int nx, int ny, int grid_mode, const float* old_top,
                            const float* old_bot, const float* new_top, const float* new_bot, double* part, double* out, hipStream_t s) {
  call("launch_linesearch_terms", Args().p(h_old).p(h_new).i(k).i(p).i(p_pad).i(nx).i(ny).i(grid_mode).p(old_top).p(old_bot).p(new_top).p(new_bot)
                                      .p(part).p(out).p(s));
  return 0;
}

}  // namespace espm

extern "C" {

const void* espm_xchg_records(const espm_xchg* x, int parity) {
  return x ? x->mailbox + (size_t)(parity & 1) * x->world * x->record_bytes : nullptr;
}
int espm_xchg_post(espm_xchg* x, uint32_t seq, espm_stream_t s) {
  call("espm_xchg_post", Args().t(x_id(x)).u(seq).p(s));
  return 0;
}
int espm_xchg_wait(espm_xchg* x, uint32_t seq, espm_stream_t s) {
  call("espm_xchg_wait", Args().t(x_id(x)).u(seq).p(s));
  return 0;
}

// ---- the HIP runtime: success, and the arguments ----------------------------------------------------------------------------------
// events are fake addresses in the region "ev", numbered in the order of their creation within a case
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = reinterpret_cast<hipEvent_t>(lt::g_ev_base + g_events++);
  call("hipEventCreate", Args().p(*e));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  call("hipEventDestroy", Args().p(e));
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = 0.5f;
  call("hipEventElapsedTime", Args().p(a).p(b));
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  call("hipEventRecord", Args().p(e).p(s));
  return hipSuccess;
}
hipError_t hipGetDevice(int* d) {
  *d = 0;
  call("hipGetDevice", Args());
  return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int d) {
  prop->multiProcessorCount = 256;
  call("hipGetDeviceProperties", Args().i(d));
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stubbed HIP runtime"; }
hipError_t hipMemset2DAsync(void* dst, size_t pitch, int value, size_t width, size_t height, hipStream_t s) {
  call("hipMemset2DAsync", Args().p(dst).u(pitch).i(value).u(width).u(height).p(s));
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  call("hipStreamSynchronize", Args().p(s));
  return hipSuccess;
}

}  // extern "C"
