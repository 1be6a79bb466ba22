// extern "C" surface of libespm_mu.so (declared in include/espm_mu.h): argument checking, kernel
// selection and launch sequencing.  No allocation, no host synchronisation.
#include <vector>
#include <stdarg.h>
#include <stdio.h>

#include "mu_common.hpp"
#include "mu_w_plan.hpp"
#include "mu_xchg.hpp"

namespace espm {

static thread_local char g_err[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return ESPM_OK;
  return set_error(ESPM_EHIP, "%s: %s", what, hipGetErrorString(e));
}

static int roundup(int v, int m) { return (v + m - 1) / m * m; }

// every field of espm_mu_state, in declaration order (tests compare espm_mu_state_layout() with the header: a field missing here fails them)
#define ESPM_MU_STATE_FIELDS(F) \
  F(struct_size) F(abi_version) F(n) F(m) F(k) F(p) F(nx) F(ny) F(n_pad) F(p_pad) F(x_dtype) F(tile_px) F(nblk_w) \
  F(x_tile) F(n_cm) F(h_variant) F(p_total) F(simplex_h) F(simplex_w) F(grid_mode) F(compute_loss) F(lambda_l) \
  F(sigma_l) F(eps_reg) F(log_shift) F(dicotomy_tol) F(rel_tol) F(xscale) F(gw_floor) F(x_cm) F(x_pm) F(g) \
  F(colsum_g) F(w) F(gw_s) F(colsum_gw) F(gw_a) F(gw_p) F(h) F(h_t) F(mu) F(fixed_h) F(fixed_w) F(simplex_rows) \
  F(halo_top) F(halo_bot) F(hpart) F(hstat) F(a_slab) F(a) F(w_scratch) F(hist) F(hist_len) F(cur) F(it) F(ell_h) \
  F(ell_h_off) F(ell_klc) F(ell_w) F(ell_w_off) F(chan_perm) F(ell_cbits) F(n_cg) F(pix_perm) F(g_t) F(breg_sr_px) \
  F(breg_sr_ch) F(h_rule) F(pg_gamma_w) F(pg_q) F(ell_fill_px) F(ell_fill_num) F(ell_fill_n) F(tail_mode) F(no_fused) \
  F(ell_pb) F(ell_stream) F(ell_hv_n) F(ell_hv_npx) F(ell_hv_ngrp) F(ell_hv_px) F(ell_hv_px_off) F(ell_hv_pm) F(ell_hv_klc) F(ell_hv_kl) \
  F(ell_hv_grp) F(ell_hv_grp_off) F(ell_hv_wm) F(hpart_alt) F(ell_blk_cnt) F(ell_keep_h) F(ell_keep_w)

// the caller's view of the state must be this library's (include/espm_mu.h, ESPM_MU_ABI_VERSION): checked before any field is read
static int check_abi(const espm_mu_state* st) {
  ESPM_REQUIRE(st != nullptr, "state is NULL");
  ESPM_REQUIRE(st->struct_size == (uint32_t)sizeof(espm_mu_state) && st->abi_version == (uint32_t)ESPM_MU_ABI_VERSION,
               "espm_mu_state of %u bytes, ABI %u handed to a library built for %zu bytes, ABI %d: the binding's copy of the layout has drifted",
               st->struct_size, st->abi_version, sizeof(espm_mu_state), ESPM_MU_ABI_VERSION);
  return ESPM_OK;
}

static int check_state(const espm_mu_state* st) {
  if (int rc = check_abi(st)) return rc;
  ESPM_REQUIRE(st->n >= 1 && st->p >= 1, "n=%d, p=%d must be >= 1", st->n, st->p);
  if (st->k < ESPM_MIN_K || st->k > ESPM_MAX_K)
    return set_error(ESPM_EUNSUPPORTED, "k=%d: this build supports %d..%d components", st->k, ESPM_MIN_K, ESPM_MAX_K);
  ESPM_REQUIRE(st->n_pad == roundup(st->n, ESPM_NPAD) && st->p_pad == roundup(st->p, ESPM_PPAD),
               "n_pad/p_pad (%d, %d) do not match n, p (%d, %d); call espm_mu_query", st->n_pad, st->p_pad, st->n,
               st->p);
  ESPM_REQUIRE(st->x_dtype >= ESPM_X_F32 && st->x_dtype <= ESPM_X_ELL, "bad x_dtype %d", st->x_dtype);
  if (st->x_dtype == ESPM_X_ELL) {
    ESPM_REQUIRE(st->ell_h && st->ell_h_off && st->ell_klc && st->ell_w && st->ell_w_off && st->chan_perm && st->pix_perm,
                 "the sparse count store needs ell_h, ell_h_off, ell_klc, ell_w, ell_w_off, chan_perm and pix_perm");
    ESPM_REQUIRE((st->tile_px == 64 || st->tile_px == 128 || st->tile_px == 256 || st->tile_px == ESPM_ELL_TILE) &&
                     st->ell_pb == 2 * st->tile_px && st->nblk_w == (st->p + st->ell_pb - 1) / st->ell_pb &&
                     st->n_cg == (st->n + 63) / 64 && st->h_variant == 0,
                 "sparse count store: tile_px must be 64..%d, ell_pb 2 tile_px, nblk_w ceil(p / ell_pb), n_cg ceil(n / 64); call espm_mu_query",
                 ESPM_ELL_TILE);
  }
  ESPM_REQUIRE(st->ell_stream == 0 || (st->ell_stream == 1 && st->x_dtype == ESPM_X_ELL), "ell_stream=%d: 0, or 1 with the sparse store", st->ell_stream);
  // (the kept part of streamed lists: ignored without ell_stream, otherwise counted in list groups of a tile and channel groups of a block)
  ESPM_REQUIRE(st->ell_stream == 0 || (st->ell_keep_h >= 0 && st->ell_keep_h <= st->tile_px / 64 && st->ell_keep_w >= 0 && st->ell_keep_w <= (st->n_cg < 255 ? st->n_cg : 255)),
               "ell_keep_h=%d, ell_keep_w=%d: 0..%d list groups of a tile, 0..%d channel groups", st->ell_keep_h, st->ell_keep_w, st->tile_px / 64, st->n_cg);
  ESPM_REQUIRE(st->ell_fill_n >= 0 && (st->ell_fill_n == 0 || (st->x_dtype == ESPM_X_ELL && st->ell_fill_px && st->ell_fill_num)),
               "ell_fill_n=%d needs the sparse store, ell_fill_px and ell_fill_num", st->ell_fill_n);
  ESPM_REQUIRE(st->ell_hv_n >= 0 && (st->ell_hv_n == 0 || (st->x_dtype == ESPM_X_ELL && st->h_rule == 0 && !st->breg_sr_px && st->ell_hv_npx >= 1 &&
                                                          st->ell_hv_npx <= st->ell_hv_n && st->ell_hv_ngrp >= 1 && st->ell_hv_ngrp <= st->ell_hv_n &&
                                                          st->ell_hv_px && st->ell_hv_px_off && st->ell_hv_pm && st->ell_hv_klc && st->ell_hv_kl &&
                                                          st->ell_hv_grp && st->ell_hv_grp_off && st->ell_hv_wm && st->ell_fill_num)),
               "ell_hv_n=%d needs the sparse store with the default H rule, 1 <= ell_hv_npx, ell_hv_ngrp <= ell_hv_n, every ell_hv_* array and "
               "ell_fill_num", st->ell_hv_n);
  ESPM_REQUIRE(st->grid_mode == 0 || (st->nx >= 1 && st->ny >= 1 && st->nx * st->ny == st->p),
               "grid %d x %d does not match p=%d", st->nx, st->ny, st->p);
  ESPM_REQUIRE(st->xscale > 0.f, "xscale must be positive");
  ESPM_REQUIRE(st->n_cm == roundup(st->n, ESPM_NCM), "n_cm must be roundup(n, %d)", ESPM_NCM);
  ESPM_REQUIRE((st->breg_sr_px == nullptr) == (st->breg_sr_ch == nullptr), "breg_sr_px and breg_sr_ch come together");
  ESPM_REQUIRE(!st->breg_sr_px || (st->m == 0 && !st->simplex_w && st->n <= 4096),
               "the Bregman variant is built for G = identity without simplex_W (and n <= 4096)");
  ESPM_REQUIRE(st->h_rule == 0 || ((st->h_rule == 1 || st->h_rule == 2) && !st->breg_sr_px), "h_rule must be 0, 1 or 2 (1, 2 not with the Bregman variant)");
  ESPM_REQUIRE(!(st->pg_gamma_w > 0.f) || (!st->simplex_w && !st->breg_sr_px && (st->m == 0 || (long)st->m * st->k <= 8192)),
               "the projected-gradient W step has no simplex over W (updates.py:368-369), no Bregman variant, and needs M k <= 8192 with a dictionary");
  ESPM_REQUIRE(st->h_variant == 0, "h_variant %d is not built (the matrix-core H-step was retired, DESIGN.md)", st->h_variant);
  ESPM_REQUIRE(st->x_tile >= 64 && ESPM_PPAD % st->x_tile == 0 && st->x_tile % st->tile_px == 0,
               "x_tile=%d must divide %d and be a multiple of tile_px=%d", st->x_tile, ESPM_PPAD, st->tile_px);
  ESPM_REQUIRE(st->m >= 0, "m must be >= 0");
  ESPM_REQUIRE(st->m == 0 || (st->g && st->colsum_g), "m=%d needs g and colsum_g", st->m);
  if (st->log_shift > 0.f && st->simplex_h && (double)st->k * (double)st->log_shift >= 1.0)
    return set_error(ESPM_ENOSOLUTION, "No solution exists! (k * log_shift >= 1)");
  return ESPM_OK;
}

static int nblk_h(const espm_mu_state* st) { return (st->p + st->tile_px - 1) / st->tile_px; }

// Sparse store, before an H-step launch on h[src]: the numerators of the fill pixels and of the heavy elements' pixels, which the
// epilogue adds (include/espm_mu.h, ell_fill_*, ell_hv_*)
static int ell_pre_h(const espm_mu_state* st, int src, hipStream_t s) {
  const int ld = st->ell_fill_n + (st->ell_hv_n > 0 ? st->ell_hv_npx : 0);
  if (st->ell_fill_n > 0)
    if (int rc = launch_ell_fill_num(st->gw_s, st->h[src], st->ell_fill_px, st->ell_fill_n, st->n, st->k, st->p_pad, st->log_shift,
                                     st->ell_fill_num, s, ld))
      return rc;
  return st->ell_hv_n > 0 ? launch_ell_hv_h(st, src, ld, s) : ESPM_OK;
}

// ... and after it: the heavy elements' part of R H'^T into the slabs (w: the W accumulation has run, with H' = h[hnew] or, hnew < 0,
// h_t) and their loss into the first record (loss: the H-step has written its records)
static int ell_post(const espm_mu_state* st, int hnew, bool w, bool loss, hipStream_t s) {
  if (st->ell_hv_n <= 0) return ESPM_OK;
  if (hnew >= 0) return launch_ell_hv_post(st, st->h[hnew], (size_t)st->p_pad, 1, w, loss, s);
  return launch_ell_hv_post(st, st->h_t, 1, ESPM_KP, w, loss, s);
}

// Both half-steps in one launch (mu_fused_kernel.hpp): sparse store, the default H rule, LDS for the table and the numerators
// of a block of ell_pb pixels.  One record per pixel BLOCK.  (Round 2 kept the two launches below blocks of 512 pixels - images
// under 2^17 pixels, shards - where one workgroup per CU left the CU idle through its serial phases.  With those phases cut
// in round 3 - prologue loads issued together, the update's inputs staged by the prologue, one barrier around the record
// reduction, no extra workgroup for the W update's tail - the fused launch wins at every block size: a 64-row shard 47.4 -> 42.8 us
// per iteration, profiles/r03d_shard_iter*.log - where the blocks cover the chip (ESPM_FUSED_MIN_BLOCKS); an image of fewer, small
// blocks keeps the two launches, whose smaller workgroups spread over more CUs.)
static bool fused_ok(const espm_mu_state* st) {
  return ESPM_MIN_K <= 8 && st->x_dtype == ESPM_X_ELL && st->h_rule == 0 && st->no_fused != 1 &&
         (st->ell_pb >= ESPM_FUSED_MIN_PB || st->nblk_w >= ESPM_FUSED_MIN_BLOCKS || st->no_fused == 3) &&
         fused_ell_lds_bytes(st->n_pad, st->k, st->ell_pb) <= ESPM_ELL_LDS_MAX;
}
static HStepArgs fused_h_args(const espm_mu_state* st, int src) {
  HStepArgs a = make_h_args(st, src, 1);
  a.rec_nb = nblk_h(st);
  return a;
}

// ---- argument checks that several entry points share (callers match on the texts) ---------------------------------------------------
// history slot `slot` exists - and, need_next, slot + 1 too, where the W update's rel_W goes
static int check_slot(const espm_mu_state* st, int slot, bool need_next) {
  if (slot >= 0 && slot + (need_next ? 1 : 0) < st->hist_len) return ESPM_OK;
  return set_error(ESPM_EINVAL, need_next ? "history slot %d + 1 outside [0, %d)" : "history slot %d outside [0, %d)", slot, st->hist_len);
}
static int check_room(const espm_mu_state* st, int n_iter) {
  ESPM_REQUIRE(st->it + n_iter < st->hist_len, "history too short: it=%d + %d >= %d", st->it, n_iter, st->hist_len);
  return ESPM_OK;
}
// the caller's image as (dtype, layout, leading dimension); `what` names the entry point (espm_mu_pack_x words the last one without ld)
static int check_src_view(const char* what, int dtype, int layout, int64_t ld, int n, int p, bool say_ld = true) {
  ESPM_REQUIRE(dtype == ESPM_SRC_F32 || dtype == ESPM_SRC_F64, "%s: bad src_dtype %d", what, dtype);
  ESPM_REQUIRE(layout == ESPM_LAYOUT_CM || layout == ESPM_LAYOUT_PM, "%s: bad layout %d", what, layout);
  if (ld >= (layout == ESPM_LAYOUT_CM ? p : n)) return ESPM_OK;
  return say_ld ? set_error(ESPM_EINVAL, "%s: ld=%lld too small", what, (long long)ld) : set_error(ESPM_EINVAL, "%s: leading dimension too small", what);
}

}  // namespace espm

using namespace espm;

extern "C" {

const char* espm_mu_version(void) { return "espm_mu 0.3 (gfx950)"; }
const char* espm_mu_last_error(void) { return g_err; }

size_t espm_mu_state_size(void) { return sizeof(espm_mu_state); }
int espm_mu_abi_version(void) { return ESPM_MU_ABI_VERSION; }

const char* espm_mu_state_layout(void) {
  static char text[4096];
  static bool done = false;
  if (!done) {
    size_t len = 0;
#define F(name)                                                                                                      \
  len += (size_t)snprintf(text + len, sizeof(text) - len, #name ":%zu:%zu;", offsetof(espm_mu_state, name), \
                          sizeof(((espm_mu_state*)nullptr)->name));
    ESPM_MU_STATE_FIELDS(F)
#undef F
    done = true;
  }
  return text;
}

int espm_mu_query(espm_mu_state* st) {
  if (int rc = check_abi(st)) return rc;
  ESPM_REQUIRE(st->n >= 1 && st->p >= 1, "n=%d, p=%d must be >= 1", st->n, st->p);
  st->n_pad = roundup(st->n, ESPM_NPAD);
  st->p_pad = roundup(st->p, ESPM_PPAD);
  int cus = 256;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
      prop.multiProcessorCount > 0)
    cus = prop.multiProcessorCount;
  // H-step: 256-pixel tiles (4 waves) when that gives >= 2 workgroups per CU, else 128-pixel tiles
  // with 8 waves splitting the channel range (tuned on MI355X, tools/tune).
  // (the widest build, 17..32 components: 128-pixel tiles only - the partial numerators of a 256-pixel tile would take 68..128 KB of LDS)
  const int big = 256;
  st->tile_px = (ESPM_KP <= 16 && (st->p + big - 1) / big >= 2 * cus) ? big : 128;
  st->x_tile = st->tile_px;
  st->n_cm = roundup(st->n, ESPM_NCM);
  st->h_variant = 0;
  st->n_cg = (st->n + 63) / 64;
  st->ell_pb = 0;
  if (st->x_dtype == ESPM_X_ELL) {  // sparse count store: fixed decomposition (mu_ell_kernel.hpp)
    // H-step: 512 pixels per workgroup (8 waves, one 64-pixel list group each); smaller images split every group
    // over 2, 4 or 8 waves so that about two workgroups per CU remain
    st->tile_px = ESPM_ELL_TILE;
    while (st->tile_px > 64 && (st->p + st->tile_px - 1) / st->tile_px < 2 * cus) st->tile_px /= 2;
    st->x_tile = st->tile_px;
    // W accumulation: blocks of two H tiles (1024 pixels for an image that fills the chip; about one block per CU below that,
    // so that one workgroup can own a block through both half-steps: mu_fused_kernel.hpp)
    st->ell_pb = 2 * st->tile_px;
    st->nblk_w = (st->p + st->ell_pb - 1) / st->ell_pb;
    st->ell_cbits = 1;
    while ((1 << st->ell_cbits) < st->n) ++st->ell_cbits;
    if (st->ell_cbits > 14) return set_error(ESPM_EUNSUPPORTED, "sparse count store: n=%d needs more than 14 index bits", st->n);
    return ESPM_OK;
  }
  // W accumulation: about 2 workgroups per CU, at least 16 pixels each.
  const int ychunks = (st->x_dtype != ESPM_X_F32 && ESPM_MIN_K <= 8) ? (st->n_pad + 2047) / 2048 : (st->n_pad + 1023) / 1024;
  int target = (2 * cus + ychunks - 1) / ychunks;
  int by_px = (st->p + 15) / 16;
  int nb = target < by_px ? target : by_px;
  if (nb < 1) nb = 1;
  const int ppb = (st->p + nb - 1) / nb;
  st->nblk_w = (st->p + ppb - 1) / ppb;
  return ESPM_OK;
}

int espm_mu_pack_x(const void* src, int src_dtype, int src_layout, int64_t ld, int n, int p, void* x_cm, void* x_pm,
                   int x_dtype, int n_pad, int p_pad, int x_tile, int n_cm, espm_stream_t stream) {
  ESPM_REQUIRE(src && x_pm, "pack_x: NULL pointer");  // x_cm may be NULL (sparse store ingest needs x_pm only)
  ESPM_REQUIRE(n >= 1 && p >= 1 && n_pad == roundup(n, ESPM_NPAD) && p_pad == roundup(p, ESPM_PPAD),
               "pack_x: bad shape n=%d p=%d n_pad=%d p_pad=%d", n, p, n_pad, p_pad);
  if (int rc = check_src_view("pack_x", src_dtype, src_layout, ld, n, p, false)) return rc;
  ESPM_REQUIRE(x_tile >= 64 && ESPM_PPAD % x_tile == 0, "pack_x: x_tile %d must divide %d", x_tile, ESPM_PPAD);
  ESPM_REQUIRE(n_cm == roundup(n, ESPM_NCM), "pack_x: n_cm must be roundup(n, %d)", ESPM_NCM);
  return launch_pack_x(src, src_dtype, src_layout, ld, n, p, x_cm, x_pm, x_dtype, n_pad, p_pad, x_tile, n_cm,
                       static_cast<hipStream_t>(stream));
}

static int check_ell_geometry(const espm_mu_state* st) {
  if (int rc = check_abi(st)) return rc;
  ESPM_REQUIRE(st->x_dtype == ESPM_X_ELL && st->n >= 1 && st->p >= 1 && st->n_pad == roundup(st->n, ESPM_NPAD) &&
                   st->p_pad == roundup(st->p, ESPM_PPAD) && st->n_cg == (st->n + 63) / 64 &&
                   st->ell_pb == 2 * st->tile_px && st->nblk_w == (st->p + st->ell_pb - 1) / st->ell_pb && st->ell_cbits >= 1 &&
                   st->ell_cbits <= 14 && (1 << st->ell_cbits) >= st->n &&
                   (st->tile_px == 64 || st->tile_px == 128 || st->tile_px == 256 || st->tile_px == ESPM_ELL_TILE),
               "sparse store builder: set x_dtype = ESPM_X_ELL and call espm_mu_query first");
  return ESPM_OK;
}

int espm_mu_ell_count_hist(const espm_mu_state* st, const void* x_pm_u8, int32_t* cnt_px, int32_t* cnt_bc, float* ell_klc, uint8_t* bkt_px,
                           uint8_t* bkt_bc, espm_stream_t stream) {
  if (int rc = check_ell_geometry(st)) return rc;
  ESPM_REQUIRE(x_pm_u8 && cnt_px && cnt_bc && ell_klc, "ell_count: NULL pointer");
  ESPM_REQUIRE((bkt_px == nullptr) == (bkt_bc == nullptr), "ell_count: the two histograms come together");
  return launch_ell_count(static_cast<const uint8_t*>(x_pm_u8), st->n, st->n_pad, st->p, st->p_pad, st->ell_cbits, st->n_cg,
                          st->nblk_w, st->ell_pb, cnt_px, cnt_bc, ell_klc, static_cast<hipStream_t>(stream), bkt_px, bkt_bc);
}

int espm_mu_ell_count(const espm_mu_state* st, const void* x_pm_u8, int32_t* cnt_px, int32_t* cnt_bc, float* ell_klc,
                      espm_stream_t stream) {
  return espm_mu_ell_count_hist(st, x_pm_u8, cnt_px, cnt_bc, ell_klc, nullptr, nullptr, stream);
}

int espm_mu_ell_plan(const espm_mu_state* st, const int32_t* cnt_px, const int32_t* cnt_bc, int32_t* chan_perm,
                     int32_t* pix_perm, int32_t* ell_h_off, int32_t* ell_w_off, int64_t* rows, espm_stream_t stream) {
  if (int rc = check_ell_geometry(st)) return rc;
  ESPM_REQUIRE(cnt_px && cnt_bc && chan_perm && pix_perm && ell_h_off && ell_w_off && rows, "ell_plan: NULL pointer");
  return launch_ell_plan(cnt_px, cnt_bc, st->n, st->n_cg, st->nblk_w, st->p_pad, st->tile_px, chan_perm, pix_perm, ell_h_off,
                         ell_w_off, reinterpret_cast<long long*>(rows), static_cast<hipStream_t>(stream));
}

int espm_mu_ell_fill(const espm_mu_state* st, const void* x_pm_u8, const int32_t* chan_perm, const int32_t* pix_perm,
                     const int32_t* ell_h_off, const int32_t* ell_w_off, uint32_t* ell_h, uint32_t* ell_w,
                     espm_stream_t stream) {
  return espm_mu_ell_fill_hist(st, x_pm_u8, chan_perm, pix_perm, ell_h_off, ell_w_off, ell_h, ell_w, nullptr, nullptr, stream);
}

int espm_mu_ell_fill_hist(const espm_mu_state* st, const void* x_pm_u8, const int32_t* chan_perm, const int32_t* pix_perm,
                          const int32_t* ell_h_off, const int32_t* ell_w_off, uint32_t* ell_h, uint32_t* ell_w, const uint8_t* bkt_px,
                          const uint8_t* bkt_bc, espm_stream_t stream) {
  if (int rc = check_ell_geometry(st)) return rc;
  ESPM_REQUIRE((bkt_px == nullptr) == (bkt_bc == nullptr), "ell_fill: the two histograms come together");
  ESPM_REQUIRE(x_pm_u8 && chan_perm && pix_perm && ell_h_off && ell_w_off && ell_h && ell_w, "ell_fill: NULL pointer");
  // st->x_cm, if set: the 8-bit counts once more, channel-major in tiles of ESPM_PPAD pixels (include/espm_mu.h) - the channel lists are filled from it
  ESPM_REQUIRE(!st->x_cm || st->n_cm == roundup(st->n, ESPM_NCM), "ell_fill: x_cm is set but n_cm=%d is not n rounded up to %d", st->n_cm, ESPM_NCM);
  return launch_ell_fill(static_cast<const uint8_t*>(x_pm_u8), st->n, st->n_pad, st->p, st->p_pad, st->ell_cbits, st->n_cg,
                         st->nblk_w, st->tile_px, st->ell_pb, chan_perm, pix_perm, ell_h_off, ell_w_off, ell_h, ell_w,
                         static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(st->x_cm), st->n_cm, bkt_px, bkt_bc);
}

int espm_mu_ell_heavy_count(const espm_mu_state* st, const void* x, int src_dtype, int src_layout, int64_t ld, uint8_t* x_pm_u8,
                            uint8_t* x_cm_u8, int32_t* cnt_px, espm_stream_t stream) {
  if (int rc = check_ell_geometry(st)) return rc;
  ESPM_REQUIRE(x && x_pm_u8 && cnt_px, "ell_heavy_count: NULL pointer");
  if (int rc = check_src_view("ell_heavy_count", src_dtype, src_layout, ld, st->n, st->p)) return rc;
  ESPM_REQUIRE(!x_cm_u8 || st->n_cm == roundup(st->n, ESPM_NCM), "ell_heavy_count: x_cm is set but n_cm=%d is not n rounded up to %d", st->n_cm, ESPM_NCM);
  return launch_ell_hv_count(x, src_dtype, src_layout, ld, st->n, st->p, st->n_pad, st->n_cm, x_pm_u8, x_cm_u8, cnt_px,
                             static_cast<hipStream_t>(stream));
}

int espm_mu_ell_heavy_fill(const espm_mu_state* st, const void* x, int src_dtype, int src_layout, int64_t ld, const int32_t* px_off,
                           int32_t* hv_pm, espm_stream_t stream) {
  if (int rc = check_ell_geometry(st)) return rc;
  ESPM_REQUIRE(x && px_off && hv_pm, "ell_heavy_fill: NULL pointer");
  if (int rc = check_src_view("ell_heavy_fill", src_dtype, src_layout, ld, st->n, st->p)) return rc;
  return launch_ell_hv_fill(x, src_dtype, src_layout, ld, st->n, st->p, px_off, hv_pm, static_cast<hipStream_t>(stream));
}

int espm_mu_hstat(const espm_mu_state* st, int which, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(which == 0 || which == 1, "which must be 0/1");
  return launch_hstat(st->h[which], st->k, st->p, st->p_pad, st->hstat[which], static_cast<hipStream_t>(stream));
}

// The forms of the W update that run inside the slab reduction's launches, ahead of launch_w_finish (0: neither - the plan of
// launch_w_finish decides, mu_w_plan.hpp: plan_w_finish).  The half-steps below switch on this; espm_mu_w_update_form returns it.
// ESPM_W_FORM_LOCAL: W' needs nothing global but the row sums of the new H: the reduction workgroups finish W themselves.
// ESPM_W_FORM_SIMPLEX_SPLIT: the simplex over W with G = identity and every row in the simplex: the multipliers follow from
// per-component sums over the channels, so the update runs as two many-workgroup launches (slab reduction + those sums, then
// w_simplex_update_kernel) instead of the reduction and ONE workgroup that finds the multipliers (mu_w_reduce.hip against
// mu_w_finish.hip).  Its tail is the local update's.
static int w_form_ahead(const espm_mu_state* st) {
  if (st->m != 0 || st->n < 64 || st->w_scratch == nullptr) return 0;
  if (!st->simplex_w) return ESPM_W_FORM_LOCAL;
  if (!st->simplex_rows && !st->breg_sr_ch && !(st->pg_gamma_w > 0.f) && st->n_pad % 32 == 0 && st->no_fused != 1) return ESPM_W_FORM_SIMPLEX_SPLIT;
  return 0;
}
static bool w_update_is_local(const espm_mu_state* st) { return w_form_ahead(st) == ESPM_W_FORM_LOCAL; }
static bool w_simplex_split(const espm_mu_state* st) { return w_form_ahead(st) == ESPM_W_FORM_SIMPLEX_SPLIT; }
// where the partials of the bracket live: behind the tail's three arrays of k * nbk doubles in w_scratch (2 n k floats)
static double* simplex_bparts(const espm_mu_state* st) {
  return reinterpret_cast<double*>(st->w_scratch) + 3 * (size_t)st->k * ((st->n_pad + 31) / 32);
}
static bool w_update_has_tail(const espm_mu_state* st) { return w_update_is_local(st) || w_simplex_split(st); }
// Sparse store: the tail of such a W update (column sums of G W', rel_W: one small workgroup, 8 us as a launch of its own) rides in
// the NEXT H-step's launch as an extra workgroup; that H-step sums the partial column sums itself, and the slab reduction that
// follows finds colsum_gw written.  The last tail is a launch of its own.  This is the rule of the library's own loops.  A caller
// that sequences the half-steps itself through tail_mode has ANOTHER one: espm_amd/engine.py (_defers_tail) defers for the local update
// alone, its simplex split pays the tail's launch.  They stay apart: one rule for both would change a path by a launch per iteration.
static bool loop_hands_tail_on(const espm_mu_state* st) {
  return st->x_dtype == ESPM_X_ELL && w_update_has_tail(st) && !(st->pg_q && st->pg_gamma_w > 0.f);
}
static int with_halo(const espm_mu_state* st) { return st->grid_mode && st->lambda_l != 0.f; }
// the simplex over `rows` rows of W has a solution (dicotomy.py:22-23)
static int simplex_w_feasible(const espm_mu_state* st, double rows) {
  if (!(st->log_shift > 0.f && rows * (double)st->log_shift >= 1.0)) return ESPM_OK;
  return set_error(ESPM_ENOSOLUTION, "No solution exists! (rows * log_shift >= 1)");
}

static WFinishArgs finish_args(const espm_mu_state* st, int src, int hsrc, int slot, int update_w) {
  WFinishArgs a;
  a.g = st->m > 0 ? st->g : nullptr;
  a.g_t = st->m > 0 ? st->g_t : nullptr;
  a.colsum_g = st->colsum_g;
  a.w_old = st->w[src];
  a.w_new = update_w ? st->w[1 - src] : st->w[src];
  a.a = st->a;
  a.hstat = st->hstat[hsrc];
  a.fixed_w = st->fixed_w;
  a.simplex_rows = st->simplex_rows;
  a.scratch = st->w_scratch;
  a.breg_sr = st->breg_sr_ch;
  a.pg_gamma_w = st->pg_gamma_w;
  a.pg_q = (st->pg_q && st->pg_gamma_w > 0.f && slot >= 0) ? st->pg_q + 2 * (size_t)slot + 1 : nullptr;
  a.gw_s = st->gw_s;
  a.colsum_gw = st->colsum_gw;
  a.gw_a = nullptr;  // reserved (matrix-core H-step, retired)
  a.gw_p = nullptr;
  a.n_cm = st->n_cm;
  a.hist_slot = (slot >= 0 && st->hist) ? st->hist + (size_t)slot * ESPM_HI_STRIDE : nullptr;
  a.n = st->n;
  a.m = st->m;
  a.k = st->k;
  a.n_pad = st->n_pad;
  a.simplex_w = st->simplex_w;
  a.update_w = update_w;
  a.log_shift = st->log_shift;
  // (the reference's W step has no tolerance argument: it calls dichotomy_simplex with the module constant,
  //  updates.py:61-68 / conf.py - only the H step takes the estimator's dicotomy_tol)
  a.tol = ESPM_W_DICOTOMY_TOL;
  a.rel_tol = st->rel_tol;
  a.xscale = st->xscale;
  a.gw_floor = st->gw_floor;
  return a;
}
// the W update of an iteration: w[src] -> w[1 - src] with the row sums of the new H h[1 - src]; state `slot` -> state slot + 1
static WFinishArgs update_args(const espm_mu_state* st, int src, int slot) { return finish_args(st, src, 1 - src, slot + 1, 1); }

static HFinalizeArgs finalize_args(const espm_mu_state* st, int src, int slot, bool write_hstat) {
  HFinalizeArgs a;
  a.hpart = st->hpart;
  a.colsum_gw = st->colsum_gw;
  a.hstat_in = st->hstat[src];
  a.hstat_out = write_hstat ? st->hstat[1 - src] : nullptr;
  a.hist_slot = st->hist + (size_t)slot * ESPM_HI_STRIDE;
  a.nblk = nblk_h(st);
  a.k = st->k;
  a.compute_loss = st->compute_loss;
  a.have_prev = st->it > 0;
  a.xscale = st->xscale;
  a.pg_q = (st->pg_q && st->h_rule == 2 && write_hstat) ? st->pg_q + 2 * (size_t)slot : nullptr;   // (not for loss-only evaluations)
  return a;
}
static int record(hipEvent_t e, hipStream_t s) { return e ? check_hip(hipEventRecord(e, s), "iterate_timed: record") : (int)ESPM_OK; }

// ---- the half-steps of an iteration, on a checked state.  Who carries the tail of a W update is an argument: the extern "C"
//      functions translate the caller's st->tail_mode into it, the library's loops hand a WTailArgs on ------------------------------
// The H half-step on h[src].  ride: the tail of the W update that produced this state, carried as an extra workgroup (sparse store
// only).  fused (fused_ok): with the W accumulation.  at_launch: an event of espm_mu_iterate_timed right ahead of the H launch itself.
static int h_half(const espm_mu_state* st, int src, int write_h, const WTailArgs* ride, bool fused, hipStream_t s, hipEvent_t at_launch = nullptr) {
  if (st->x_dtype != ESPM_X_ELL) return dispatch_h_step(make_h_args(st, src, write_h), st->x_dtype, st->tile_px, nblk_h(st), s);
  HStepArgs a = fused ? fused_h_args(st, src) : make_h_args(st, src, write_h);
  if (ride) a.tail = *ride, a.cs_parts = ride->parts, a.cs_nbk = ride->nbk, a.tail_on = 1;
  // pixels without counts: the numerator of their log_shift fill first; heavy elements likewise (include/espm_mu.h)
  if (int rc = ell_pre_h(st, src, s)) return rc;
  if (int rc = record(at_launch, s)) return rc;
  if (fused) {
    if (int rc = launch_fused_ell(a, make_w_args(st), st->nblk_w, s, st->no_fused == 2, st->ell_stream ? (1 | st->ell_keep_h << 8 | st->ell_keep_w << 16) : 0)) return rc;   // (keep values: 0..255, check_state)
    return ell_post(st, 1 - src, true, true, s);
  }
  if (int rc = launch_h_ell(a, nblk_h(st), s)) return rc;
  return ell_post(st, -1, false, true, s);
}
// a tail on its way to the H-step that carries it (on: null when there is none)
struct Ride {
  WTailArgs tail;
  const WTailArgs* on = nullptr;
};
// ESPM_TAIL_RIDE: the tail that the caller has the H-step on h[src] carry (sparse store)
static int ride_of_tail_mode(const espm_mu_state* st, int src, Ride* r) {
  if (st->x_dtype != ESPM_X_ELL || !(st->tail_mode & ESPM_TAIL_RIDE)) return ESPM_OK;
  ESPM_REQUIRE(st->it >= 1 && w_update_has_tail(st), "tail_mode: no local W update produced state %d", st->it);
  r->tail = make_w_tail_args(update_args(st, 1 - src, st->it - 1));
  r->on = &r->tail;
  return ESPM_OK;
}
// ESPM_TAIL_DEFER: where a finish call leaves the tail that the caller has carried later
static WTailArgs* left_out_of(const espm_mu_state* st, WTailArgs* left_out) { return (st->tail_mode & ESPM_TAIL_DEFER) ? left_out : nullptr; }

static int loss_only(const espm_mu_state* st, int src, int slot, const WTailArgs* ride, hipStream_t s) {
  if (int rc = h_half(st, src, 0, ride, false, s)) return rc;
  return launch_h_finalize(finalize_args(st, src, slot, false), s);   // (loss-only: does not touch hstat[1 - src])
}

static int w_accum(const espm_mu_state* st, hipStream_t s) {
  ESPM_REQUIRE(st->nblk_w >= 1, "nblk_w must be >= 1");
  if (st->x_dtype != ESPM_X_ELL) return dispatch_w_accum(make_w_args(st), st->k, st->x_dtype, st->nblk_w, s);
  if (int rc = launch_w_ell(make_w_args(st), st->k, st->nblk_w, s)) return rc;
  return ell_post(st, -1, true, false, s);   // (H' = h_t)
}

static int w_finish(const espm_mu_state* st, int src, int hsrc, int slot, hipStream_t s) {
  if (st->simplex_w && !st->simplex_rows)
    if (int rc = simplex_w_feasible(st, st->m > 0 ? st->m : st->n)) return rc;
  return launch_w_finish(finish_args(st, src, hsrc, slot, 1), s);
}
static int simplex_update(const espm_mu_state* st, int src, int slot, WTailArgs* tail_out, hipStream_t s) {
  return launch_w_simplex_update(update_args(st, src, slot), st->a, simplex_bparts(st), (double)ESPM_W_DICOTOMY_TOL, s, tail_out);
}
// The W half-step behind the accumulation: slab reduction and W update w[src] -> w[1 - src].  fin: the reduction of the H-step's
// records rides in the reduction's launch (null: hstat[1 - src] is already reduced).  tail_out: the update's tail is handed to the
// caller instead of being launched (null: launched; the one-workgroup finish has no tail).
static int w_half(const espm_mu_state* st, int src, int slot, const HFinalizeArgs* fin, WTailArgs* tail_out, hipStream_t s) {
  switch (w_form_ahead(st)) {
    case ESPM_W_FORM_LOCAL:
      return launch_w_reduce_update(update_args(st, src, slot), st->a_slab, (size_t)st->k * st->n_pad * sizeof(float), st->nblk_w, st->a,
                                    fin ? st->hpart : nullptr, nblk_h(st), fin ? nullptr : st->hstat[1 - src], 0, nullptr, fin, s, tail_out);
    case ESPM_W_FORM_SIMPLEX_SPLIT:   // st->a_slab -> st->a and the bracket's partials; then the update
      if (int rc = simplex_w_feasible(st, st->n)) return rc;
      if (int rc = launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, fin, s, st->w[src], simplex_bparts(st), st->n, st->k, st->n_pad)) return rc;
      return simplex_update(st, src, slot, tail_out, s);
    default:   // launch_w_finish's plan chooses among the other four forms
      if (int rc = launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, fin, s)) return rc;
      return w_finish(st, src, 1 - src, slot + 1, s);
  }
}
// the same from the gathered records of `world` ranks: their sum, the global statistics of the new H, the W update
static int shard_combine_finish(const espm_mu_state* st, const void* records, int world, int src, int slot, WTailArgs* tail_out, hipStream_t s) {
  const size_t stride = espm_mu_shard_record_bytes(st);
  if (w_update_is_local(st))
    return launch_w_reduce_update(update_args(st, src, slot), records, stride, world, st->a, nullptr, 0, nullptr,
                                  (size_t)st->k * st->n_pad * sizeof(float), st->hstat[1 - src], nullptr, s, tail_out);
  if (w_simplex_split(st)) {   // the sum over the ranks leaves the bracket's sums, many workgroups update
    if (int rc = simplex_w_feasible(st, st->n)) return rc;
    if (int rc = launch_shard_combine(records, world, stride, st->k * st->n_pad, st->a, st->hstat[1 - src], s, st->w[src], simplex_bparts(st), st->n, st->k, st->n_pad)) return rc;
    return simplex_update(st, src, slot, tail_out, s);
  }
  if (int rc = launch_shard_combine(records, world, stride, st->k * st->n_pad, st->a, st->hstat[1 - src], s)) return rc;
  return w_finish(st, src, 1 - src, slot + 1, s);
}

int espm_mu_build_gw(const espm_mu_state* st, int which, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(which == 0 || which == 1, "which must be 0/1");
  return launch_w_finish(finish_args(st, which, 0, -1, 0), static_cast<hipStream_t>(stream));
}

int espm_mu_step_h(const espm_mu_state* st, int src, int write_h, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  Ride r;
  if (int rc = ride_of_tail_mode(st, src, &r)) return rc;
  return h_half(st, src, write_h, r.on, false, static_cast<hipStream_t>(stream));
}

int espm_mu_h_finalize(const espm_mu_state* st, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  if (int rc = check_slot(st, slot, false)) return rc;
  return launch_h_finalize(finalize_args(st, src, slot, true), static_cast<hipStream_t>(stream));
}

int espm_mu_loss_only(const espm_mu_state* st, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  if (int rc = check_slot(st, slot, false)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  Ride r;
  if (int rc = ride_of_tail_mode(st, src, &r)) return rc;
  return loss_only(st, src, slot, r.on, static_cast<hipStream_t>(stream));
}

int espm_mu_w_accum(const espm_mu_state* st, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  return w_accum(st, static_cast<hipStream_t>(stream));
}

int espm_mu_fused_applies(const espm_mu_state* st) {
  if (check_state(st)) return 0;
  return fused_ok(st) ? 1 : 0;
}

int espm_mu_step_hw(const espm_mu_state* st, int src, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool fused = fused_ok(st);
  Ride r;
  if (int rc = ride_of_tail_mode(st, src, &r)) return rc;
  if (int rc = h_half(st, src, 1, r.on, fused, s)) return rc;
  return fused ? ESPM_OK : w_accum(st, s);
}

int espm_mu_w_reduce(const espm_mu_state* st, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  return launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, nullptr, static_cast<hipStream_t>(stream));
}

int espm_mu_w_reduce_finalize(const espm_mu_state* st, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  if (int rc = check_slot(st, slot, false)) return rc;
  const HFinalizeArgs fin = finalize_args(st, src, slot, true);
  return launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, &fin, static_cast<hipStream_t>(stream));
}

int espm_mu_w_finish(const espm_mu_state* st, int src, int hsrc, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE((src == 0 || src == 1) && (hsrc == 0 || hsrc == 1), "src/hsrc must be 0/1");
  ESPM_REQUIRE(slot < st->hist_len, "history slot %d outside [0, %d)", slot, st->hist_len);   // (slot < 0: no history row, no rel_W)
  return w_finish(st, src, hsrc, slot, static_cast<hipStream_t>(stream));
}

int espm_mu_w_reduce_finish(const espm_mu_state* st, int src, int slot, int with_finalize, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  if (int rc = check_slot(st, slot, true)) return rc;
  const HFinalizeArgs fin = finalize_args(st, src, slot, true);
  WTailArgs left_out;
  return w_half(st, src, slot, with_finalize ? &fin : nullptr, left_out_of(st, &left_out), static_cast<hipStream_t>(stream));
}

int espm_mu_shard_combine_finish(const espm_mu_state* st, const void* records, int world, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(records && world >= 1 && (src == 0 || src == 1), "shard_combine_finish: bad arguments");
  if (int rc = check_slot(st, slot, true)) return rc;
  WTailArgs left_out;
  return shard_combine_finish(st, records, world, src, slot, left_out_of(st, &left_out), static_cast<hipStream_t>(stream));
}

int espm_mu_w_update_is_local(const espm_mu_state* st) {
  if (check_state(st)) return 0;
  return w_update_is_local(st) ? 1 : 0;
}

int espm_mu_w_update_form(const espm_mu_state* st, int* detail) {
  if (int rc = check_state(st)) return rc;   // (negative: a state the library cannot read)
  if (detail) *detail = 0;
  if (const int ahead = w_form_ahead(st)) return ahead;
  // what w_half's launch_w_finish plans for an update (its arguments but for the history row, which no form depends on)
  const WFinishPlan pl = plan_w_finish(finish_args(st, st->cur == 1 ? 1 : 0, 0, -1, 1));
  if (detail && pl.form == ESPM_W_FORM_ONE_WG_REGISTERS) *detail = pl.nt | pl.rows << 12 | pl.crows << 16 | pl.gta_all << 20;
  return pl.form;
}

int espm_mu_w_update_tail(const espm_mu_state* st, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE((src == 0 || src == 1) && slot >= 0 && slot + 1 < st->hist_len && w_update_has_tail(st), "w_update_tail: bad arguments");
  return launch_w_update_tail(make_w_tail_args(update_args(st, src, slot)), static_cast<hipStream_t>(stream));
}

// ev (espm_mu_iterate_timed only): 3 HIP events per iteration, recorded on the launch stream ahead of the iteration's first launch,
// between its first launch (the H update - with the W accumulation where the fused kernel applies) and what follows, and behind its last.
// (st->tail_mode is the input of callers that sequence the half-steps themselves: the loop neither reads nor writes it)
static int iterate_impl(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream, hipEvent_t* ev) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(n_iter >= 0, "n_iter must be >= 0");
  if (int rc = check_room(st, n_iter)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool hand_on = loop_hands_tail_on(st);
  // Both half-steps in one launch where the fused kernel applies (mu_fused_kernel.hpp): 2 launches per iteration instead of 3.
  const bool fused = fused_ok(st);
  Ride r;   // the tail of the last W update while an H-step is still to carry it
  int rc;
  for (int i = 0; i < n_iter; ++i) {
    const int cur = st->cur, slot = st->it;
    auto mark = [&](int j) { return record(ev ? ev[3 * i + j] : nullptr, s); };
    // (where the tail is handed on, the first event has always sat behind the sparse store's preparatory passes and the second ahead
    //  of a W accumulation of its own; elsewhere around the whole of what espm_mu_step_hw issues)
    if (!hand_on && (rc = mark(0))) return rc;
    if ((rc = h_half(st, cur, 1, r.on, fused, s, hand_on && ev ? ev[3 * i] : nullptr))) return rc;
    if (hand_on && (rc = mark(1))) return rc;
    if (!fused && (rc = w_accum(st, s))) return rc;   // (with the heavy elements' part of the slabs)
    if (!hand_on && (rc = mark(1))) return rc;
    // slab reduction with the H-step's finalize riding in the same launch, then (or, when W' is local, in it) the W update
    const HFinalizeArgs fin = finalize_args(st, cur, slot, true);
    if ((rc = w_half(st, cur, slot, &fin, hand_on ? &r.tail : nullptr, s))) return rc;
    if ((rc = mark(2))) return rc;
    r.on = hand_on ? &r.tail : nullptr;
    st->cur = 1 - cur;
    st->it = slot + 1;
  }
  if (r.on && (rc = launch_w_update_tail(r.tail, s))) return rc;
  return final_loss ? loss_only(st, st->cur, st->it, nullptr, s) : (int)ESPM_OK;
}

int espm_mu_iterate(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream) { return iterate_impl(st, n_iter, final_loss, stream, nullptr); }

int espm_mu_iterate_timed(espm_mu_state* st, int n_iter, float* first_ms, float* rest_ms, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(n_iter >= 1 && n_iter <= 4096 && first_ms && rest_ms, "iterate_timed: 1..4096 iterations, two host arrays of that length");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<hipEvent_t> ev((size_t)3 * n_iter, nullptr);
  int rc = ESPM_OK;
  for (size_t i = 0; i < ev.size() && !rc; ++i) rc = check_hip(hipEventCreate(&ev[i]), "iterate_timed: event");
  if (!rc) rc = iterate_impl(st, n_iter, 0, stream, ev.data());
  if (!rc) rc = check_hip(hipStreamSynchronize(s), "iterate_timed: synchronize");
  for (int i = 0; i < n_iter && !rc; ++i) {
    rc = check_hip(hipEventElapsedTime(first_ms + i, ev[3 * i], ev[3 * i + 1]), "iterate_timed: elapsed");
    if (!rc) rc = check_hip(hipEventElapsedTime(rest_ms + i, ev[3 * i + 1], ev[3 * i + 2]), "iterate_timed: elapsed");
  }
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  return rc;
}

// ---- H-only iterations (include/espm_mu.h) -------------------------------------------------------------------------------------
static bool h_chain_ok(const espm_mu_state* st) { return st->hpart_alt != nullptr && h_chain_built(st); }

int espm_mu_h_chain_applies(const espm_mu_state* st) {
  if (int rc = check_state(st)) return rc;   // (negative: a state the library cannot read)
  return h_chain_ok(st) ? 1 : 0;
}

int espm_mu_iterate_h(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(n_iter >= 0, "n_iter must be >= 0");
  if (int rc = check_room(st, n_iter)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_iter > 0)   // rel_W of an update that leaves W alone (base.py:323)
    if (int rc = check_hip(hipMemset2DAsync(st->hist + (size_t)(st->it + 1) * ESPM_HI_STRIDE + ESPM_HI_REL_W, ESPM_HI_STRIDE * sizeof(double), 0,
                                            sizeof(double), (size_t)n_iter, s), "iterate_h: rel_W"))
      return rc;
  if (h_chain_ok(st) && n_iter > 0) {
    double* rec[2] = {st->hpart, st->hpart_alt};
    for (int i = 0; i < n_iter; ++i) {
      const int cur = st->cur, slot = st->it;
      HStepArgs a = make_h_args(st, cur, 1);
      a.hpart = rec[i & 1];
      if (i > 0) {   // the records of the step before: their statistics for this step, their history row by the extra workgroup
        a.chain_prev = rec[(i - 1) & 1];
        a.chain_nb = nblk_h(st);
        a.chain_fin_on = 1;
        a.chain_fin = finalize_args(st, 1 - cur, slot - 1, true);
        a.chain_fin.have_prev = slot - 1 > 0;
        a.chain_fin.hpart = a.chain_prev;
      }
      if (st->x_dtype == ESPM_X_ELL)   // pixels without counts: the numerator of their log_shift fill first (include/espm_mu.h)
        if (int rc = ell_pre_h(st, cur, s)) return rc;
      if (int rc = launch_h_chain(a, st->x_dtype, st->tile_px, nblk_h(st), s)) return rc;
      st->cur = 1 - cur;
      st->it = slot + 1;
    }
    // the last step's records
    HFinalizeArgs fin = finalize_args(st, 1 - st->cur, st->it - 1, true);
    fin.have_prev = st->it - 1 > 0;
    fin.hpart = rec[(n_iter - 1) & 1];
    if (int rc = launch_h_finalize(fin, s)) return rc;
  } else {
    for (int i = 0; i < n_iter; ++i) {
      const int cur = st->cur, slot = st->it;
      if (int rc = espm_mu_step_h(st, cur, 1, stream)) return rc;
      if (int rc = launch_h_finalize(finalize_args(st, cur, slot, true), s)) return rc;
      st->cur = 1 - cur;
      st->it = slot + 1;
    }
  }
  return final_loss ? espm_mu_loss_only(st, st->cur, st->it, stream) : (int)ESPM_OK;
}

// the exchange context was created for this state's records
static int check_record_bytes(const char* what, const espm_mu_state* st, const espm_xchg* x) {
  ESPM_REQUIRE(x->record_bytes == espm_mu_shard_record_bytes(st), "%s: the exchange was created for records of %zu bytes, the state packs %zu", what,
               x->record_bytes, espm_mu_shard_record_bytes(st));
  return ESPM_OK;
}

// The sharded W half-step behind the accumulation; fin rides always, tail_out as in w_half.
static int shard_exchange_finish(const espm_mu_state* st, espm_xchg* x, uint32_t seq, int src, int slot, WTailArgs* tail_out, hipStream_t s) {
  const HFinalizeArgs fin = finalize_args(st, src, slot, true);
  const WFinishArgs f = update_args(st, src, slot);
  const size_t slab_bytes = (size_t)st->k * st->n_pad * sizeof(float);
  if (!w_update_is_local(st) && st->no_fused != 1 && w_gsplit_applies(f)) {
    // a dictionary G without a simplex over W: every rank contracts its own A with G and the m k results cross the links as
    // granules (w_gxchg_update_kernel): slab reduction + record reduction, exchange + W update, rows of G W' - three launches
    // (this rank's statistics go to its own record in its own mailbox: the exchange launch sends them on, and writes the global ones)
    double* local = reinterpret_cast<double*>(x->mailbox + (size_t)(seq & 1u) * x->world * x->record_bytes + (size_t)x->rank * x->record_bytes + slab_bytes);
    HFinalizeArgs fin_local = fin;
    fin_local.hstat_out = local;
    if (int rc = launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, &fin_local, s)) return rc;
    return launch_w_gxchg_update(f, x, seq, local, st->hstat[1 - src], st->h[1 - src], st->nx, st->ny, st->p_pad, with_halo(st), s);
  }
  const bool split = w_simplex_split(st) && nblk_h(st) > 0;
  if (!split && (!w_update_is_local(st) || st->no_fused == 1)) {   // W' needs a global finish (G given, simplex over W): the four steps
    if (int rc = espm_mu_w_reduce_pack(st, src, slot, x->staging, s)) return rc;
    if (int rc = espm_xchg_post(x, seq, s)) return rc;
    if (int rc = espm_xchg_wait(x, seq, s)) return rc;
    return shard_combine_finish(st, espm_xchg_records(x, (int)(seq & 1u)), x->world, src, slot, tail_out, s);
  }
  // One launch when W' is local.  The simplex over W with G = identity (the estimator's default constraints): the pieces of A cross
  // the links as granules like the local update's, the workgroup that sums 32 entries leaves the bracket's partials,
  // w_simplex_update_kernel follows and owns the tail - two launches
  if (split)
    if (int rc = simplex_w_feasible(st, st->n)) return rc;
  if (int rc = launch_w_exchange_update(f, st->a_slab, slab_bytes, st->nblk_w, st->a, st->hstat[1 - src], fin, x, seq, st->h[1 - src], st->nx, st->ny,
                                        st->p_pad, with_halo(st), s, split ? nullptr : tail_out, split ? simplex_bparts(st) : nullptr))
    return rc;
  return split ? simplex_update(st, src, slot, tail_out, s) : ESPM_OK;
}

int espm_mu_shard_exchange_finish(const espm_mu_state* st, espm_xchg* x, uint32_t seq, int src, int slot, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(x && (src == 0 || src == 1), "shard_exchange_finish: bad arguments");
  if (int rc = check_slot(st, slot, true)) return rc;
  if (int rc = check_record_bytes("shard_exchange_finish", st, x)) return rc;
  WTailArgs left_out;
  return shard_exchange_finish(st, x, seq, src, slot, left_out_of(st, &left_out), static_cast<hipStream_t>(stream));
}

// (st->tail_mode is read once: ESPM_TAIL_RIDE hands over a deferred tail of the caller's own last update.  Never written.)
int espm_mu_iterate_sharded(espm_mu_state* st, espm_xchg* x, uint32_t* seq, int n_iter, int final_loss, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(x && seq && n_iter >= 0, "iterate_sharded: bad arguments");
  if (int rc = check_room(st, n_iter)) return rc;
  if (int rc = check_record_bytes("iterate_sharded", st, x)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool hand_on = loop_hands_tail_on(st), fused = fused_ok(st);
  // byte offsets inside a record: [A | statistics | first owned image row | last owned image row]
  const size_t off_top = (size_t)st->k * st->n_pad * 4 + ESPM_HS_STRIDE * 8, off_bot = off_top + (size_t)st->k * (st->ny > 0 ? st->ny : 0) * 4;
  Ride r;
  int rc = ride_of_tail_mode(st, st->cur, &r);
  for (int i = 0; i < n_iter && !rc; ++i) {
    const int cur = st->cur, slot = st->it;
    rc = h_half(st, cur, 1, r.on, fused, s);
    if (!rc && !fused) rc = w_accum(st, s);
    const uint32_t q = ++*seq;
    const unsigned char* recs = static_cast<const unsigned char*>(espm_xchg_records(x, (int)(q & 1u)));
    // slab reduction, exchange of the records and W update: one launch when W' needs nothing but the global row sums
    if (!rc) rc = shard_exchange_finish(st, x, q, cur, slot, hand_on ? &r.tail : nullptr, s);
    r.on = hand_on ? &r.tail : nullptr;
    if (with_halo(st)) {   // the row above this block is the LAST owned row of rank - 1, the row below the FIRST of rank + 1
      st->halo_top = x->rank > 0 ? reinterpret_cast<const float*>(recs + (size_t)(x->rank - 1) * x->record_bytes + off_bot) : nullptr;
      st->halo_bot = x->rank < x->world - 1 ? reinterpret_cast<const float*>(recs + (size_t)(x->rank + 1) * x->record_bytes + off_top) : nullptr;
    }
    st->cur = 1 - cur;
    st->it = slot + 1;
  }
  if (!rc && r.on) rc = launch_w_update_tail(r.tail, s);
  if (rc || !final_loss) return rc;
  return loss_only(st, st->cur, st->it, nullptr, s);
}

int espm_dichotomy_simplex(const double* num, const double* den, int k, int p, int den_cols, double log_shift,
                           double tol, int maxit, double* nu_out, int32_t* status_out, espm_stream_t stream) {
  ESPM_REQUIRE(num && den && nu_out && status_out, "dichotomy: NULL pointer");
  ESPM_REQUIRE(k >= 1 && p >= 1 && (den_cols == 1 || den_cols == p), "dichotomy: bad shape k=%d p=%d den_cols=%d", k,
               p, den_cols);
  if (log_shift > 0 && (double)k * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  return launch_dichotomy(num, den, k, p, den_cols, log_shift, tol, maxit, nu_out, status_out,
                          static_cast<hipStream_t>(stream));
}

int espm_simplex_root_f32(const float* num, const float* den, int k, int p, float log_shift, float tol, int maxit, int fast_exit,
                          float* delta_out, float* e_out, int32_t* status_out, espm_stream_t stream) {
  ESPM_REQUIRE(num && den && delta_out && e_out && status_out, "simplex_root_f32: NULL pointer");
  ESPM_REQUIRE(k >= ESPM_MIN_K && k <= ESPM_MAX_K && p >= 1, "simplex_root_f32: bad shape k=%d p=%d (this library: %d..%d components)", k, p, ESPM_MIN_K, ESPM_MAX_K);
  if (log_shift > 0 && (double)k * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  return launch_simplex_root_f32(num, den, k, p, log_shift, tol, maxit, fast_exit, delta_out, e_out, status_out, static_cast<hipStream_t>(stream));
}

int espm_surrogate_terms(const float* h_old, const float* h_new, int k, int p, int64_t ld, int nx, int ny, int grid_mode, double* part,
                         int part_doubles, double* out, espm_stream_t stream) {
  ESPM_REQUIRE(h_old && h_new && part && out && k >= 1 && k <= ESPM_KP && p >= 1 && ld >= p, "surrogate_terms: bad arguments");
  ESPM_REQUIRE(!grid_mode || (nx >= 1 && ny >= 1 && (int64_t)nx * ny == p), "surrogate_terms: grid %d x %d does not match p=%d", nx, ny, p);
  ESPM_REQUIRE(part_doubles >= (4 + ESPM_KP) * ((p + 511) / 512), "surrogate_terms: scratch of %d doubles is too small", part_doubles);
  return launch_linesearch_terms(h_old, h_new, k, p, (int)ld, nx, ny, grid_mode, nullptr, nullptr, nullptr, nullptr, part, out,
                                 static_cast<hipStream_t>(stream));
}

int espm_dichotomy_simplex_acc(double a, const double* b, const double* minus_c, int k, int p, int b_cols, double log_shift,
                               double tol, int maxit, double* nu_out, int32_t* status_out, espm_stream_t stream) {
  ESPM_REQUIRE(b && minus_c && nu_out && status_out, "dichotomy_acc: NULL pointer");
  ESPM_REQUIRE(k >= 1 && p >= 1 && (b_cols == 1 || b_cols == p) && a >= 0, "dichotomy_acc: bad arguments k=%d p=%d b_cols=%d", k, p, b_cols);
  if (log_shift > 0 && (double)k * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  return launch_dichotomy_acc(a, b, minus_c, k, p, b_cols, log_shift, tol, maxit, nu_out, status_out, static_cast<hipStream_t>(stream));
}

int espm_dichotomy_simplex_pg(const double* a, int k, int p, double log_shift, double tol, int maxit, double* nu_out,
                              espm_stream_t stream) {
  ESPM_REQUIRE(a && nu_out && k >= 1 && p >= 1, "dichotomy_pg: bad arguments");
  if (log_shift > 0 && (double)k * log_shift >= 1.0) return set_error(ESPM_ENOSOLUTION, "No solution exists!");
  return launch_dichotomy_pg(a, k, p, log_shift, tol, maxit, nu_out, static_cast<hipStream_t>(stream));
}

int espm_mu_laplacian(const float* h, int k, int nx, int ny, int64_t ld, float* out, espm_stream_t stream) {
  ESPM_REQUIRE(h && out && k >= 1 && nx >= 1 && ny >= 1 && ld >= (int64_t)nx * ny, "laplacian: bad arguments");
  return launch_laplacian(h, k, nx, ny, ld, out, static_cast<hipStream_t>(stream));
}


// ---- Frobenius ("l2") branch of the step functions (mu_l2.hip) ----------------------------------------------------
static int check_l2(const espm_mu_state* st, const float* work, const double* scratch, int scratch_doubles) {
  ESPM_REQUIRE(work && scratch && scratch_doubles >= ESPM_KP * ESPM_KP, "l2 step: work (2, KP, KP) and a scratch of >= %d doubles are needed", ESPM_KP * ESPM_KP);
  ESPM_REQUIRE(st->x_dtype == ESPM_X_F32, "l2 step: the f32 store is required");
  ESPM_REQUIRE(st->xscale == 1.f, "l2 step: xscale = 1 is required");
  return ESPM_OK;
}

int espm_mu_l2_step_h(const espm_mu_state* st, int src, float* work, double* scratch, int scratch_doubles, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  if (int rc = check_l2(st, work, scratch, scratch_doubles)) return rc;
  ESPM_REQUIRE(src == 0 || src == 1, "src must be 0/1");
  ESPM_REQUIRE(st->lambda_l == 0.f && st->mu == nullptr, "l2 H step: lambda_L = 0 and mu = 0 are required (updates.py:110-114)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = launch_gram(st->gw_s, st->n, st->k, scratch, scratch_doubles, work, s)) return rc;   // GW^T GW
  HStepArgs a = make_h_args(st, src, 1);
  a.compute_loss = 0;
  a.l2_m = work;
  return dispatch_h_step(a, st->x_dtype, st->tile_px, nblk_h(st), s);
}

int espm_mu_l2_w_partials(const espm_mu_state* st, float* work, double* scratch, int scratch_doubles, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  if (int rc = check_l2(st, work, scratch, scratch_doubles)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* hh = work + ESPM_KP * ESPM_KP;
  if (int rc = launch_gram(st->h_t, st->p, st->k, scratch, scratch_doubles, hh, s)) return rc;      // H H^T
  WAccumArgs wa = make_w_args(st);
  wa.l2 = 1;
  if (int rc = dispatch_w_accum(wa, st->k, st->x_dtype, st->nblk_w, s)) return rc;                 // slabs of X H^T
  return launch_w_reduce(st->a_slab, st->a, st->nblk_w, st->k * st->n_pad, nullptr, s);
}

int espm_mu_l2_w_finish(const espm_mu_state* st, int src, const float* gtg, const float* work, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(work && (src == 0 || src == 1), "l2 W finish: bad arguments");
  ESPM_REQUIRE(st->m == 0 || gtg, "l2 W step: G^T G (m, m) is needed when G is given");
  ESPM_REQUIRE(!st->simplex_w, "l2 W step: no simplex over W in the Frobenius branch (updates.py:31-36)");
  return launch_w_finish_l2(st->a, st->n, st->n_pad, st->m, st->k, st->m > 0 ? st->g : nullptr, gtg, work + ESPM_KP * ESPM_KP, st->w[src],
                            st->w[1 - src], st->fixed_w, st->log_shift, static_cast<hipStream_t>(stream));
}

int espm_mu_l2_step_w(const espm_mu_state* st, int src, const float* gtg, float* work, double* scratch, int scratch_doubles,
                      espm_stream_t stream) {
  if (int rc = espm_mu_l2_w_partials(st, work, scratch, scratch_doubles, stream)) return rc;
  return espm_mu_l2_w_finish(st, src, gtg, work, stream);
}

int espm_mu_linesearch_terms(const espm_mu_state* st, int hold, int hnew, double* out, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(out && (hold == 0 || hold == 1) && hnew == 1 - hold, "linesearch_terms: bad arguments");
  ESPM_REQUIRE(!st->halo_top && !st->halo_bot && (st->p_total == 0 || st->p_total == st->p), "linesearch_terms: not built for a sharded image");
  // the H-step's record buffer is free between espm_mu_h_finalize and the next espm_mu_step_h: ESPM_HP_STRIDE rows of
  // ceil(p / tile_px) >= ceil(p / 512) doubles hold the 3 + KP rows of partials
  return launch_linesearch_terms(st->h[hold], st->h[hnew], st->k, st->p, st->p_pad, st->nx, st->ny, st->grid_mode, nullptr, nullptr,
                                 nullptr, nullptr, st->hpart, out, static_cast<hipStream_t>(stream));
}

int espm_mu_linesearch_terms_sharded(const espm_mu_state* st, int hold, int hnew, const float* old_halo_top, const float* old_halo_bot,
                                     double* out, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(out && (hold == 0 || hold == 1) && hnew == 1 - hold, "linesearch_terms_sharded: bad arguments");
  // the boundary rows travel in the records only when the Laplacian term is on (espm_mu_shard_record_bytes)
  ESPM_REQUIRE(!st->grid_mode || st->lambda_l != 0.f, "linesearch_terms_sharded: lambda_L = 0 leaves the boundary rows out of the records");
  ESPM_REQUIRE((old_halo_top == nullptr) == (st->halo_top == nullptr) && (old_halo_bot == nullptr) == (st->halo_bot == nullptr),
               "linesearch_terms_sharded: the old H's boundary rows must be given where the new H has them");
  return launch_linesearch_terms(st->h[hold], st->h[hnew], st->k, st->p, st->p_pad, st->nx, st->ny, st->grid_mode, old_halo_top,
                                 old_halo_bot, st->halo_top, st->halo_bot, st->hpart, out, static_cast<hipStream_t>(stream));
}

size_t espm_mu_shard_record_bytes(const espm_mu_state* st) {
  if (check_abi(st)) return 0;
  size_t b = (size_t)st->k * st->n_pad * 4 + ESPM_HS_STRIDE * 8 + 2 * (size_t)st->k * (st->ny > 0 ? st->ny : 0) * 4;
  return (b + 15) / 16 * 16;
}

int espm_mu_shard_pack(const espm_mu_state* st, int hnew, void* record, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(record && (hnew == 0 || hnew == 1), "shard_pack: bad arguments");
  return launch_shard_pack(st->a, st->hstat[hnew], st->h[hnew], st->k, st->n_pad, st->nx, st->ny, st->p_pad,
                           with_halo(st), record, static_cast<hipStream_t>(stream));
}

int espm_mu_w_reduce_pack(const espm_mu_state* st, int src, int slot, void* record, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(record && (src == 0 || src == 1), "w_reduce_pack: bad arguments");
  if (int rc = check_slot(st, slot, false)) return rc;
  HFinalizeArgs fin = finalize_args(st, src, slot, true);
  fin.hstat_out = reinterpret_cast<double*>(static_cast<unsigned char*>(record) + (size_t)st->k * st->n_pad * 4);
  return launch_w_reduce_pack(st->a_slab, st->nblk_w, st->k, st->n_pad, fin, st->h[1 - src], st->nx, st->ny, st->p_pad, with_halo(st),
                              record, static_cast<hipStream_t>(stream));
}

int espm_mu_shard_combine(const espm_mu_state* st, const void* records, int world, int hnew, espm_stream_t stream) {
  if (int rc = check_state(st)) return rc;
  ESPM_REQUIRE(records && world >= 1 && (hnew == 0 || hnew == 1), "shard_combine: bad arguments");
  return launch_shard_combine(records, world, espm_mu_shard_record_bytes(st), st->k * st->n_pad, st->a,
                              st->hstat[hnew], static_cast<hipStream_t>(stream));
}

}  // extern "C"
