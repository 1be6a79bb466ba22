// The sparse store's launchers on the CPU: csrc/mu_ell.hip, mu_h_chain.hip and mu_fused.hip compiled for the host alone and linked
// against the stubs below - the HIP runtime's launch, attribute and registration calls, check_hip / set_error and the two lean fused
// launchers - run anywhere.  A launch leaves one record: the kernel (the name the unit registered for the launched host pointer),
// grid, block, dynamic LDS, the LDS granted through hipFuncSetAttribute, every field of the argument block that the launcher lays
// out, the return code and the error text.  tests/test_ell_plan_cpu.py drives it:
//   driver sweep             the n_pad at which anything discrete of a record changes, per (k, pb) and (k, tile_px): the grid file
//   driver trace GRID        the records over the grid, per (launch, k, pb) as a line count and an FNV-1a hash
//   driver trace GRID --full the same written out
//   driver predicates        fused_ell_lds_bytes, its comparison with ESPM_ELL_LDS_MAX and ell_chain_fits for n = 1 .. 16384
//   driver shapes            every distinct shape of the fused launch's plan, at the smallest (k, n_pad) that reaches it
//   driver shape K N_PAD PB STREAM  the fused and the chained record of one case as the engine launches it (tests/ell_plan_cases.py)
// ESPM_FUSED_PLAIN and ESPM_FUSED_SMALL_SEGS are read once per process: the test runs the program once per pair of values.
#include <cxxabi.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "mu_fused_kernel.hpp"

namespace espm {
int launch_h_ell(const HStepArgs& args, int nblk, hipStream_t stream);
int launch_h_chain(const HStepArgs& args, int x_dtype, int tile_px, int nblk, hipStream_t stream);
int launch_fused_ell(const HStepArgs& h, const WAccumArgs& w, int nblk, hipStream_t stream, int static_units, int stream_lists);
bool h_chain_built(const espm_mu_state* st);
}  // namespace espm

// ---- what a launch leaves -------------------------------------------------------------------------------------------------------------
struct Record {
  std::string kernel = "-";
  int grid = 0, block = 0, grant = 0;
  size_t lds = 0;
  std::string args = "-";
};
static Record g_rec;
static char g_err[512];

static std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}
static std::map<const void*, std::string>& kernels() {   // (filled by the units' static initialisers: constructed on first use)
  static std::map<const void*, std::string> m;
  return m;
}
static std::string h_fields(const espm::HStepArgs& h) { return fmt("cs=%d tail=%d chain=%d", h.cs_lds_off, h.tail_on, h.chain_lds_off); }
static std::string fused_fields(const espm::FusedArgs& a) {
  return fmt("segs=%d cnt=%d meta=%d perm=%d red=%d perm_lds=%d slab=%d w_split=%d static=%d stream=%d keep=%d,%d ", a.h_segs, a.cnt_lds_off,
             a.meta_lds_off, a.perm_lds_off, a.red_lds_off, a.perm_lds, a.slab_lds, a.w_split, a.static_units, a.stream_lists, a.keep_h, a.keep_w) +
         h_fields(a.h);
}

// ---- the stubs --------------------------------------------------------------------------------------------------------------------------
extern "C" {
// (no device image: the units are compiled with -fuse-cuid=none, so that their registrations all hand on this one symbol; nothing reads it)
char __hip_fatbin[16] = {0};
void** __hipRegisterFatBinary(const void*) {
  static void* handle = nullptr;
  return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*, int*) {
  int status = 0;
  char* d = abi::__cxa_demangle(name, nullptr, nullptr, &status);
  kernels()[host] = d ? d : name;
  free(d);
}
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
  g_grid = grid, g_block = block, g_shmem = shmem, g_stream = stream;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
  *grid = g_grid, *block = g_block, *shmem = g_shmem, *stream = g_stream;
  return hipSuccess;
}
hipError_t hipLaunchKernel(const void* host, dim3 grid, dim3 block, void** args, size_t shmem, hipStream_t) {
  auto it = kernels().find(host);
  g_rec.kernel = it == kernels().end() ? "unregistered" : it->second;
  g_rec.grid = (int)grid.x, g_rec.block = (int)block.x, g_rec.lds = shmem;
  if (grid.y != 1 || grid.z != 1 || block.y != 1 || block.z != 1) g_rec.kernel += " (not 1-D)";
  if (g_rec.kernel.find("mu_fused_ell_kernel") != std::string::npos) g_rec.args = fused_fields(*static_cast<const espm::FusedArgs*>(args[0]));
  else if (g_rec.kernel.find("h_step_ell_kernel") != std::string::npos) g_rec.args = h_fields(*static_cast<const espm::HStepArgs*>(args[0]));
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute attr, int value) {
  g_rec.grant = attr == hipFuncAttributeMaxDynamicSharedMemorySize ? value : -1;
  return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int* d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
  prop->multiProcessorCount = 256;
  return hipSuccess;
}
}  // extern "C"

namespace espm {
int set_error(int code, const char* f, ...) {
  va_list ap;
  va_start(ap, f);
  vsnprintf(g_err, sizeof(g_err), f, ap);
  va_end(ap);
  return code;
}
int check_hip(hipError_t e, const char* what) { return e == hipSuccess ? ESPM_OK : set_error(ESPM_EHIP, "%s: stubbed HIP runtime", what); }
static int plain_stub(const char* name, const FusedArgs& args, int k, bool loss, bool full, int nblk, size_t lds_bytes) {
  g_rec.kernel = fmt("%s(k=%d,loss=%d,full=%d)", name, k, (int)loss, (int)full);
  g_rec.grid = nblk, g_rec.lds = lds_bytes, g_rec.args = fused_fields(args);
  return ESPM_OK;
}
int launch_fused_plain(const FusedArgs& args, int k, bool loss, bool full, int nblk, size_t lds_bytes, hipStream_t) {
  return plain_stub("launch_fused_plain", args, k, loss, full, nblk, lds_bytes);
}
int launch_fused_plain_stream(const FusedArgs& args, int k, bool loss, bool full, int nblk, size_t lds_bytes, hipStream_t) {
  return plain_stub("launch_fused_plain_stream", args, k, loss, full, nblk, lds_bytes);
}
}  // namespace espm

// ---- the cases --------------------------------------------------------------------------------------------------------------------------
static void* const GIVEN = reinterpret_cast<void*>(0x1000);   // a pointer that is set; nothing dereferences it
static const int NBLK = 3;

struct Opt {
  int cs_parts = 0, tail = 0 /* 0: none, 1: rides, 2: rides with the projected gradient's term */, loss = 0, stream = 0;
  int h_rule = 0, chain_fin = 0;
  const char* flip = "";   // one fact of the fused launch's common case turned the other way
};
static std::string opt_name(const Opt& o) {
  return fmt("cs_parts=%d tail=%d loss=%d stream=%d h_rule=%d chain_fin=%d%s%s", o.cs_parts, o.tail, o.loss, o.stream, o.h_rule, o.chain_fin, *o.flip ? " flip=" : "", o.flip);
}

static espm::HStepArgs h_args(int k, int n_pad, int tile_px, const Opt& o) {
  espm::HStepArgs h;
  memset(&h, 0, sizeof(h));
  h.ell = (const uint32_t*)GIVEN, h.ell_off = (const int32_t*)GIVEN, h.ell_klc = (const float*)GIVEN, h.ell_pix = (const int32_t*)GIVEN;
  h.ell_blk_cnt = (const float*)GIVEN;
  h.n = h.n_pad = n_pad, h.k = k, h.p = 2 * NBLK * tile_px, h.p_pad = h.p, h.ell_bits = 14, h.ell_tp = tile_px;
  h.simplex_h = h.grid_mode = h.write_h = h.have_prev = 1, h.lambda_l = 1.f, h.compute_loss = o.loss, h.h_rule = o.h_rule;
  h.cs_lds_off = h.chain_lds_off = -7;   // (a launcher that leaves them alone shows it)
  if (o.cs_parts) h.cs_parts = (const double*)GIVEN, h.cs_nbk = (n_pad + 31) / 32;
  if (o.tail) h.tail_on = 1, h.tail.pg_q = o.tail == 2 ? (double*)GIVEN : nullptr;
  h.chain_fin_on = o.chain_fin;
  return h;
}

static std::string finish(int rc) {
  std::string s = fmt("%s grid=%d block=%d lds=%zu grant=%d | %s | rc=%d", g_rec.kernel.c_str(), g_rec.grid, g_rec.block, g_rec.lds, g_rec.grant,
                      g_rec.args.c_str(), rc);
  return rc ? s + " error: " + g_err : s;
}
static std::string run_fused(int k, int n_pad, int pb, const Opt& o) {
  g_rec = Record();
  espm::HStepArgs h = h_args(k, n_pad, pb / 2, o);
  espm::WAccumArgs w;
  memset(&w, 0, sizeof(w));
  w.ell = (const uint32_t*)GIVEN, w.ell_off = (const int32_t*)GIVEN, w.chan_perm = (const int32_t*)GIVEN;
  w.n_pad = n_pad, w.p = h.p, w.n_cg = (n_pad + 63) / 64, w.pb = pb, w.pbits = espm::ell_pbits(pb);
  int static_units = 0;
  const std::string f = o.flip;
  if (f == "fixed_h") h.fixed_h = (const float*)GIVEN;
  if (f == "fill_num") h.fill_num = (const float*)GIVEN, h.fill_n = 5;
  if (f == "breg_sr") h.breg_sr = (const float*)GIVEN;
  if (f == "simplex_h") h.simplex_h = 0;
  if (f == "lambda_l") h.lambda_l = 0.f;
  if (f == "grid_mode") h.grid_mode = 0;
  if (f == "have_prev") h.have_prev = 0;
  if (f == "static_units") static_units = 1;
  if (f == "cs_nbk") h.cs_nbk = 65;
  if (f == "ell_blk_cnt") h.ell_blk_cnt = nullptr;
  if (f == "n_cg") w.n_cg = 1;
  return finish(espm::launch_fused_ell(h, w, NBLK, nullptr, static_units, o.stream ? 1 | 3 << 8 | 5 << 16 : 0));
}
static std::string run_h(int k, int n_pad, int tile_px, const Opt& o, bool chained) {
  g_rec = Record();
  const espm::HStepArgs h = h_args(k, n_pad, tile_px, o);
  return finish(chained ? espm::launch_h_chain(h, ESPM_X_ELL, tile_px, 2 * NBLK, nullptr) : espm::launch_h_ell(h, 2 * NBLK, nullptr));
}

static std::vector<Opt> fused_opts(bool flips) {
  std::vector<Opt> v;
  for (int cs = 0; cs < 2; ++cs)
    for (int tail = 0; tail < 3; ++tail)
      for (int loss = 0; loss < 2; ++loss)
        for (int stream = 0; stream < 2; ++stream) {
          Opt o;
          o.cs_parts = cs, o.tail = tail, o.loss = loss, o.stream = stream;
          v.push_back(o);
        }
  if (flips)
    for (const char* f : {"fixed_h", "fill_num", "breg_sr", "simplex_h", "lambda_l", "grid_mode", "have_prev", "static_units", "cs_nbk", "ell_blk_cnt", "n_cg"}) {
      Opt o;
      o.cs_parts = o.tail = o.loss = 1, o.flip = f;
      v.push_back(o);
    }
  return v;
}
static std::vector<Opt> h_opts() {
  std::vector<Opt> v;
  for (int cs = 0; cs < 2; ++cs)
    for (int tail = 0; tail < 2; ++tail)
      for (int loss = 0; loss < 2; ++loss)
        for (int rule = 0; rule < 3; ++rule) {
          Opt o;
          o.cs_parts = cs, o.tail = tail, o.loss = loss, o.h_rule = rule;
          v.push_back(o);
        }
  return v;
}
static std::vector<Opt> chain_opts() {
  std::vector<Opt> v(2);
  v[0].loss = v[1].loss = 1, v[1].chain_fin = 1;
  return v;
}

// what of a record is discrete: everything but the numbers that grow with every n_pad (the offsets and sizes), which are kept as
// their side of what they are compared with
static std::string discrete(const std::string& rec) {
  std::string out;
  for (size_t i = 0; i < rec.size();) {
    if (isdigit((unsigned char)rec[i]) && i > 0 && (rec[i - 1] == '=' || rec[i - 1] == ' ')) {
      size_t j = i;
      while (j < rec.size() && isdigit((unsigned char)rec[j])) ++j;
      const long v = atol(rec.substr(i, j - i).c_str());
      out += v == 0 ? "0" : v <= 16 ? rec.substr(i, j - i) : v <= 64 * 1024 ? "s" : v <= ESPM_ELL_LDS_MAX ? "m" : "L";
      i = j;
    } else {
      out += rec[i++];
    }
  }
  return out;
}

static const int PBS[4] = {128, 256, 512, 1024};
enum Launch { FUSED, HSTEP, CHAIN };
static const char* const LAUNCH_NAME[3] = {"fused", "h_step", "h_chain"};
static std::vector<Opt> opts_of(int launch, bool flips) { return launch == FUSED ? fused_opts(flips) : launch == HSTEP ? h_opts() : chain_opts(); }
static std::string run_one(int launch, int k, int n_pad, int pb, const Opt& o) {
  return launch == FUSED ? run_fused(k, n_pad, pb, o) : run_h(k, n_pad, pb / 2, o, launch == CHAIN);
}
// where the red scratch of a fused record lies relative to the counters: in the table (below them) or behind
static std::string red_side(const std::string& rec) {
  const size_t c = rec.find(" cnt="), r = rec.find(" red=");
  if (c == std::string::npos || r == std::string::npos) return "";
  const long cnt = atol(rec.c_str() + c + 5), red = atol(rec.c_str() + r + 5);
  return red < 0 ? " red:none" : red < cnt ? " red:table" : " red:behind";
}

// ---- the shape of a fused launch's plan (tests/ell_plan_cases.py): what is where, without the sizes ------------------------------------
template <int K>
static void geom_k(int rows, size_t* table, int* floor_full) {
  *table = espm::FixTab<K>::bytes(rows), *floor_full = espm::FusedGeom<K>::S;
}
static long field(const std::string& rec, const char* name) {
  const size_t at = rec.find(name);
  return at == std::string::npos ? -1 : atol(rec.c_str() + at + strlen(name));
}
static std::string shape_key(int k, int n_pad, int pb, const std::string& rec) {
  if (rec.find("rc=0") == std::string::npos) return "refused";
  size_t table = 0;
  int floor_full = 0;
  switch (k) {
#define ESPM_X(KK) case KK: geom_k<KK>(n_pad > pb ? n_pad : pb, &table, &floor_full); break;
    ESPM_K_CASES(ESPM_X)
#undef ESPM_X
  }
  const bool full = pb == ESPM_ELL_PB;
  const long segs = field(rec, "segs="), region = field(rec, " cnt=") - (long)table, slab = (long)4 * k * n_pad;
  const bool grown = field(rec, " slab=") == 1 && region == slab && region > segs * k * pb * 4;
  const std::string instance = rec.find("launch_fused_plain_stream") == 0 ? "plain-stream" : rec.find("launch_fused_plain") == 0 ? "plain" : "generic";
  return fmt("%s perm_lds=%ld%s slab:%s cs:%s segs:%s %s", full ? "full" : "small", field(rec, " perm_lds="), red_side(rec).c_str(),
             grown ? "grown" : field(rec, " slab=") == 1 ? "lds" : "none", field(rec, " cs=") > 0 ? "behind" : field(rec, " cs=") == 0 ? "late" : "none",
             segs > (full ? floor_full : ESPM_ELL_PB / pb) ? "above" : "floor", instance.c_str());
}
static Opt engine_opt(int stream) {   // as espm_mu_iterate launches it from the second iteration on: the W update's tail rides, with the loss
  Opt o;
  o.cs_parts = o.tail = o.loss = 1, o.stream = stream;
  return o;
}
// every shape the fused launch reaches over k, n_pad = 8 .. 16384 and pb where fused_ell_lds_bytes admits it (mu_api.hip: fused_ok), each
// at the smallest (k, n_pad) that reaches it; a launch refused there would show as a shape "refused"
static void shapes() {
  std::set<std::string> seen;
  for (int k = ESPM_MIN_K; k <= ESPM_MAX_K; ++k)
    for (int n_pad = 8; n_pad <= 16384; n_pad += 8)
      for (int pb : PBS) {
        if (espm::fused_ell_lds_bytes(n_pad, k, pb) > ESPM_ELL_LDS_MAX) continue;
        for (int stream = 0; stream < 2; ++stream) {   // (espm_mu_state.ell_stream: the lists read past the last-level cache)
          const std::string key = shape_key(k, n_pad, pb, run_fused(k, n_pad, pb, engine_opt(stream)));
          if (seen.insert(key).second) printf("k=%d n_pad=%d pb=%d stream=%d: %s\n", k, n_pad, pb, stream, key.c_str());
        }
      }
}

static void sweep() {
  for (int launch = 0; launch < 3; ++launch)
    for (int k = ESPM_MIN_K; k <= ESPM_MAX_K; ++k)
      for (int pb : PBS) {
        std::set<int> at = {8, 1000};
        const std::vector<Opt> opts = opts_of(launch, false);
        std::vector<std::string> prev(opts.size());
        for (int n_pad = 8; n_pad <= 16384; n_pad += 8)
          for (size_t i = 0; i < opts.size(); ++i) {
            const std::string rec = run_one(launch, k, n_pad, pb, opts[i]);
            const std::string d = discrete(rec) + red_side(rec);
            if (n_pad > 8 && d != prev[i]) at.insert(n_pad - 8), at.insert(n_pad);
            prev[i] = d;
          }
        printf("%s %d %d :", LAUNCH_NAME[launch], k, pb);
        for (int n : at) printf(" %d", n);
        printf("\n");
      }
}

static uint32_t fnv(uint32_t h, const std::string& s) {
  for (unsigned char c : s) h = (h ^ c) * 16777619u;
  return (h ^ '\n') * 16777619u;
}

static int trace(const char* grid_path, bool full) {
  FILE* f = fopen(grid_path, "r");
  if (!f) return fprintf(stderr, "cannot read %s\n", grid_path), 2;
  char buf[8192];
  const char* plain = getenv("ESPM_FUSED_PLAIN");
  const char* segs = getenv("ESPM_FUSED_SMALL_SEGS");
  const std::string knobs = fmt("ESPM_FUSED_PLAIN=%s ESPM_FUSED_SMALL_SEGS=%s", plain ? plain : "unset", segs ? segs : "unset");
  while (fgets(buf, sizeof(buf), f)) {
    char name[32];
    int k, pb, used = 0;
    if (sscanf(buf, "%31s %d %d :%n", name, &k, &pb, &used) != 3 || k < ESPM_MIN_K || k > ESPM_MAX_K) continue;
    int launch = 0;
    while (launch < 3 && strcmp(name, LAUNCH_NAME[launch])) ++launch;
    if (launch == 3) continue;
    std::vector<std::string> lines;
    const char* p = buf + used;
    int n_pad, adv;
    while (sscanf(p, "%d%n", &n_pad, &adv) == 1) {
      p += adv;
      for (const Opt& o : opts_of(launch, n_pad == 1000))
        lines.push_back(fmt("%s k=%d %s=%d n_pad=%d %s: ", name, k, launch == FUSED ? "pb" : "tile_px", launch == FUSED ? pb : pb / 2, n_pad, opt_name(o).c_str()) +
                        run_one(launch, k, n_pad, pb, o));
    }
    uint32_t h = 2166136261u;
    for (const std::string& l : lines) h = fnv(h, l);
    printf("%s k=%d %s=%d [%s] lines=%zu fnv1a=%08x\n", name, k, launch == FUSED ? "pb" : "tile_px", launch == FUSED ? pb : pb / 2,
           launch == FUSED ? knobs.c_str() : "-", lines.size(), h);
    if (full)
      for (const std::string& l : lines) printf("  %s\n", l.c_str());
  }
  fclose(f);
  return 0;
}

static bool chain_fits(int k, int n_pad, int tile_px) {
  espm_mu_state st;
  memset(&st, 0, sizeof(st));
  st.k = k, st.n_pad = n_pad, st.tile_px = tile_px, st.compute_loss = 1, st.x_dtype = ESPM_X_ELL;
  return espm::h_chain_built(&st);
}
static void predicates() {
  long compared = 0;
  for (int k = ESPM_MIN_K; k <= ESPM_MAX_K; ++k)
    for (int pb : PBS) {
      uint32_t hb = 2166136261u, hc = 2166136261u;
      int fused_n = 0, chain_n = 0;
      std::string slack;   // n_pad the 8 bytes of slack in fused_ell_lds_bytes (mu_ell_plan.hpp: FUSED_FLOOR_SLACK) keep off the fused launch
      for (int n = 1; n <= 16384; ++n, ++compared) {
        const int n_pad = (n + 7) / 8 * 8;
        const size_t b = espm::fused_ell_lds_bytes(n_pad, k, pb);
        const bool fits = b <= ESPM_ELL_LDS_MAX, cf = chain_fits(k, n_pad, pb / 2);
        hb = fnv(hb, fmt("%zu %d", b, (int)fits)), hc = fnv(hc, cf ? "1" : "0");
        fused_n += fits, chain_n += cf;
        if (!fits && b != (size_t)-1 && b - 8 <= ESPM_ELL_LDS_MAX && n == n_pad) slack += fmt(" %d", n_pad);
      }
      printf("predicates k=%d pb=%d tile_px=%d: fused_ell_lds_bytes fits for %d n, fnv1a=%08x; ell_chain_fits for %d n, fnv1a=%08x\n", k, pb, pb / 2,
             fused_n, hb, chain_n, hc);
      if (!slack.empty()) printf("predicates k=%d pb=%d: the layout at the floor fits exactly and fused_ell_lds_bytes says no at n_pad =%s\n", k, pb, slack.c_str());
    }
  printf("predicates compared: %ld inputs each\n", compared);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sweep") return sweep(), 0;
  if (mode == "trace" && argc > 2) return trace(argv[2], argc > 3 && !strcmp(argv[3], "--full"));
  if (mode == "predicates") return predicates(), 0;
  if (mode == "shapes") return shapes(), 0;
  if (mode == "shape" && argc == 6) {
    const int k = atoi(argv[2]), n_pad = atoi(argv[3]), pb = atoi(argv[4]);
    const std::string rec = run_fused(k, n_pad, pb, engine_opt(atoi(argv[5])));
    printf("%s\n", rec.c_str());
    Opt c;
    c.loss = c.chain_fin = 1;
    printf("%s\n", run_h(k, n_pad, pb / 2, c, true).c_str());
    printf("fused_ell_lds_bytes=%zu\n", espm::fused_ell_lds_bytes(n_pad, k, pb));
    printf("shape: %s\n", shape_key(k, n_pad, pb, rec).c_str());
    return 0;
  }
  fprintf(stderr, "usage: driver sweep | trace GRID [--full] | predicates | shapes | shape K N_PAD PB STREAM\n");
  return 2;
}
