// The second launch of an iteration with G = identity (the W step as a whole: mu_w_parts.hpp): the slab reduction alone, with the
// update of W folded in, the update under the simplex over W, and the tail that forms what is global.
#include "mu_w_parts.hpp"

namespace espm {

// Slab reduction A = sum_b A_b in ONE pass and in a fixed order (bit-reproducible; no float atomics):
// a workgroup owns 32 consecutive entries of A; its 256 threads are 32 entries x 8 slab groups, group g
// sums the slabs b = g, g + 8, ... with 8 independent partial sums (loads in flight), then the 8 groups are
// combined through LDS in group order.  One extra workgroup (when `fin` is set) reduces the H-step's
// per-workgroup records at the same time (h_finalize_body), which saves a dependent launch per iteration.
struct WReduceArgs {
  const float* slab;
  float* out;
  int nblk, total, nred_blocks, fuse_finalize;
  HFinalizeArgs fin;
  // sharded image: `out` is the A block of this rank's record and the extra workgroup also copies the first and
  // the last owned image row of the new H behind the statistics (shard_pack_kernel's job, without its launch)
  const float* halo_h;
  float* halo_top;
  float* halo_bot;
  int halo_k, halo_nx, halo_ny, halo_ppad;
  // simplex over W with G = identity (w_simplex_update_kernel): the workgroup also leaves, for its 32 entries of component
  // kk = entry / n_pad (n_pad a multiple of 32), what the bracket and the root of that component's multiplier need -
  // sum, maximum and count of the positive numerators W A (dicotomy.py:29-49) - in bparts[3 * workgroup ..]; else null
  const float* bw_old;
  double* bparts;
  int bn, bk, bn_pad;
};

__global__ __launch_bounds__(256) void w_reduce_kernel(const WReduceArgs a) {
  __shared__ double fscratch[5 * (ESPM_HP_NSCALAR + 2 * KP + 1)];
  __shared__ float s_part[8][32];
  if ((int)blockIdx.x >= a.nred_blocks) {  // the extra workgroups: one value of the record reduction each (h_finalize_one); the boundary rows with the one that needs no records
    const int job = (int)blockIdx.x - a.nred_blocks;
    if (a.halo_top && job == H_FINALIZE_NV) {
      for (int e = threadIdx.x; e < a.halo_k * a.halo_ny; e += 256) {
        const int kk = e / a.halo_ny, j = e - kk * a.halo_ny;
        a.halo_top[e] = a.halo_h[(size_t)kk * a.halo_ppad + j];
        a.halo_bot[e] = a.halo_h[(size_t)kk * a.halo_ppad + (size_t)(a.halo_nx - 1) * a.halo_ny + j];
      }
    }
    h_finalize_one(a.fin, job, fscratch);
    return;
  }
  const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + col;
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  if (e < a.total) {
    int b = grp;
    for (; b + 56 < a.nblk; b += 64) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += a.slab[(size_t)(b + 8 * u) * a.total + e];
    }
    for (int u = 0; b < a.nblk; b += 8, ++u) acc[u & 7] += a.slab[(size_t)b * a.total + e];
  }
  s_part[grp][col] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (grp == 0) {   // (32 lanes: half of wave 0)
    float t = 0.f;
    if (e < a.total) {
#pragma unroll
      for (int g = 0; g < 8; ++g) t += s_part[g][col];
      a.out[e] = t;
    }
    if (a.bparts) {
      const int kk = e / a.bn_pad, c = e - kk * a.bn_pad;
      const float num = (e < a.total && c < a.bn) ? a.bw_old[(size_t)c * a.bk + kk] * t : 0.f;   // updates.py:59 (G = identity)
      double sum = num > 0.f ? (double)num : 0.0, cnt = num > 0.f ? 1.0 : 0.0;
      float mx = fmaxf(num, 0.f);
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {   // (fixed order: the same partials run to run)
        sum += __shfl_xor(sum, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      }
      if (col == 0) {
        a.bparts[3 * (size_t)blockIdx.x] = sum;
        a.bparts[3 * (size_t)blockIdx.x + 1] = (double)mx;
        a.bparts[3 * (size_t)blockIdx.x + 2] = cnt;
      }
    }
  }
}

// ---- Slab (or rank-record) reduction with the W update folded in: G = identity, no simplex_W -------------------
// When W' needs nothing global beyond the row sums of the new H (updates.py:58-60, :70-76 with G = I and no
// simplex over W), the update of an entry of W only needs the matching entry of A = sum of the sources: the
// workgroups that reduce the sources finish "their" entries of W right away - W' = max(W A / rowsum(H'), eps),
// fixed_W, the row of G W' for the next half step - instead of one workgroup doing all of W afterwards.  What IS
// global (column sums of G W', mean of W' for rel_W) leaves as per-workgroup partials for w_update_tail_kernel.
//   sources: `nsrc` arrays of (k, n_pad) floats, `src_stride` bytes apart: the slabs of the W accumulation, or
//            the A blocks of the ranks' records (sharded image), always summed in the same fixed order.
//   row sums of the new H: from the H-step's per-workgroup records (same order of operations as h_finalize_body,
//            so the value equals hstat's), or the sum over the ranks' records (which this kernel also turns into
//            the global hstat, like shard_combine).
// Workgroup (kk, j) owns channels [32 j, 32 j + 32) of component kk; one extra workgroup runs h_finalize_body.
__global__ __launch_bounds__(256) void w_reduce_update_kernel(const WUpdateArgs a) {
  __shared__ double fscratch[5 * (ESPM_HP_NSCALAR + 2 * KP + 1)];
  __shared__ float s_part[8][32];
  __shared__ double s_rsw[4];
  const int nwg = a.k * a.nbk;
  if ((int)blockIdx.x >= nwg) {  // the extra workgroups: one value of the H-step's record reduction each (h_finalize_one)
#ifndef ESPM_EXPERIMENT_NO_FINALIZE   // (TIMING ONLY when defined: is the record reduction what this launch ends with?)
    h_finalize_one(a.fin, (int)blockIdx.x - nwg, fscratch);
#endif
    return;
  }
  const int kk = blockIdx.x / a.nbk, j = blockIdx.x - kk * a.nbk;
  const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int c = 32 * j + col;
  const int e = kk * a.n_pad + c;
  auto src = [&](int b) { return reinterpret_cast<const float*>(a.src + (size_t)b * a.src_stride)[e]; };
  // Everything this workgroup needs from memory is requested up front - 32 sources per thread (256 slabs), its share of
  // the H-step's records - so that ONE memory round trip and ONE barrier separate the launch from the update: the kernel
  // is pure latency (8 us before, of an iteration of 150).
  constexpr int INFLIGHT = 32;
  float v[INFLIGHT];
  const bool live = c < a.n_pad;
#pragma unroll
  for (int u = 0; u < INFLIGHT; ++u) {
    const int b = grp + 8 * u;
    v[u] = (live && b < a.nsrc) ? src(b) : 0.f;
  }
  float wo_pre, fx_pre;
  w_update_preload(a, kk, c, threadIdx.x < 32, wo_pre, fx_pre);   // (lanes 0..31 of wave 0 own the 32 entries)
  double rsp = 0.0;   // slab mode: this thread's share of row sum kk of the new H (the order of h_finalize_body: same value as hstat's)
  if (a.hpart) {
    const size_t nb = a.nblk_h;
    for (int b = threadIdx.x; b < a.nblk_h; b += 256) rsp += a.hpart[(ESPM_HP_ROWSUM + kk) * nb + b];
  }
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = ((v[u] + v[u + 8]) + v[u + 16]) + v[u + 24];   // (the order of the loop below: source b ascending per partial)
  if (live) {
    int b = grp + 8 * INFLIGHT;
    for (; b + 56 < a.nsrc; b += 64) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += src(b + 8 * u);
    }
    for (int u = 0; b < a.nsrc; b += 8, ++u) acc[u & 7] += src(b);
  }
  s_part[grp][col] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  // row sum of component kk of the new H
  double rs = 0.0;
  if (a.hpart) {
    rsp = wave_sum(rsp);
    if ((threadIdx.x & 63) == 0) s_rsw[threadIdx.x >> 6] = rsp;
    __syncthreads();   // (also orders s_part)
    rs = ((s_rsw[0] + s_rsw[1]) + s_rsw[2]) + s_rsw[3];   // wave order, like block_reduce
  } else if (a.hstat_rs) {
    rs = a.hstat_rs[ESPM_HS_ROWSUM + kk];
    __syncthreads();
  } else {
    for (int r = 0; r < a.nsrc; ++r)
      rs += reinterpret_cast<const double*>(a.src + (size_t)r * a.src_stride + a.rec_hstat_off)[ESPM_HS_ROWSUM + kk];
    if (blockIdx.x == 0 && threadIdx.x < ESPM_HS_STRIDE) {  // global statistics of the new H (as shard_combine)
      double t = 0.0;
      for (int r = 0; r < a.nsrc; ++r) {
        const double v2 = reinterpret_cast<const double*>(a.src + (size_t)r * a.src_stride + a.rec_hstat_off)[threadIdx.x];
        t = (int)threadIdx.x < ESPM_HS_MAX ? t + v2 : fmax(t, v2);
      }
      a.hstat_out[threadIdx.x] = t;
    }
    __syncthreads();
  }
  if (threadIdx.x < 64) {  // wave 0; its first 32 lanes own the 32 entries
    float t = 0.f;
    const bool owns = grp == 0 && c < a.n_pad;
    if (owns) {
#pragma unroll
      for (int g = 0; g < 8; ++g) t += s_part[g][col];
    }
    w_update_entries(a, kk, c, e, owns, t, rs, nwg, blockIdx.x, wo_pre, fx_pre);
  }
}

// ---- W update under the simplex over W, G = identity, all rows in the simplex: many workgroups instead of one ----------------
// With G = identity every denominator of a column of W is the same number (rowsum of H', updates.py:60), so the multiplier's
// function is f(delta) = S / delta + n0 eps - 1 in delta = nu + rowsum, with S the sum of the positive numerators and n0 the
// rows without one: what the reference's bisection (dicotomy.py:111-173, global stop rule) does to it follows from S, the
// largest numerator and the counts alone.  w_reduce_kernel leaves those per 32 channels (WReduceArgs::bparts); here EVERY
// workgroup (component kk, 32 channels - the geometry of w_reduce_update_kernel) adds the partials of all components in a
// fixed order, walks the same decisions as w_finish_fast_kernel - bracket, root, the sweep the reference stops at (estimate
// from the linearisation, the exact f where that is within 1 % of the tolerance), the midpoint of that sweep - and updates
// its 32 entries with delta in the place of the row sum.  37 us of one workgroup become 8 us of 320.
// (A positive numerator below eps delta counts as itself, not as eps: at most n eps = 2e-11 of f.)
struct WSimplexArgs {
  WUpdateArgs u;             // the update of the entries and what it leaves for the tail (src / hpart unused: A is read from u.a_out)
  const double* bparts;      // [k * nbk][3]
  const double* hstat;       // statistics of the new H (row sums)
  double rows;               // rows of W (all of them in the simplex)
  double tol;
};

__global__ __launch_bounds__(64) void w_simplex_update_kernel(const WSimplexArgs x) {
  const WUpdateArgs& a = x.u;
  const int nwg = a.k * a.nbk;
  const int kk = blockIdx.x / a.nbk, j = blockIdx.x - kk * a.nbk;
  const int lane = threadIdx.x;
  // the entries first: their loads fly while the multipliers are worked out
  const int c = 32 * j + (lane & 31);
  const int e = kk * a.n_pad + c;
  const bool owns = lane < 32 && c < a.n_pad;
  const float t_e = owns ? a.a_out[e] : 0.f;
  float wo_pre, fx_pre;
  w_update_preload(a, kk, c, owns, wo_pre, fx_pre);
  double ssum[KP], smax[KP], spos[KP], rs[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    ssum[q] = 0.0; smax[q] = 0.0; spos[q] = 0.0; rs[q] = 1.0;
    if (q < a.k) {
      double s1 = 0.0, s3 = 0.0, s2 = 0.0;
      for (int b = lane; b < a.nbk; b += 64) {
        const double* p = x.bparts + 3 * ((size_t)q * a.nbk + b);
        s1 += p[0];
        s2 = fmax(s2, p[1]);
        s3 += p[2];
      }
      ssum[q] = wave_sum(s1);
      smax[q] = wave_max(s2);
      spos[q] = wave_sum(s3);
      rs[q] = x.hstat[ESPM_HS_ROWSUM + q];
    }
  }
  // per component (every lane the same arithmetic): bracket [ad, ad + width] in delta, root, slope, place of the root
  const double eps = (double)a.log_shift;
  double root[KP], fder[KP], ad[KP], width[KP], uu[KP], cst[KP];
  bool solve[KP];
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    solve[q] = q < a.k && ssum[q] > 0.0 && ssum[q] < INFINITY;
    const double den = (double)(float)rs[q];                 // dv = colsum(G) * (float) rowsum = the fp32 row sum
    const double lo = smax[q] / 2 - den;                     // a, dicotomy.py:29-43
    const double hi = x.rows * smax[q] / 0.5 - den;          // b, dicotomy.py:49
    cst[q] = (x.rows - spos[q]) * eps;                       // the rows without a positive numerator: eps each
    ad[q] = lo + den;
    width[q] = hi - lo;
    // Newton from delta = S: f(S) = cst; the finish accepts |f| <= 1e-11, else converges to S / (1 - cst)
    root[q] = solve[q] ? (fabs(cst[q]) <= 1e-11 ? ssum[q] : ssum[q] / (1.0 - cst[q])) : 1.0;
    fder[q] = solve[q] ? -ssum[q] / (root[q] * root[q]) : 0.0;
    uu[q] = solve[q] ? fmin(fmax((root[q] - ad[q]) / width[q], 0.0), 1.0) : 0.5;
  }
  auto mid_frac = [](double u1, int t) {
    const double scale = ldexp(1.0, t - 1);
    const double cell = fmin(floor(u1 * scale), scale - 1.0);
    return ldexp(2.0 * cell + 1.0, -t);
  };
  // the sweep the reference stops at: lane l looks at sweeps l + 1 and l + 65 (at most 101)
  unsigned long long mc[2], mb[2];
  for (int hf = 0; hf < 2; ++hf) {
    const int t = 1 + lane + 64 * hf;
    double est = 0.0;
#pragma unroll
    for (int q = 0; q < KP; ++q)
      if (q < a.k) est = fmax(est, fabs(fder[q] * ((ad[q] + width[q] * mid_frac(uu[q], t)) - root[q])));
    const bool certain = t <= 101 && (est <= 0.99 * x.tol || t == 101);
    const bool band = t <= 101 && !certain && est <= 1.01 * x.tol;
    mc[hf] = __ballot(certain);
    mb[hf] = __ballot(band);
  }
  int t_stop = 101;
  for (;;) {   // (uniform)
    const unsigned long long w0 = mc[0] | mb[0], w1 = mc[1] | mb[1];
    if (!w0 && !w1) break;
    const int hf = w0 ? 0 : 1;
    const int bit = __ffsll((long long)(hf ? w1 : w0)) - 1;
    const int t = 1 + bit + 64 * hf;
    if ((mc[hf] >> bit) & 1ull) { t_stop = t; break; }
    double worst = 0.0;
#pragma unroll
    for (int q = 0; q < KP; ++q)
      if (q < a.k && fder[q] != 0.0) {
        const double d = ad[q] + width[q] * mid_frac(uu[q], t);
        worst = fmax(worst, fabs(ssum[q] / d + cst[q] - 1.0));
      }
    if (worst <= x.tol) { t_stop = t; break; }
    mb[hf] &= ~(1ull << bit);
  }
  // delta of this workgroup's component: den + nu = (den - d*) + delta = delta (no multiplier without a positive numerator)
  double delta = rs[0];
#pragma unroll
  for (int q = 0; q < KP; ++q)
    if (q == kk) delta = solve[q] ? ad[q] + width[q] * mid_frac(uu[q], t_stop) : (double)(float)rs[q];
  w_update_entries(a, kk, c, e, owns, t_e, delta, nwg, blockIdx.x, wo_pre, fx_pre);
}

// Column sums of G W' and rel_W (base.py:323) from the partials and W', W: one workgroup (w_tail_body, mu_common.hpp).
// 256 threads: the cross-wave stage of a block reduction costs per wave, and everything here is latency - the
// entries of W are requested up front, before the partials are reduced, so that only one memory round trip and
// two short reductions separate the launch from the result.
constexpr int WT_THREADS = 256;
__global__ __launch_bounds__(WT_THREADS) void w_update_tail_kernel(const WTailArgs a) {
  __shared__ double scratch[(WT_THREADS / 64 + 1) * (KP + 1) + 1];
  w_tail_body<40>(a, scratch);   // 40 x 256 = 10240 entries of W held in registers (the headline size); more take the loop
}

int launch_w_reduce(const float* slab, float* out, int nblk, int total, const HFinalizeArgs* fused_finalize,
                    hipStream_t stream, const float* bw_old, double* bparts, int n, int k, int n_pad) {
  WReduceArgs a = {};   // (no record to pack into)
  a.bw_old = bw_old;
  a.bparts = bparts;
  a.bn = n;
  a.bk = k;
  a.bn_pad = n_pad;
  a.slab = slab;
  a.out = out;
  a.nblk = nblk;
  a.total = total;
  a.nred_blocks = (total + 31) / 32;
  a.fuse_finalize = fused_finalize != nullptr;
  if (fused_finalize) a.fin = *fused_finalize;
  hipLaunchKernelGGL(w_reduce_kernel, dim3(a.nred_blocks + (fused_finalize ? H_FINALIZE_JOBS : 0)), dim3(256), 0, stream, a);
  return check_hip(hipGetLastError(), "w_reduce launch");
}

// Slab reduction straight into a rank's record: A block, statistics of the new H (the finalize workgroup writes them
// there), boundary rows of the new H.
int launch_w_reduce_pack(const float* slab, int nblk, int k, int n_pad, const HFinalizeArgs& fin_to_record,
                         const float* h_new, int nx, int ny, int p_pad, int with_halo, void* rec, hipStream_t stream) {
  WReduceArgs a = {};   // (no simplex over W: no partials of its bracket)
  unsigned char* r = static_cast<unsigned char*>(rec);
  const int na = k * n_pad;
  a.slab = slab;
  a.out = reinterpret_cast<float*>(r);
  a.nblk = nblk;
  a.total = na;
  a.nred_blocks = (na + 31) / 32;
  a.fuse_finalize = 1;
  a.fin = fin_to_record;
  a.halo_h = h_new;
  a.halo_top = with_halo ? reinterpret_cast<float*>(r + (size_t)na * 4 + ESPM_HS_STRIDE * 8) : nullptr;
  a.halo_bot = with_halo ? a.halo_top + (size_t)k * ny : nullptr;
  a.halo_k = k;
  a.halo_nx = nx;
  a.halo_ny = ny;
  a.halo_ppad = p_pad;
  hipLaunchKernelGGL(w_reduce_kernel, dim3(a.nred_blocks + H_FINALIZE_JOBS), dim3(256), 0, stream, a);
  return check_hip(hipGetLastError(), "w_reduce_pack launch");
}

// the tail's view of a local W update: partials in f.scratch, W before / after, where the results go
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
  t.nbk = (f.n_pad + 31) / 32;
  t.rel_tol = f.rel_tol;
  return t;
}

int w_tail_defer_or_launch(const WFinishArgs& f, WTailArgs* defer_tail, hipStream_t stream, const char* what) {
  const WTailArgs t = make_w_tail_args(f);
  if (defer_tail)   // (espm_mu_iterate: the tail rides in the next H-step's launch, or in launch_w_update_tail at the end)
    *defer_tail = t;
  else
    hipLaunchKernelGGL(w_update_tail_kernel, dim3(1), dim3(WT_THREADS), 0, stream, t);
  return check_hip(hipGetLastError(), what);
}

int launch_w_reduce_update(const WFinishArgs& f, const void* src, size_t src_stride, int nsrc, float* a_out,
                           const double* hpart, int nblk_h, const double* hstat_rs, size_t rec_hstat_off, double* hstat_out,
                           const HFinalizeArgs* fused_finalize, hipStream_t stream, WTailArgs* defer_tail) {
  WUpdateArgs a = make_w_update_args(f);
  a.src = static_cast<const unsigned char*>(src);
  a.src_stride = src_stride;
  a.nsrc = nsrc;
  a.a_out = a_out;
  a.hpart = hpart;
  a.hstat_rs = hstat_rs;
  a.nblk_h = nblk_h;
  a.rec_hstat_off = rec_hstat_off;
  a.hstat_out = hstat_out;
  a.fuse_finalize = fused_finalize != nullptr;
  if (fused_finalize) a.fin = *fused_finalize;
  hipLaunchKernelGGL(w_reduce_update_kernel, dim3(a.k * a.nbk + (fused_finalize ? H_FINALIZE_JOBS : 0)), dim3(256), 0, stream, a);
  return w_tail_defer_or_launch(f, defer_tail, stream, "w_reduce_update launch");
}

int launch_w_simplex_update(const WFinishArgs& f, float* a_inout, const double* bparts, double tol, hipStream_t stream, WTailArgs* defer_tail) {
  WSimplexArgs x;
  x.u = make_w_update_args(f);   // (no sources, no records: A is read from a_out, the row sums from hstat)
  x.u.a_out = a_inout;
  x.u.breg_sr = nullptr;
  x.u.pg_gamma_w = 0.f;
  x.u.pg_track = 0;
  x.bparts = bparts;
  x.hstat = f.hstat;
  x.rows = (double)f.n;
  x.tol = tol;
  hipLaunchKernelGGL(w_simplex_update_kernel, dim3(x.u.k * x.u.nbk), dim3(64), 0, stream, x);
  if (int rc = check_hip(hipGetLastError(), "w_simplex_update launch")) return rc;
  return w_tail_defer_or_launch(f, defer_tail, stream, "w_simplex_update tail launch");
}

int launch_w_update_tail(const WTailArgs& t, hipStream_t stream) {
  hipLaunchKernelGGL(w_update_tail_kernel, dim3(1), dim3(WT_THREADS), 0, stream, t);
  return check_hip(hipGetLastError(), "w_update_tail launch");
}

}  // namespace espm
