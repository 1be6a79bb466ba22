// The second launch of an iteration on a SHARDED image with G = identity (the W step as a whole: mu_w_parts.hpp).
#include "mu_w_parts.hpp"

namespace espm {

// ---- Slab reduction, record exchange and W update of a SHARDED image in ONE launch (espm_mu_shard_exchange_finish) ----------
// The sharded W step after the accumulation used to be four launches - slab reduction into the rank's record, post, wait,
// sum over the ranks' records + update - i.e. ~17 us of launch latencies around 100 KB of traffic.  Here the reduction
// workgroup (kk, j) that has summed the slabs for ITS 32 entries of A delivers that 128-byte piece to every rank's mailbox
// itself (P2P stores), raises ITS flag there, waits for the same piece of every other rank, sums the pieces in rank order
// (bit-identical W on all ranks) and updates its entries of W: the exchange is as fine-grained as the dependency.  The extra
// workgroup reduces the H-step's records, delivers the statistics of the new H block to every rank and its boundary rows
// to the neighbours (and to itself), and raises flag `nwg`; every reduction workgroup also waits for that flag of every
// rank (the global row sums are in the denominator of W'), so by the end of the launch the halo rows of the next H-step
// have arrived too.  Every workgroup posts before it waits and the grid (k n_pad / 32 + 1 workgroups of 256 threads) is
// resident at once: no deadlock; waits are bounded (a lost peer is counted in the mailbox's error word).
#ifndef ESPM_XCHG_SMALL_WORLD
#define ESPM_XCHG_SMALL_WORLD 8
#endif
struct WExchangeArgs {
  WUpdateArgs u;
  unsigned char* mbox[16];   // every rank's mailbox as mapped here
  int world, rank, nfl, with_halo;
  size_t rec_bytes, slot_base, wgflags_off, gran_off, err_off, hstat_off, top_off, bot_off;   // (gran_off: of this sequence number's parity)
  unsigned int seq;
  long long max_ticks;
  int release;               // flags stored with release order at system scope (espm_xchg_set_order) instead of behind s_waitcnt vmcnt(0) alone
  const float* halo_h;
  int halo_k, halo_nx, halo_ny, halo_ppad;
  // simplex over W with G = identity: the summed A and, per reduction workgroup, what the bracket of its component's multiplier
  // needs (the three doubles w_reduce_kernel leaves) go out INSTEAD of the update - w_simplex_update_kernel follows; else null
  double* bparts;
};

template <int MAXW>   // ranks the unrolled polls are laid out for (8: a node; 16: the mailbox's limit) - the kernel's code size follows it
__global__ __launch_bounds__(256) void w_exchange_update_kernel(const WExchangeArgs x) {
  const WUpdateArgs& a = x.u;
  __shared__ double fscratch[5 * (ESPM_HP_NSCALAR + 2 * KP + 1)];
  __shared__ float s_part[8][32];
  const int nwg = a.k * a.nbk;
  auto record = [&](int dst, int src_rank) { return x.mbox[dst] + x.slot_base + (size_t)src_rank * x.rec_bytes; };
  auto flag = [&](int dst, int src_rank, int idx) {
    return reinterpret_cast<unsigned int*>(x.mbox[dst] + x.wgflags_off + ((size_t)src_rank * x.nfl + idx) * sizeof(unsigned int));
  };
  // Progress without the whole grid being resident (grids of k n_pad / 32 + 1 workgroups exceed what the device
  // holds at once from k = 8, n = 8192 on): workgroups are dispatched in index order, every workgroup POSTS before it waits,
  // and what it waits for was posted by the workgroup of the SAME index on every rank (reduction workgroup wg: the pieces of
  // the workgroups wg) or by the first H_FINALIZE_JOBS workgroups (the record reduction's: only reduction workgroup 0 waits for them).  The
  // lowest-indexed unfinished workgroup of every rank is therefore resident and can finish; whatever it frees lets the next
  // one in.  (Round 2 had the extra workgroup LAST and every reduction workgroup waiting for it: a grid beyond the residency
  // dead-locked for the 2 s bound of the waits.  An occupancy query as a second guard was tried and dropped: on this stack
  // hipOccupancyMaxActiveBlocksPerMultiprocessor answers 2 workgroups per CU for this 256-thread kernel, which would send
  // the headline's 321 workgroups down the four-launch path - profiles/r03c_shard_iter_residency_guard.log.)  The waits stay bounded.
  // granule g of rank src_rank's contribution, in rank dst's mailbox (GRAN granules per source rank): g = 32 wg + column for a
  // reduction workgroup's piece, 32 nfl + 2 wg + half for its row sum, 34 nfl + 2 i + half for statistic i of the new H block
  const size_t GRAN = (size_t)34 * x.nfl + 2 * ESPM_HS_STRIDE;
  auto gran = [&](int dst, int src_rank, int g) {
    return reinterpret_cast<unsigned long long*>(x.mbox[dst] + x.gran_off) + (size_t)src_rank * GRAN + g;
  };
  constexpr int NJ = H_FINALIZE_JOBS;
  if ((int)blockIdx.x < NJ) {  // the extra workgroups, FIRST in the grid: one value of the record reduction each (h_finalize_one);
    // the one whose value needs no records (SUMY) also posts the boundary rows of this rank's new H block
    const int job = (int)blockIdx.x;
    const bool halo_job = job == H_FINALIZE_NV;
    // the boundary rows first - they are in memory since the launch before this one, and nobody needs them before the NEXT
    // launch: their stores are long acknowledged when the flag that covers them is raised at the end
    // (every store into a mailbox is a system-scope write-through store: whatever memory type a peer's mapping has here,
    //  the data is on its way to that rank's memory when the store is acknowledged, and `s_waitcnt vmcnt(0)` orders the flag)
    if (halo_job && x.with_halo) {
      for (int d = -1; d <= 1; ++d) {   // the neighbours read these rows as their halo; this rank keeps a copy (record layout)
        const int r = x.rank + d;
        if (r < 0 || r >= x.world) continue;
        float* top = reinterpret_cast<float*>(record(r, x.rank) + x.top_off);
        float* bot = reinterpret_cast<float*>(record(r, x.rank) + x.bot_off);
        if ((x.halo_ny & 3) == 0) {   // rows of whole quads: 16-byte write-through stores (a 4-byte store to a peer is a fabric write of its own)
          typedef float xf4 __attribute__((ext_vector_type(4)));
          for (int e = 4 * threadIdx.x; e < x.halo_k * x.halo_ny; e += 4 * 256) {
            const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
            const xf4 vt = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + j);
            const xf4 vb = *reinterpret_cast<const xf4*>(x.halo_h + (size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j);
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(top + e), "v"(vt) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(bot + e), "v"(vb) : "memory");
          }
        } else {
          for (int e = threadIdx.x; e < x.halo_k * x.halo_ny; e += 256) {
            const int kk = e / x.halo_ny, j = e - kk * x.halo_ny;
            __hip_atomic_store(top + e, x.halo_h[(size_t)kk * x.halo_ppad + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(bot + e, x.halo_h[(size_t)kk * x.halo_ppad + (size_t)(x.halo_nx - 1) * x.halo_ny + j], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
      }
    }
    // a statistic: reduced, then one granule {half of a double, sequence number} per half and destination - value and "it is
    // there" in one store, like the pieces: reduction workgroup 0 of every rank has it one trip over the link after the reduction
    __shared__ double s_hstat[ESPM_HS_STRIDE];
    HFinalizeArgs fin = a.fin;
    double* rec_hstat = fin.hstat_out;   // this rank's record in its OWN mailbox (the plain copy: espm_xchg_records' readers)
    fin.hstat_out = s_hstat;
    h_finalize_one(fin, job, fscratch);
    if (halo_job) {
      // the boundary rows' stores were issued long ago: this wait returns at once
      // (the mailboxes are uncached memory: a store is delivered once it is acknowledged - no cache to write back, so no
      //  system-scope fence, which would flush this XCD's whole L2 - only ORDER: every thread's stores before any flag)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if ((int)threadIdx.x < x.world) xchg_store_flag(flag(threadIdx.x, x.rank, nwg), x.seq, x.release);
      return;
    }
    // which entry of the statistics this job's value is (row sums [0, KP), maxima [KP, 2 KP)); the others go to the history only
    int js = -1;
    if (job >= ESPM_HP_ROWSUM && job < ESPM_HP_ROWSUM + KP) js = ESPM_HS_ROWSUM + (job - ESPM_HP_ROWSUM);
    if (job >= 5 + KP && job < 5 + 2 * KP) js = ESPM_HS_MAX + (job - (5 + KP));
    if (js < 0) return;
    __syncthreads();   // (thread 0 of h_finalize_one wrote s_hstat[js])
    if ((int)threadIdx.x < 2 * x.world) {
      const int r = threadIdx.x >> 1, half_i = threadIdx.x & 1;
      const unsigned long long bits = __builtin_bit_cast(unsigned long long, s_hstat[js]);
      const unsigned int half = half_i ? (unsigned int)(bits >> 32) : (unsigned int)bits;
      __hip_atomic_store(gran(r, x.rank, 34 * x.nfl + 2 * js + half_i), ((unsigned long long)x.seq << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) rec_hstat[js] = s_hstat[js];
    return;
  }
  const int wg = (int)blockIdx.x - NJ;   // reduction workgroup (component kk, 32 channels)
  const int kk = wg / a.nbk, j = wg - kk * a.nbk;
  const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int c = 32 * j + col;
  const int e = kk * a.n_pad + c;
  auto src = [&](int b) { return reinterpret_cast<const float*>(a.src + (size_t)b * a.src_stride)[e]; };
  constexpr int INFLIGHT = 32;
  float v[INFLIGHT];
  const bool live = c < a.n_pad;
#pragma unroll
  for (int u = 0; u < INFLIGHT; ++u) {
    const int b = grp + 8 * u;
    v[u] = (live && b < a.nsrc) ? src(b) : 0.f;
  }
  float wo_pre, fx_pre;
  w_update_preload(a, kk, c, threadIdx.x < 32, wo_pre, fx_pre);
  // Row sum kk of THIS rank's new H block from the H-step's records, in the order of h_finalize_body (the same value the extra
  // workgroup leaves in the statistics): it travels with the piece, so that the W update waits for pieces only - not for the
  // extra workgroups' record reductions, which only workgroup 0 (the global statistics for the NEXT H-step) still waits for.
  __shared__ double s_rsw[4];
  double rsp = 0.0;
  {
    const size_t nb = a.nblk_h;
    for (int b = threadIdx.x; b < a.nblk_h; b += 256) rsp += a.hpart[(ESPM_HP_ROWSUM + kk) * nb + b];
  }
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = ((v[u] + v[u + 8]) + v[u + 16]) + v[u + 24];
  if (live) {
    int b = grp + 8 * INFLIGHT;
    for (; b + 56 < a.nsrc; b += 64) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += src(b + 8 * u);
    }
    for (int u = 0; b < a.nsrc; b += 8, ++u) acc[u & 7] += src(b);
  }
  s_part[grp][col] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  rsp = wave_sum(rsp);
  if ((threadIdx.x & 63) == 0) s_rsw[threadIdx.x >> 6] = rsp;
  __syncthreads();
  if (threadIdx.x < 64) {  // wave 0: lanes 0..31 own the 32 entries, lanes 32 and 33 the two halves of the row sum
    const int lane = threadIdx.x;
    const bool owns = grp == 0 && live;
    float t = 0.f;
    if (owns) {
#pragma unroll
      for (int g = 0; g < 8; ++g) t += s_part[g][col];
    }
    // A value travels as ONE 8-byte granule {bits, sequence number} (system scope, write-through): the store that delivers it is
    // also what says it is there - no drain, no flag, no second trip over the link (MI355X_MICROARCH.md, handoff-1to1 against
    // handoff-flag; an aligned 8-byte store is observed whole).  The slot of a sequence number's parity is rewritten two
    // exchanges later, which a peer can only do after this rank posted the exchange in between (mu_xchg.hip).
    const double rs_mine = ((s_rsw[0] + s_rsw[1]) + s_rsw[2]) + s_rsw[3];   // wave order, like block_reduce
    const unsigned long long rs_bits = __builtin_bit_cast(unsigned long long, rs_mine);
    const bool sends = owns || lane == 32 || lane == 33;
    const int g_idx = lane < 32 ? 32 * wg + col : 32 * x.nfl + 2 * wg + (lane - 32);
    const unsigned int bits = lane < 32 ? __float_as_uint(t) : (lane == 32 ? (unsigned int)rs_bits : (unsigned int)(rs_bits >> 32));
    const unsigned long long mine = ((unsigned long long)x.seq << 32) | bits;
    if (sends)
      for (int r = 0; r < x.world; ++r) __hip_atomic_store(gran(r, x.rank, g_idx), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // every rank's granule of the same index: polled together (one load per rank in flight), bounded
    unsigned int* err = reinterpret_cast<unsigned int*>(x.mbox[x.rank] + x.err_off);
    unsigned int got[MAXW];
    {
      const long long t0 = wall_clock64();
      bool all = !sends;
      for (;;) {
        unsigned long long v[MAXW];
#pragma unroll
        for (int r = 0; r < MAXW; ++r)
          v[r] = (sends && r < x.world) ? __hip_atomic_load(gran(x.rank, r, g_idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ((unsigned long long)x.seq << 32);
        all = true;
#pragma unroll
        for (int r = 0; r < MAXW; ++r) {
          all = all && (unsigned int)(v[r] >> 32) == x.seq;
          got[r] = (unsigned int)v[r];
        }
        if (__builtin_amdgcn_ballot_w64(!all) == 0) break;
        if (wall_clock64() - t0 > x.max_ticks) {   // a peer that never delivers must not hang the device: give up, count it
          if (!all) atomicAdd(err, 1u);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    // added in rank order: the same sums on every rank
    float tt = 0.f;
    double rs = 0.0;
#pragma unroll
    for (int r = 0; r < MAXW; ++r)
      if (r < x.world) {
        tt += __uint_as_float(got[r]);
        const unsigned long long lo = (unsigned int)__builtin_amdgcn_readlane((int)got[r], 32), hi = (unsigned int)__builtin_amdgcn_readlane((int)got[r], 33);
        rs += __builtin_bit_cast(double, (hi << 32) | lo);
      }
    if (x.bparts) {   // the numerators' sum, maximum and count of positives (dicotomy.py:29-49), as w_reduce_kernel forms them
      if (owns) a.a_out[e] = tt;
      const float num = (owns && c < a.n) ? wo_pre * tt : 0.f;   // updates.py:59 (G = identity)
      double sum = num > 0.f ? (double)num : 0.0, cnt = num > 0.f ? 1.0 : 0.0;
      float mx = fmaxf(num, 0.f);
#pragma unroll
      for (int off = 16; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      }
      if (lane == 0) {
        x.bparts[3 * (size_t)wg] = sum;
        x.bparts[3 * (size_t)wg + 1] = (double)mx;
        x.bparts[3 * (size_t)wg + 2] = cnt;
      }
    } else {
      w_update_entries(a, kk, c, e, owns, tt, rs, nwg, wg, wo_pre, fx_pre);
    }
#ifdef ESPM_EXPERIMENT_XCHG_NO_STATS_WAIT   // TIMING ONLY: is the statistics' path (record reduction in the extra workgroup, granules, this wait) what the launch ends with?
    if (false) {
#else
    if (wg == 0) {  // global statistics of the new H (as shard_combine): every rank's extra workgroup sends them as granules
#endif
      // one lane per half of a statistic: 2 ESPM_HS_STRIDE halves, 64 per pass (one pass up to 16 components, two in the widest build)
      for (int hl = lane; hl < ((2 * ESPM_HS_STRIDE + 63) & ~63); hl += 64) {
      const bool polls = hl < 2 * ESPM_HS_STRIDE;
      unsigned int hv[MAXW];
      {
        const long long t0 = wall_clock64();
        bool all = !polls;
        for (;;) {
          unsigned long long v[MAXW];
#pragma unroll
          for (int r = 0; r < MAXW; ++r)
            v[r] = (polls && r < x.world) ? __hip_atomic_load(gran(x.rank, r, 34 * x.nfl + hl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                          : ((unsigned long long)x.seq << 32);
          all = true;
#pragma unroll
          for (int r = 0; r < MAXW; ++r) {
            all = all && (unsigned int)(v[r] >> 32) == x.seq;
            hv[r] = (unsigned int)v[r];
          }
          if (__builtin_amdgcn_ballot_w64(!all) == 0) break;
          if (wall_clock64() - t0 > x.max_ticks) {
            if (!all) atomicAdd(err, 1u);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      double g = 0.0;
#pragma unroll
      for (int r = 0; r < MAXW; ++r)
        if (r < x.world) {   // lane 2 i holds the low half of statistic i, lane 2 i + 1 the high half
          const unsigned int other = (unsigned int)__shfl_xor((int)hv[r], 1, 64);
          const unsigned long long bits = (lane & 1) ? (((unsigned long long)hv[r] << 32) | other) : (((unsigned long long)other << 32) | hv[r]);
          const double v2 = __builtin_bit_cast(double, bits);
          g = (hl >> 1) < ESPM_HS_MAX ? g + v2 : fmax(g, v2);
        }
      if (polls && !(lane & 1)) a.hstat_out[hl >> 1] = g;
      }
      // the boundary rows of the neighbours (the next launch reads them): their flag
      if (lane < x.world) xchg_wait_flag(flag(x.rank, lane, nwg), x.seq, x.max_ticks, err);
    }
  }
}

int launch_w_exchange_update(const WFinishArgs& f, const void* slabs, size_t slab_stride, int nslab, float* a_out, double* hstat_out,
                             const HFinalizeArgs& fin, const espm_xchg* xc, unsigned int seq, const float* h_new, int nx, int ny, int p_pad,
                             int with_halo, hipStream_t stream, WTailArgs* defer_tail, double* bparts) {
  WExchangeArgs x;
  x.bparts = bparts;
  x.u = make_w_update_args(f);
  WUpdateArgs& a = x.u;
  a.src = static_cast<const unsigned char*>(slabs);
  a.src_stride = slab_stride;
  a.nsrc = nslab;
  a.a_out = a_out;
  a.hpart = fin.hpart;       // (every reduction workgroup forms the row sum it needs from the H-step's records itself)
  a.nblk_h = fin.nblk;
  a.hstat_out = hstat_out;
  a.fuse_finalize = 1;
  a.fin = fin;
  const int nwg = a.k * a.nbk;
  ESPM_REQUIRE(nwg + 1 <= xc->wgflags, "exchange: %d reduction workgroups, the mailbox holds flags for %d", nwg, xc->wgflags - 1);
  if (int rc = fill_w_mailbox_args(x, xc, seq, f, h_new, nx, ny, p_pad, with_halo)) return rc;
  x.hstat_off = (size_t)f.k * f.n_pad * 4;
  a.fin.hstat_out = reinterpret_cast<double*>(xc->mailbox + x.slot_base + (size_t)xc->rank * xc->record_bytes + x.hstat_off);
  if (xc->world <= ESPM_XCHG_SMALL_WORLD)
    hipLaunchKernelGGL(w_exchange_update_kernel<ESPM_XCHG_SMALL_WORLD>, dim3(nwg + H_FINALIZE_JOBS), dim3(256), 0, stream, x);
  else
    hipLaunchKernelGGL(w_exchange_update_kernel<16>, dim3(nwg + H_FINALIZE_JOBS), dim3(256), 0, stream, x);
  if (bparts) return check_hip(hipGetLastError(), "w_exchange_update launch");   // (the caller's w_simplex_update_kernel updates W and owns the tail)
  return w_tail_defer_or_launch(f, defer_tail, stream, "w_exchange_update launch");
}

}  // namespace espm
