// The chained H-only iteration (espm_mu_iterate_h): what an H-step launch does itself so that no launch stands between two H-steps.
//
// An H-step needs two things of the state it starts from that only a reduction over ALL pixels gives: the row sums of H (the mean
// in rel_H, base.py:324) and its row maxima (the Laplacian term of the rule, updates.py:139).  In a full iteration the W launches
// that follow the H-step reduce its per-workgroup records into hstat; in an H-only iteration nothing follows, and a launch of
// espm_mu_h_finalize between two H-steps is a launch of nearly pure latency.  The CHAIN instances of the H-step kernels
// (mu_h_kernel.hpp, mu_ell_kernel.hpp) instead
//   - reduce the 2 k values they need from the previous launch's records in every workgroup (chain_stats, at the start of the
//     kernel), and
//   - carry one extra workgroup that reduces ALL fields of those records into the previous step's history row and hstat
//     (chain_finalize_wg), off every other workgroup's path.
// The records ping-pong between two buffers by the parity of the iteration: a launch never reads what it writes.
//
// Both follow the order of operations of h_finalize_one (mu_common.hpp) - 256 virtual threads, thread t the blocks t, t + 256, ...
// in ascending order, the wave stage over each run of 64 virtual threads, the four runs in order - so the values are the bits
// espm_mu_h_finalize gives.  A (value, run of 64) pair is one unit of work for one real wave, whatever the workgroup's size.
#pragma once
#include "mu_common.hpp"

namespace espm {

// one unit: the wave stage of `field` over the virtual threads 64 q .. 64 q + 63 (every lane of the calling wave takes part)
__device__ __forceinline__ double chain_unit(const double* __restrict__ rec, int nblk, int field, int q, bool is_sum, double ident) {
  const int lane = threadIdx.x & 63;
  double v = ident;
  for (int b = 64 * q + lane; b < nblk; b += 256) {
    const double t = rec[(size_t)field * nblk + b];
    v = is_sum ? v + t : fmax(v, t);
  }
  return is_sum ? wave_sum(v) : wave_max(v);
}
// ... and the four runs in order (thread-local: after the barrier that follows the wave stage); scr[q * nv + i]
__device__ __forceinline__ double chain_combine(const double* scr, int nv, int i, bool is_sum) {
  double acc = scr[i];
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    const double o = scr[q * nv + i];
    acc = is_sum ? acc + o : (o > acc ? o : acc);
  }
  return acc;
}

// every workgroup: row sums (values 0 .. K - 1) and row maxima (K .. 2 K - 1) of the H the previous launch wrote; scr: 8 K doubles
template <int K>
__device__ __forceinline__ void chain_stats_wave_stage(const double* __restrict__ prev, int nblk, double* scr) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  for (int u = wave; u < 8 * K; u += nw) {
    const int i = u >> 2, q = u & 3;
    const bool is_sum = i < K;
    const double v = chain_unit(prev, nblk, is_sum ? ESPM_HP_ROWSUM + i : ESPM_HP_MAX + (i - K), q, is_sum, 0.0);
    if ((threadIdx.x & 63) == 0) scr[q * 2 * K + i] = v;
  }
}
// (the same value in every lane: kept in a scalar register, where the scalar loads of hstat_in leave it in the other instances)
__device__ __forceinline__ float chain_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <int K>
__device__ __forceinline__ double chain_stat(const double* scr, int i) { return chain_combine(scr, 2 * K, i, i < K); }

// What the epilogue needs of them (h_epilogue: rel_shift, mhv), in scalar registers - where the scalar loads of hstat_in leave them in
// the other instances.  The dense kernels form them at the start behind a barrier of its own (chain_stats) and hold them through the
// channel loop; the sparse kernel's walk has no scalar register to spare (held through it they cost its k = 7, 8 instances 28 and 25
// more spilled vector registers): it runs the wave stage at the start, ahead of the barrier behind its table fill, and combines in the
// epilogue (chain_stats_combine).
template <int K>
struct ChainStats {
  float rel_shift;   // base.py:324: tol * mean(H)
  float mhv[K];      // updates.py:139: max over the pixels of every row of H
};
template <int K>
__device__ __forceinline__ ChainStats<K> chain_stats_combine(const HStepArgs& a, const double* scr) {   // (behind a barrier that follows the wave stage)
  ChainStats<K> s;
  double tot = 0.0;
#pragma unroll
  for (int kk = 0; kk < K; ++kk) tot += chain_stat<K>(scr, kk);
  s.rel_shift = chain_uniform((float)((double)a.rel_tol * tot * a.inv_count));
#pragma unroll
  for (int kk = 0; kk < K; ++kk) s.mhv[kk] = chain_uniform((float)chain_stat<K>(scr, K + kk));
  return s;
}
template <int K>
__device__ __forceinline__ ChainStats<K> chain_stats(const HStepArgs& a, double* scr) {
  chain_stats_wave_stage<K>(a.chain_prev, a.chain_nb, scr);
  __syncthreads();
  return chain_stats_combine<K>(a, scr);
}

// the extra workgroup: h_finalize_one's jobs 0 .. NV (every value, and SUMY) by one workgroup of any size; scr: 4 NV doubles
__device__ __forceinline__ void chain_finalize_wg(const HFinalizeArgs& a, double* scr) {
  constexpr int NV = H_FINALIZE_NV, V_RELH = 4 + KP, V_MAX = 5 + KP, V_RELW = 5 + 2 * KP;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  auto field_of = [](int i) { return i < 4 + KP ? i : (i == V_RELH ? ESPM_HP_RELH : (i == V_RELW ? ESPM_HP_RELW : ESPM_HP_MAX + (i - V_MAX))); };
  for (int u = wave; u < 4 * NV; u += nw) {
    const int i = u >> 2, q = u & 3;
    const double v = chain_unit(a.hpart, a.nblk, field_of(i), q, i < 4 + KP, i == V_RELW ? -1.0 : 0.0);
    if ((threadIdx.x & 63) == 0) scr[q * NV + i] = v;
  }
  __syncthreads();
  const int job = threadIdx.x;
  if (job == NV) {   // sum_k colsum(GW)_k rowsum(H)_k of the state the records belong to
    double sumy = 0.0;
    for (int kk = 0; kk < a.k; ++kk) sumy += a.colsum_gw[kk] * a.hstat_in[ESPM_HS_ROWSUM + kk];
    a.hist_slot[ESPM_HI_SUMY] = sumy;
  }
  if (job >= NV) return;
  const bool is_sum = job < 4 + KP;
  const double v = chain_combine(scr, NV, job, is_sum);
  if (job == ESPM_HP_KL) {
    if (a.compute_loss) a.hist_slot[ESPM_HI_KLX] = (double)a.xscale * 0.6931471805599453 * v;
  } else if (job == ESPM_HP_REG) {
    a.hist_slot[ESPM_HI_REG] = v;
  } else if (job == ESPM_HP_LAP) {
    a.hist_slot[ESPM_HI_LAP] = v;
  } else if (job == ESPM_HP_BAD) {
    a.hist_slot[ESPM_HI_BAD] = v;
  } else if (is_sum) {
    if (a.hstat_out) a.hstat_out[ESPM_HS_ROWSUM + (job - ESPM_HP_ROWSUM)] = v;
  } else if (job == V_RELH) {
    if (a.have_prev) a.hist_slot[ESPM_HI_REL_H] = v;
  } else if (job == V_RELW) {
    if (v >= 0.0) a.hist_slot[ESPM_HI_REL_W] = v;
  } else {
    if (a.hstat_out) a.hstat_out[ESPM_HS_MAX + (job - V_MAX)] = v;
  }
}

}  // namespace espm
