// The W finish as ONE workgroup (the W step as a whole: mu_w_parts.hpp): register-resident for the sizes a workgroup's registers
// hold, general beyond.  A dictionary G that a many-workgroup form applies to goes to mu_w_dict.hip instead.
#include "mu_w_parts.hpp"

namespace espm {

// ---- W finish: one workgroup of 1024 threads --------------------------------------------------

// (WF_THREADS, WF_FEW_THREADS, WF_HALF_MAX_K, WF_GTA_MAX, WF_GTA_PAR: mu_w_plan.hpp, with the plan that chooses among the kernels below)

// Register-resident variant for M <= WF_ROWS * 1024 rows (and M * k <= WF_GTA_MAX when G is given): thread t
// owns rows t, t + 1024, ... of W and keeps their old / numerator / denominator / new entries in registers
// across the phases (no index division, no scratch traffic); the second stage of the slab reduction
// (sum over the `nsplit` partials, fixed order) is folded into the load of A; G^T A is formed by one wave
// per output entry and G W' reads W' from LDS.  Same arithmetic and the same global-stop bisection as
// w_finish_kernel below; only the data movement differs.
// One step of a packed butterfly sum over the lanes of a wave: of the first N values a lane keeps one half
// (the upper one when `up`) and adds the partner's copy of that half, which the partner sends instead of keeping.
template <int N>
__device__ __forceinline__ void butterfly_half(float (&v)[32], bool up, int off) {
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const float send = up ? v[j] : v[N / 2 + j];
    const float keep = up ? v[N / 2 + j] : v[j];
    v[j] = keep + __shfl_xor(send, off, 64);
  }
}

__device__ __forceinline__ float load_a(const WFinishArgs& a, int kk, int c) {
  return a.a[(size_t)kk * a.n_pad + c];
}

// 1 / x for the bisection's sum_c num_c / (nu + den_c): v_rcp_f64 and two Newton steps (a few ulp; an IEEE division is
// three times the instructions, and 10 of them per thread and step were what the one-workgroup W finish spent its time on)
__device__ __forceinline__ double rcp_f64(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

// NT threads: 1024 (16 waves, 128 registers each) or 512 (8 waves, 256 registers): the thread count that spills less wins -
// with G = identity and the simplex over W the 16-wave version kept 80 of its values in scratch memory and took 49 us, the
// 8-wave one takes 37 (tools/analysis/w_finish_clock.py); with a dictionary G the loops over its rows want the 16 waves.
// WF_ROWS rows of W per thread (its state stays in registers through the phases); CROWS channels per thread in the phase that
// forms G^T A with thread = channel (a dictionary G has few rows - W state for ONE row per thread - and many channels: sizing
// the W state by the channels spilled 245 registers at 8 components).
template <int KK, int WF_ROWS, int NT, int CROWS = WF_ROWS>
__global__ __launch_bounds__(NT) void w_finish_fast_kernel(const WFinishArgs a) {
  constexpr int KA = KK;  // per-thread arrays are sized by the real component count (k == KK)
  __shared__ double scratch[(NT / 64 + 1) * KP];
  __shared__ double bis[2][(NT / 64) * 2 * KA];   // per-wave partial sums (f, f') of the root finder, two alternating buffers
  __shared__ double s_lo[KA], s_hi[KA], s_mid[KA], s_dstar[KA], s_sum[KA];
  __shared__ double s_x[KA], s_root[KA], s_fder[KA], s_ad[KA], s_width[KA], s_u[KA];
  __shared__ int s_flag[KA];
  __shared__ unsigned long long s_mask[4];
  __shared__ int s_go;
  extern __shared__ __attribute__((aligned(16))) float dyn[];  // G given: [M*k] new W, [M*k] G^T A
  const int M = a.m > 0 ? a.m : a.n;
  const int k = a.k;
  const int MK = M * k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int SW = (KA + 3) / 4 * 4;   // stride of a row of W' in LDS: whole 16-byte quads (the rows of G W' read them as float4)
  float* s_w = dyn;
  float* s_gta = dyn + (size_t)M * SW;
  ESPM_PHASE_STAMP(0);
#ifdef ESPM_PHASE_CLOCK
  if (threadIdx.x == 0 && espm_phase_buf) espm_phase_buf[20] = (unsigned long long)clock64();   // shader clock ticks (against the 100 MHz stamps)
#endif

  float wn[WF_ROWS][KA];
#pragma unroll
  for (int r = 0; r < WF_ROWS; ++r)
#pragma unroll
    for (int kk = 0; kk < KA; ++kk) wn[r][kk] = 0.f;

  if (a.update_w) {
    if (KA <= 8 && a.g && a.g_t && MK <= WF_GTA_PAR) {   // (the packed sum below is laid out for 4 rows x 8 components)
      // G^T A with the association G^T (R H^T), updates.py:58-59, with every thread busy: thread = channel
      // (its k entries of A in registers), G^T rows read coalesced, the products of a wave summed across its lanes
      // and the per-wave partials by the workgroup.  s_part lives behind s_gta.
      float* s_part = s_gta + MK;  // [NT / 64][MK]
      float av[CROWS][KA];
#pragma unroll
      for (int r = 0; r < CROWS; ++r) {
        const int c = tid + r * NT;
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) av[r][kk] = (kk < k && c < a.n) ? load_a(a, kk, c) : 0.f;
      }
      // Batches of 4 rows of G^T: 32 (row, component) products per lane, summed over the 64 lanes by a packed
      // butterfly - in every step a lane hands the half of its values it does not keep to its partner - which
      // takes 32 cross-lane moves instead of 6 x 32 (the moves, on one CU, are what bounds this phase).
      constexpr int MB = 4, KB8 = 8;
      for (int m0 = 0; m0 < a.m; m0 += MB) {
        float gv[MB][CROWS];
#pragma unroll
        for (int b = 0; b < MB; ++b) {
          const int mm = m0 + b < a.m ? m0 + b : a.m - 1;
#pragma unroll
          for (int r = 0; r < CROWS; ++r) {
            const int c = tid + r * NT;
            gv[b][r] = c < a.n ? a.g_t[(size_t)mm * a.n_pad + c] : 0.f;
          }
        }
        float v[MB * KB8];
#pragma unroll
        for (int b = 0; b < MB; ++b)
#pragma unroll
          for (int kk = 0; kk < KB8; ++kk) {
            float t = 0.f;
            if (kk < KA) {
#pragma unroll
              for (int r = 0; r < CROWS; ++r) t = fmaf(gv[b][r], av[r][kk < KA ? kk : 0], t);
            }
            v[b * KB8 + kk] = t;
          }
        butterfly_half<32>(v, (lane & 32) != 0, 32);
        butterfly_half<16>(v, (lane & 16) != 0, 16);
        butterfly_half<8>(v, (lane & 8) != 0, 8);
        butterfly_half<4>(v, (lane & 4) != 0, 4);
        butterfly_half<2>(v, (lane & 2) != 0, 2);
        const float total = v[0] + __shfl_xor(v[0], 1, 64);
        const int idx = (lane >> 1) & 31, b = idx >> 3, kk = idx & 7;  // the (row, component) this lane pair ended up with
        if (!(lane & 1) && m0 + b < a.m && kk < k) s_part[wave * MK + (m0 + b) * k + kk] = total;
      }
      __syncthreads();
      for (int o = tid; o < MK; o += NT) {
        float t = 0.f;
        for (int w = 0; w < NT / 64; ++w) t += s_part[w * MK + o];
        s_gta[o] = t;
      }
      __syncthreads();
    } else if (a.g) {  // no transposed copy: one wave per (mm, kk), G read with a stride of m
      for (int o = wave; o < MK; o += NT / 64) {
        const int mm = o / k, kk = o - mm * k;
        float sacc = 0.f;
        for (int c = lane; c < a.n; c += 64) sacc = fmaf(a.g[(size_t)c * a.m + mm], load_a(a, kk, c), sacc);
        sacc = wave_sum(sacc);
        if (lane == 0) s_gta[o] = sacc;
      }
      __syncthreads();
    }
    ESPM_PHASE_STAMP(1);   // (instrumented build, tools/analysis/w_finish_clock.py) G^T A done
    float rs[KA];
#pragma unroll
    for (int kk = 0; kk < KA; ++kk) rs[kk] = kk < k ? (float)a.hstat[ESPM_HS_ROWSUM + kk] : 0.f;
    float wo[WF_ROWS][KA], nv[WF_ROWS][KA], dv[WF_ROWS][KA], pgrad[WF_ROWS][KA];
    bool in_set[WF_ROWS];
#pragma unroll
    for (int r = 0; r < WF_ROWS; ++r) {
      const int mm = tid + r * NT;
      in_set[r] = false;
#pragma unroll
      for (int kk = 0; kk < KA; ++kk) { wo[r][kk] = 0.f; nv[r][kk] = 0.f; dv[r][kk] = 1.f; pgrad[r][kk] = 0.f; }
      if (mm < M) {
        in_set[r] = !a.simplex_rows || a.simplex_rows[mm];
        const float cg = a.g ? a.colsum_g[mm] : 1.f;
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
          if (kk < k) {
            const float gta = a.g ? s_gta[mm * k + kk] : load_a(a, kk, mm);
            wo[r][kk] = a.w_old[mm * k + kk];
            nv[r][kk] = wo[r][kk] * gta;        // updates.py:59
            dv[r][kk] = cg * rs[kk];            // updates.py:60
            if (a.pg_gamma_w > 0.f) {           // projected gradient: W - (colsum(G) rowsum(H) - G^T A) / gamma, updates.py:353-362
              pgrad[r][kk] = dv[r][kk] - gta;
              nv[r][kk] = wo[r][kk] - pgrad[r][kk] / a.pg_gamma_w;
              dv[r][kk] = 1.f;
            } else if (a.breg_sr) {             // Bregman variant (G = identity), updates.py:41-48
              const float sr = a.xscale * a.breg_sr[mm];
              dv[r][kk] = (dv[r][kk] - gta) * wo[r][kk] + sr;
              nv[r][kk] = sr * wo[r][kk];
            }
          }
        }
      }
    }
    ESPM_PHASE_STAMP(10);   // loads, numerators, denominators
    if (a.simplex_w) {
      // Multipliers of the simplex over W, all components at once.  The reference bisects the bracket [a, b] of every
      // column with a GLOBAL stop rule (dicotomy.py:146-171): all columns stop at the first sweep t in which every column's
      // midpoint has |f| <= tol, so its nu is the t-th midpoint of the bisection path towards the root - accurate to tol
      // only, and W' inherits that (column sums 1 +- 1e-5).  Walking those ~40 sweeps on one CU was 90 us of a 260 us
      // iteration.  The same nu in ~5 evaluations of f instead of ~40:
      //   1. the ROOT by Newton in the shifted unknown delta = nu + d* (as the H-step's simplex_root): f is convex and
      //      decreasing, sum(num) bounds the root from the right (every e = den - d* >= 0), so the first step lands left of
      //      the root and the rest converges monotonically; safeguarded by the running bracket;
      //   2. the bisection path needs no sweeps once the root is known: the t-th midpoint towards a root at fraction u of
      //      the bracket is a + (b - a) (2 floor(u 2^(t-1)) + 1) / 2^t;
      //   3. the sweep the reference stops at: the first t with max_k |f_k(mid_t)| <= tol - decided from the linearisation
      //      f ~ f'(root) (mid - root) (its relative error is |mid - root| / delta ~ tol there), and by a real evaluation of
      //      f where the estimate is within 1 % of tol.
      // Thread kk < k OWNS component kk (bracket, iterate, decisions); the evaluation points travel through LDS (two
      // barriers per evaluation): per-thread copies of the state of all components cost more registers than a wave has.
      double cnt_l = 0.0;
#pragma unroll
      for (int r = 0; r < WF_ROWS; ++r) cnt_l += (tid + r * NT < M && in_set[r]) ? 1.0 : 0.0;
      const double rows = block_sum1(cnt_l, scratch);
      {  // per column: max(num/2 - den), max num, max(-den) (dicotomy.py:29-49); max(-den | num > 0), sum num
        double b1[KA], b2[KA], b3[KA];
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) { b1[kk] = -INFINITY; b2[kk] = 0.0; b3[kk] = -INFINITY; }
#pragma unroll
        for (int r = 0; r < WF_ROWS; ++r) {
          if (tid + r * NT < M && in_set[r]) {
#pragma unroll
            for (int kk = 0; kk < KA; ++kk) {
              if (kk < k) {
                const double nn = nv[r][kk], dd = dv[r][kk];
                if (nn > 0) b1[kk] = fmax(b1[kk], nn / 2 - dd);
                b2[kk] = fmax(b2[kk], nn);
                b3[kk] = fmax(b3[kk], -dd);
              }
            }
          }
        }
        block_reduce<KA, 0>(b1, scratch);
        block_reduce<KA, 0>(b2, scratch);
        block_reduce<KA, 0>(b3, scratch);
        if (tid == 0)
          for (int kk = 0; kk < k; ++kk) {
            s_lo[kk] = b1[kk];                          // a, dicotomy.py:29-43
            s_hi[kk] = rows * b2[kk] / 0.5 + b3[kk];    // b, dicotomy.py:49
          }
      }
      {
        double b4[KA], b5[KA];
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) { b4[kk] = -INFINITY; b5[kk] = 0.0; }
#pragma unroll
        for (int r = 0; r < WF_ROWS; ++r) {
          if (tid + r * NT < M && in_set[r]) {
#pragma unroll
            for (int kk = 0; kk < KA; ++kk) {
              if (kk < k && nv[r][kk] > 0.f) {
                b4[kk] = fmax(b4[kk], -(double)dv[r][kk]);
                b5[kk] += (double)nv[r][kk];
              }
            }
          }
        }
        block_reduce<KA, 0>(b4, scratch);
        block_reduce<KA, KA>(b5, scratch);
        if (tid == 0)
          for (int kk = 0; kk < k; ++kk) {
            s_dstar[kk] = b5[kk] > 0.0 ? -b4[kk] : 0.0;   // d* = min{den : num > 0}: the last pole of f is at nu = -d*
            s_sum[kk] = b5[kk];
          }
      }
      __syncthreads();
      constexpr int NWV = NT / 64;
      const double tol = (double)a.tol;
      // owner state (threads kk < k); a column without a positive numerator has no multiplier (dicotomy.py:19)
      const bool owner = tid < k;
      const bool solve = owner && s_sum[owner ? tid : 0] > 0.0 && s_sum[owner ? tid : 0] < INFINITY;
      double o_x = 1.0, o_lo = 0.0, o_hi = 1.0, o_dxold = 1.0, o_fder = 0.0;
      bool o_done = true;
      if (owner) {
        const double dstar = s_dstar[tid];
        if (solve) {
          o_lo = fmax(s_lo[tid] + dstar, 0.0);
          o_hi = s_hi[tid] + dstar;
          o_x = fmin(fmax(s_sum[tid], o_lo), o_hi);
          o_dxold = o_hi - o_lo;
          o_done = false;
        }
        s_x[tid] = o_x;
        s_flag[tid] = o_done ? 1 : 0;
      }
      __syncthreads();
      ESPM_PHASE_STAMP(2);   // numerators, denominators, bracket
      int evals = 0;
      // per-wave partial sums of f_kk and f_kk' at delta = s_x[kk] into bis[evals & 1]; ends with a barrier
      auto evaluate = [&]() {
        double* sc = bis[evals & 1];
        ++evals;
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
          double f = 0.0, fp = 0.0;
          if (kk < k) {
            const double at = s_x[kk] - s_dstar[kk];   // (delta + den - d*: den - d* >= 0 is exact in fp64 for fp32 inputs of one scale)
#pragma unroll
            for (int r = 0; r < WF_ROWS; ++r) {
              if (tid + r * NT < M && in_set[r]) {
                const double inv = rcp_f64(at + (double)dv[r][kk]);
                const double t = nv[r][kk] > 0.f ? (double)nv[r][kk] * inv : 0.0;
                if (t > (double)a.log_shift) {
                  f += t;
                  fp -= t * inv;
                } else {
                  f += (double)a.log_shift;
                }
              }
            }
          }
          f = wave_sum(f);
          fp = wave_sum(fp);
          if (lane == 0) {
            sc[wave * 2 * KA + kk] = f;
            sc[wave * 2 * KA + KA + kk] = fp;
          }
        }
        __syncthreads();
        return sc;
      };
      auto combine = [&](const double* sc, int kk, double& fs, double& fps) {   // wave order: deterministic
        fs = sc[kk];
        fps = sc[KA + kk];
        for (int w = 1; w < NWV; ++w) {
          fs += sc[w * 2 * KA + kk];
          fps += sc[w * 2 * KA + KA + kk];
        }
        fs -= 1.0;
      };
      for (int it = 0; it < 100; ++it) {   // 1. the roots
        const double* sc = evaluate();
        if (owner && !o_done) {
          double fs, fps;
          combine(sc, tid, fs, fps);
          o_fder = fps;
          if (fabs(fs) <= 1e-11) {
            o_done = true;
          } else {
            if (fs > 0) o_lo = o_x; else o_hi = o_x;
            double dx = fps < 0 ? -fs / fps : 0.0;
            double xn = o_x + dx;
            if (!(fps < 0) || !(xn > o_lo && xn < o_hi) || fabs(dx) > 0.5 * fabs(o_dxold)) {
              dx = (o_hi - o_lo) / 2;
              xn = o_lo + dx;
            }
            o_dxold = dx;
            if (xn == o_x || fabs(dx) <= 1e-15 * fabs(o_x)) o_done = true;
            o_x = xn;
          }
          s_x[tid] = o_x;
          s_flag[tid] = o_done ? 1 : 0;
        }
        __syncthreads();
        bool all_done = true;
        for (int kk = 0; kk < k; ++kk) all_done = all_done && s_flag[kk] != 0;
        if (all_done) break;
      }
      // 2., 3. the reference's sweep count and its midpoints (in delta: a + d* + (b - a) frac)
      if (owner) {
        const double ad = s_lo[tid] + s_dstar[tid], width = s_hi[tid] - s_lo[tid];
        s_root[tid] = o_x;
        s_fder[tid] = solve ? o_fder : 0.0;
        s_ad[tid] = ad;
        s_width[tid] = width;
        s_u[tid] = solve ? fmin(fmax((o_x - ad) / width, 0.0), 1.0) : 0.5;
      }
      __syncthreads();
      // midpoint of sweep t (the first midpoint is t = 1) on the way to a root at fraction u of the bracket, as a fraction
      auto mid_frac = [](double uu, int t) {
        const double scale = ldexp(1.0, t - 1);
        const double cell = fmin(floor(uu * scale), scale - 1.0);
        return ldexp(2.0 * cell + 1.0, -t);
      };
      ESPM_PHASE_STAMP(3);   // roots found
#ifdef ESPM_PHASE_CLOCK
      if (threadIdx.x == 0 && espm_phase_buf) espm_phase_buf[8] = (unsigned long long)evals;
#endif
      // the sweeps are independent given the roots: lane l of wave 0 looks at sweeps l + 1 and l + 65 (dicotomy.py:152: at
      // most maxit = 100 sweeps after the first midpoint); two bit masks - "certainly stops here", "within 1 % of tol"
      if (wave == 0) {
        for (int hf = 0; hf < 2; ++hf) {
          const int t = 1 + lane + 64 * hf;
          double est = 0.0;
          for (int kk = 0; kk < k; ++kk)
            est = fmax(est, fabs(s_fder[kk] * ((s_ad[kk] + s_width[kk] * mid_frac(s_u[kk], t)) - s_root[kk])));
          const bool certain = t <= 101 && (est <= 0.99 * tol || t == 101);
          const bool band = t <= 101 && !certain && est <= 1.01 * tol;
          const unsigned long long mc = __ballot(certain), mb = __ballot(band);
          if (lane == 0) {
            s_mask[hf] = mc;
            s_mask[2 + hf] = mb;
          }
        }
      }
      __syncthreads();
      unsigned long long mc[2] = {s_mask[0], s_mask[1]}, mb[2] = {s_mask[2], s_mask[3]};
      int t_stop = 101;
      for (;;) {   // (uniform: every thread reads the same masks and the same sums)
        const unsigned long long w0 = mc[0] | mb[0], w1 = mc[1] | mb[1];
        if (!w0 && !w1) break;
        const int hf = w0 ? 0 : 1;
        const int bit = __ffsll((long long)(hf ? w1 : w0)) - 1;
        const int t = 1 + bit + 64 * hf;
        if ((mc[hf] >> bit) & 1ull) { t_stop = t; break; }
        if (owner) s_x[tid] = s_ad[tid] + s_width[tid] * mid_frac(s_u[tid], t);
        __syncthreads();
        const double* sc = evaluate();
        double worst = 0.0;
        for (int kk = 0; kk < k; ++kk) {
          double fs, fps;
          combine(sc, kk, fs, fps);
          if (s_fder[kk] != 0.0) worst = fmax(worst, fabs(fs));
        }
        if (worst <= tol) { t_stop = t; break; }
        mb[hf] &= ~(1ull << bit);
      }
      if (owner) s_mid[tid] = solve ? s_ad[tid] + s_width[tid] * mid_frac(s_u[tid], t_stop) : s_dstar[tid];   // delta = nu + d* (no multiplier: nu = 0)
      __syncthreads();
    }
    ESPM_PHASE_STAMP(4);   // the sweep the reference stops at
#ifdef ESPM_PHASE_CLOCK
    if (a.simplex_w && threadIdx.x == 0 && espm_phase_buf) espm_phase_buf[9] = 1000ull;   // (marks a simplex call)
#endif
    // W' = max(num / (den + nu), eps), fixed entries (updates.py:70-76); rel_W (base.py:323)
    double sum_l = 0.0;
#pragma unroll
    for (int r = 0; r < WF_ROWS; ++r) {
      const int mm = tid + r * NT;
      if (mm < M) {
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
          if (kk < k) {
            float den = dv[r][kk];
            if (a.simplex_w && in_set[r]) den = (float)(((double)den - s_dstar[kk]) + s_mid[kk]);
            float v = fmaxf(nv[r][kk] / den, a.log_shift);
            if (a.fixed_w) {
              const float fx = a.fixed_w[mm * k + kk];
              if (fx >= 0.f) v = fx;
            }
            wn[r][kk] = v;
            a.w_new[mm * k + kk] = v;
            if (a.g) s_w[mm * SW + kk] = v;
            sum_l += (double)v;
          }
        }
      }
    }
    const double mean_w = block_sum1(sum_l, scratch) / (double)MK;
    double rel_l = 0.0;
#pragma unroll
    for (int r = 0; r < WF_ROWS; ++r) {
      if (tid + r * NT < M) {
#pragma unroll
        for (int kk = 0; kk < KA; ++kk)
          if (kk < k)
            rel_l = fmax(rel_l, fabs((double)wn[r][kk] - (double)wo[r][kk]) / ((double)wn[r][kk] + (double)a.rel_tol * mean_w));
      }
    }
    const double rel_w = block_max1(rel_l, scratch);
    if (tid == 0 && a.hist_slot) a.hist_slot[ESPM_HI_REL_W] = rel_w;
    if (a.pg_q) {  // (uniform) the projected gradient's linesearch term sum <W' - W, grad> + gamma ||W' - W||^2
      double q_l = 0.0;
#pragma unroll
      for (int r = 0; r < WF_ROWS; ++r) {
        if (tid + r * NT < M) {
#pragma unroll
          for (int kk = 0; kk < KA; ++kk)
            if (kk < k) {
              const double dw = (double)wn[r][kk] - (double)wo[r][kk];
              q_l += dw * (double)pgrad[r][kk] + (double)a.pg_gamma_w * dw * dw;
            }
        }
      }
      const double q_w = block_sum1(q_l, scratch);
      if (tid == 0) *a.pg_q = q_w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < WF_ROWS; ++r) {
      const int mm = tid + r * NT;
      if (mm < M) {
#pragma unroll
        for (int kk = 0; kk < KA; ++kk) {
          if (kk < k) {
            wn[r][kk] = a.w_new[mm * k + kk];
            if (a.g) s_w[mm * SW + kk] = wn[r][kk];
          }
        }
      }
    }
    __syncthreads();
  }

  ESPM_PHASE_STAMP(5);   // W', rel_W
  // GW = G W' (updates.py:107 of the next half step), stored / xscale with a positive floor
  double cs[KA];
#pragma unroll
  for (int kk = 0; kk < KA; ++kk) cs[kk] = 0.0;
  const float inv_scale = 1.f / a.xscale;
  auto emit_row = [&](int c, const float (&src)[KA]) {
    float row[espm::KP];
#pragma unroll
    for (int kk = 0; kk < espm::KP; ++kk) row[kk] = 0.f;
    if (c >= a.n) {
#pragma unroll
      for (int kk = 0; kk < KA; ++kk) row[kk] = 1.f;  // padding channels: X = 0 there
    } else {
#pragma unroll
      for (int kk = 0; kk < KA; ++kk) {
        const float v = fmaxf(src[kk], a.gw_floor);
        cs[kk] += (double)v;
        row[kk] = v * inv_scale;
      }
    }
    if (c < a.n_pad) {
      espm::store_row_kp(a.gw_s + (size_t)c * espm::KP, row);
    }
  };
  const int n_rows = a.n_pad;
  if (a.g) {
    for (int c = tid; c < n_rows; c += NT) {
      float row[KA];
#pragma unroll
      for (int kk = 0; kk < KA; ++kk) row[kk] = 0.f;
      if (c < a.n) {
        constexpr int MB = 8;  // entries of the G row requested together
        for (int m0 = 0; m0 < a.m; m0 += MB) {
          float gv[MB];
#pragma unroll
          for (int b = 0; b < MB; ++b) {
            const int mm = m0 + b < a.m ? m0 + b : a.m - 1;
            gv[b] = a.g_t ? a.g_t[(size_t)mm * a.n_pad + c] : a.g[(size_t)c * a.m + mm];
          }
#pragma unroll
          for (int b = 0; b < MB; ++b) {
            if (m0 + b < a.m) {
              // a row of W' as aligned 16-byte reads (one 4-byte read per multiply-add was 16 us of this kernel's 36 at C5)
              const float4* wr = reinterpret_cast<const float4*>(s_w + (size_t)(m0 + b) * SW);
#pragma unroll
              for (int q4 = 0; q4 < SW / 4; ++q4) {
                const float4 w4 = wr[q4];
                const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
                  if (4 * q4 + i < KA) row[4 * q4 + i] = fmaf(gv[b], wv[i], row[4 * q4 + i]);
              }
            }
          }
        }
      }
      emit_row(c, row);
    }
  } else {  // G = identity: row c of G W' is row c of W', already in this thread's registers
#pragma unroll
    for (int r = 0; r < WF_ROWS; ++r) {
      const int c = tid + r * NT;
      if (c < n_rows) emit_row(c, wn[r]);
    }
  }
  block_reduce<KA, KA>(cs, scratch);
  if (tid == 0)
    for (int kk = 0; kk < espm::KP; ++kk) a.colsum_gw[kk] = kk < KA ? cs[kk] : 0.0;
  ESPM_PHASE_STAMP(6);   // rows of G W', column sums
#ifdef ESPM_PHASE_CLOCK
  if (threadIdx.x == 0 && espm_phase_buf) espm_phase_buf[21] = (unsigned long long)clock64();
#endif
}

__global__ __launch_bounds__(WF_THREADS) void w_finish_kernel(const WFinishArgs a) {
  __shared__ double scratch[(WF_THREADS / 64 + 1) * 2 * KP];
  __shared__ double s_lo[KP], s_hi[KP], s_mid[KP], s_f[KP];
  __shared__ int s_go;
  const int M = a.m > 0 ? a.m : a.n;
  const int k = a.k;
  const int tid = threadIdx.x;
  float* numv = a.scratch;
  float* denv = a.scratch + (size_t)M * k;

  if (a.update_w) {
    // numerator W * (G^T A) and denominator colsum(G) rowsum(H)^T, updates.py:58-60
    for (int e = tid; e < M * k; e += WF_THREADS) {
      const int mm = e / k, kk = e - mm * k;
      float gta;
      if (a.g) {
        float s = 0.f;
        for (int c = 0; c < a.n; ++c) s = fmaf(a.g[(size_t)c * a.m + mm], load_a(a, kk, c), s);
        gta = s;
      } else {
        gta = load_a(a, kk, mm);
      }
      const float wo = a.w_old[e];
      float nvv = wo * gta;
      float dvv = (a.g ? a.colsum_g[mm] : 1.f) * (float)a.hstat[ESPM_HS_ROWSUM + kk];
      if (a.pg_gamma_w > 0.f) {           // projected gradient: W - (colsum(G) rowsum(H) - G^T A) / gamma, updates.py:353-362 (as w_finish_fast_kernel)
        const float pgr = dvv - gta;
        nvv = wo - pgr / a.pg_gamma_w;
        dvv = pgr;                        // (the denominator is 1: its slot carries the gradient for the linesearch term below)
      } else if (a.breg_sr) {             // Bregman variant (G = identity), updates.py:41-48
        const float sr = a.xscale * a.breg_sr[mm];
        dvv = (dvv - gta) * wo + sr;
        nvv = sr * wo;
      }
      numv[e] = nvv;
      denv[e] = dvv;
    }
    __syncthreads();

    if (a.simplex_w) {
      // bracket of dicotomy.py:29-49 per column kk over the constrained rows
      double cnt_l = 0.0;
      for (int mm = tid; mm < M; mm += WF_THREADS) cnt_l += (!a.simplex_rows || a.simplex_rows[mm]) ? 1.0 : 0.0;
      const double rows = block_sum1(cnt_l, scratch);
      for (int kk = 0; kk < k; ++kk) {
        double lo = -INFINITY, nmax = 0.0, dmin_neg = -INFINITY;
        for (int mm = tid; mm < M; mm += WF_THREADS) {
          if (a.simplex_rows && !a.simplex_rows[mm]) continue;
          const double nn = numv[mm * k + kk], dd = denv[mm * k + kk];
          if (nn > 0) lo = fmax(lo, nn / 2 - dd);
          nmax = fmax(nmax, nn);
          dmin_neg = fmax(dmin_neg, -dd);
        }
        lo = block_max1(lo, scratch);
        nmax = block_max1(nmax, scratch);
        dmin_neg = block_max1(dmin_neg, scratch);
        if (tid == 0) {
          s_lo[kk] = lo;
          s_hi[kk] = rows * nmax / 0.5 + dmin_neg;
        }
      }
      __syncthreads();
      // bisection with the reference's global stop rule, dicotomy.py:146-171
      for (int it = 0; it <= 100; ++it) {
        if (tid < k) s_mid[tid] = (s_lo[tid] + s_hi[tid]) / 2;
        __syncthreads();
        double f[KP];
#pragma unroll
        for (int kk = 0; kk < KP; ++kk) f[kk] = 0.0;
        for (int mm = tid; mm < M; mm += WF_THREADS) {
          if (a.simplex_rows && !a.simplex_rows[mm]) continue;
#pragma unroll
          for (int kk = 0; kk < KP; ++kk)
            if (kk < k)
              f[kk] += fmax((double)numv[mm * k + kk] / (s_mid[kk] + (double)denv[mm * k + kk]), (double)a.log_shift);
        }
        block_reduce<KP, KP>(f, scratch);
        if (tid == 0) {
          double worst = 0.0;
          for (int kk = 0; kk < k; ++kk) {
            s_f[kk] = f[kk] - 1.0;
            worst = fmax(worst, fabs(s_f[kk]));
          }
          s_go = (worst > (double)a.tol) && (it < 100);
          if (s_go) {
            for (int kk = 0; kk < k; ++kk) {
              if (s_f[kk] <= 0.0) s_hi[kk] = s_mid[kk]; else s_lo[kk] = s_mid[kk];
            }
          }
        }
        __syncthreads();
        if (!s_go) break;
      }
    }

    // W' = max(num / (den + nu), eps), fixed entries, updates.py:70-76
    double sum_l = 0.0, q_l = 0.0;
    const bool pg = a.pg_gamma_w > 0.f;   // (never with the simplex over W: espm_mu's state check)
    for (int e = tid; e < M * k; e += WF_THREADS) {
      const int mm = e / k, kk = e - mm * k;
      float den = pg ? 1.f : denv[e];
      if (a.simplex_w && (!a.simplex_rows || a.simplex_rows[mm])) den += (float)s_mid[kk];
      float wn = fmaxf(numv[e] / den, a.log_shift);
      if (a.fixed_w && a.fixed_w[e] >= 0.f) wn = a.fixed_w[e];
      a.w_new[e] = wn;
      sum_l += (double)wn;
      if (pg) {   // the linesearch term sum <W' - W, grad> + gamma ||W' - W||^2
        const double dw = (double)wn - (double)a.w_old[e];
        q_l += dw * (double)denv[e] + (double)a.pg_gamma_w * dw * dw;
      }
    }
    if (a.pg_q) {   // (uniform)
      const double q_w = block_sum1(q_l, scratch);
      if (tid == 0) *a.pg_q = q_w;
    }
    const double mean_w = block_sum1(sum_l, scratch) / ((double)M * k);
    double rel_l = 0.0;
    for (int e = tid; e < M * k; e += WF_THREADS) {
      const double wn = a.w_new[e], wo = a.w_old[e];
      rel_l = fmax(rel_l, fabs(wn - wo) / (wn + (double)a.rel_tol * mean_w));  // base.py:323
    }
    const double rel_w = block_max1(rel_l, scratch);
    if (tid == 0 && a.hist_slot) a.hist_slot[ESPM_HI_REL_W] = rel_w;
  }

  // GW = G W' (updates.py:107 of the next half step), stored / xscale with a positive floor
  const float* w = a.w_new;
  double cs[KP];
#pragma unroll
  for (int kk = 0; kk < KP; ++kk) cs[kk] = 0.0;
  const float inv_scale = 1.f / a.xscale;
  for (int c = tid; c < a.n_pad; c += WF_THREADS) {
    float row[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      float v = 0.f;
      if (kk < k) {
        if (c >= a.n) {
          v = 1.f;  // padding channels: X = 0 there, any positive value keeps X / Y = 0
        } else {
          if (a.g) {
            for (int mm = 0; mm < a.m; ++mm) v = fmaf(a.g[(size_t)c * a.m + mm], w[mm * k + kk], v);
          } else {
            v = w[c * k + kk];
          }
          v = fmaxf(v, a.gw_floor);
          cs[kk] += (double)v;
          v *= inv_scale;
        }
      }
      row[kk] = v;
    }
    store_row_kp(a.gw_s + (size_t)c * KP, row);
  }
  block_reduce<KP, KP>(cs, scratch);
  if (tid == 0)
    for (int kk = 0; kk < KP; ++kk) a.colsum_gw[kk] = cs[kk];
}

// the instance w_finish_fast_kernel<KK, rows, NT, crows> that the plan names (plan_w_finish, mu_w_plan.hpp, has chosen among those built)
template <int KK, int NT>
static void launch_fast(const WFinishPlan& pl, const WFinishArgs& args, hipStream_t stream) {
  const size_t lds = pl.lds;
  if (pl.crows != pl.rows) {   // dictionary G with at most NT rows: W state of one row per thread, 2 or 4 channels per thread for G^T A
    if (pl.crows == 2)
      hipLaunchKernelGGL((w_finish_fast_kernel<KK, 1, NT, 2>), dim3(1), dim3(NT), lds, stream, args);
    else
      hipLaunchKernelGGL((w_finish_fast_kernel<KK, 1, NT, 4>), dim3(1), dim3(NT), lds, stream, args);
    return;
  }
  // (NT == 256 exists only in the A/B build with -DESPM_WF_FEW_THREADS=256, and so does its instance of 8 rows per thread - 4 waves at
  //  2048 channels; the product's plan never names either)
  if constexpr (NT == 256) {
    if (pl.rows == 8) {
      hipLaunchKernelGGL((w_finish_fast_kernel<KK, 8, NT>), dim3(1), dim3(NT), lds, stream, args);
      return;
    }
  }
  if (pl.rows == 1)
    hipLaunchKernelGGL((w_finish_fast_kernel<KK, 1, NT>), dim3(1), dim3(NT), lds, stream, args);
  else if (pl.rows == 2)
    hipLaunchKernelGGL((w_finish_fast_kernel<KK, 2, NT>), dim3(1), dim3(NT), lds, stream, args);
  else
    hipLaunchKernelGGL((w_finish_fast_kernel<KK, 4, NT>), dim3(1), dim3(NT), lds, stream, args);
}

// (which form, and which instance: plan_w_finish, mu_w_plan.hpp)
int launch_w_finish(const WFinishArgs& args, hipStream_t stream) {
  const WFinishPlan pl = plan_w_finish(args);
  switch (pl.form) {
    case ESPM_W_FORM_DICT_COLUMNS:
    case ESPM_W_FORM_DICT_TWO_LAUNCH: return launch_w_dict_finish(args, pl.form, stream);
    case ESPM_W_FORM_ONE_WG_GENERAL:
      // (w_finish_kernel keeps numerators and denominators of an update in the workspace; the register-resident finishes need none,
      //  which is how a state without one gets here at all - mu_api.hip: w_form_ahead)
      ESPM_REQUIRE(!args.update_w || args.scratch, "w_finish: the general one-workgroup W update of %d x %d entries needs w_scratch", args.m > 0 ? args.m : args.n, args.k);
      hipLaunchKernelGGL(w_finish_kernel, dim3(1), dim3(WF_THREADS), 0, stream, args);
      break;
    default:
      switch (args.k) {
#if ESPM_KP <= 16
#define ESPM_X(KK)                                                              \
  case KK:                                                                      \
    if (pl.nt == WF_FEW_THREADS) launch_fast<KK, (KK <= WF_HALF_MAX_K ? WF_FEW_THREADS : WF_THREADS)>(pl, args, stream); \
    else launch_fast<KK, WF_THREADS>(pl, args, stream);                  \
    break;
        ESPM_K_CASES(ESPM_X)
#undef ESPM_X
#endif
        default: return set_error(ESPM_EUNSUPPORTED, "w_finish: k=%d not built", args.k);
      }
  }
  return check_hip(hipGetLastError(), "w_finish launch");
}

}  // namespace espm

#ifdef ESPM_PHASE_CLOCK
// debug build only (tools/analysis/w_finish_clock.py): where this file's kernels write their phase stamps
extern "C" int espm_debug_phase_buffer_w(void* dev_ptr) {
  unsigned long long* p = static_cast<unsigned long long*>(dev_ptr);
  return espm::check_hip(hipMemcpyToSymbol(HIP_SYMBOL(espm::espm_phase_buf), &p, sizeof(p)), "phase buffer (w)");
}
#endif
