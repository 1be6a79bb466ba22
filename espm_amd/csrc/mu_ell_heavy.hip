// Heavy elements of the sparse count store (include/espm_mu.h, espm_mu_state.ell_hv_*): integer counts 256 .. 2^24, kept outside the
// 16-bit lists with their exact values.  The builder's two steps (count and zero them in the 8-bit copies, then compact them
// pixel-major) and the two passes of an iteration: before the H update the heavy numerators and loss terms of the pixels that hold
// such elements, after the W accumulation their part of R H'^T added to the slabs of their W blocks and their loss to the first
// H-step record.  No float atomics: every output entry has one writer, every sum runs in a fixed order.
#include "mu_common.hpp"

namespace espm {

// ---- builder ---------------------------------------------------------------------------------------------------------------
// One wave per pixel, lanes over the channels; the heavy elements are those >= ESPM_ELL_HEAVY_MIN (the caller has checked that X
// holds integers <= ESPM_ELL_HEAVY_MAX).
template <typename ST>
__device__ __forceinline__ float hv_src(const ST* x, int layout, int64_t ld, int c, int j) {
  return (float)(layout == ESPM_LAYOUT_CM ? x[(int64_t)c * ld + j] : x[(int64_t)j * ld + c]);
}

template <typename ST>
__global__ __launch_bounds__(256) void ell_hv_count_kernel(const ST* __restrict__ x, int layout, int64_t ld, int n, int p, int n_pad,
                                                           int n_cm, uint8_t* __restrict__ x8, uint8_t* __restrict__ x8c,
                                                           int32_t* __restrict__ cnt_px) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;   // (whole waves)
  int cnt = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int c = c0 + lane;
    const bool heavy = c < n && hv_src(x, layout, ld, c, j) >= (float)ESPM_ELL_HEAVY_MIN;
    if (heavy) {
      x8[(size_t)j * n_pad + c] = 0;
      if (x8c) x8c[((size_t)(j / ESPM_PPAD) * n_cm + c) * ESPM_PPAD + (j % ESPM_PPAD)] = 0;
    }
    cnt += __popcll(__ballot(heavy));
  }
  if (lane == 0) cnt_px[j] = cnt;
}

template <typename ST>
__global__ __launch_bounds__(256) void ell_hv_fill_kernel(const ST* __restrict__ x, int layout, int64_t ld, int n, int p,
                                                          const int32_t* __restrict__ px_off, int32_t* __restrict__ hv_pm) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= p) return;
  int base = px_off[j];
  const int end = px_off[j + 1];
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int c0 = 0; c0 < n && base < end; c0 += 64) {
    const int c = c0 + lane;
    const float v = c < n ? hv_src(x, layout, ld, c, j) : 0.f;
    const bool heavy = v >= (float)ESPM_ELL_HEAVY_MIN;
    const unsigned long long m = __ballot(heavy);
    if (heavy) {
      const int at = base + __popcll(m & below);
      if (at < end) {   // (the count pass found exactly these; a guard all the same)
        hv_pm[2 * (size_t)at] = c;
        hv_pm[2 * (size_t)at + 1] = (int32_t)v;
      }
    }
    base += __popcll(m);
  }
}

int launch_ell_hv_count(const void* x, int src_dtype, int layout, int64_t ld, int n, int p, int n_pad, int n_cm, uint8_t* x8, uint8_t* x8c,
                        int32_t* cnt_px, hipStream_t stream) {
  const dim3 grid((p + 3) / 4);
  if (src_dtype == ESPM_SRC_F64)
    hipLaunchKernelGGL(ell_hv_count_kernel<double>, grid, dim3(256), 0, stream, static_cast<const double*>(x), layout, ld, n, p, n_pad, n_cm,
                       x8, x8c, cnt_px);
  else
    hipLaunchKernelGGL(ell_hv_count_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float*>(x), layout, ld, n, p, n_pad, n_cm,
                       x8, x8c, cnt_px);
  return check_hip(hipGetLastError(), "ell_heavy_count launch");
}

int launch_ell_hv_fill(const void* x, int src_dtype, int layout, int64_t ld, int n, int p, const int32_t* px_off, int32_t* hv_pm,
                       hipStream_t stream) {
  const dim3 grid((p + 3) / 4);
  if (src_dtype == ESPM_SRC_F64)
    hipLaunchKernelGGL(ell_hv_fill_kernel<double>, grid, dim3(256), 0, stream, static_cast<const double*>(x), layout, ld, n, p, px_off, hv_pm);
  else
    hipLaunchKernelGGL(ell_hv_fill_kernel<float>, grid, dim3(256), 0, stream, static_cast<const float*>(x), layout, ld, n, p, px_off, hv_pm);
  return check_hip(hipGetLastError(), "ell_heavy_fill launch");
}

// ---- iteration -------------------------------------------------------------------------------------------------------------
// Before the H update of state (GW, H): one thread per pixel with heavy elements.  Numerator sum_c x GW_c / Y_c (Y_c = GW_c . H_pixel,
// stored units like the lists' partial numerators: the epilogue scales it by xscale) into column col0 + i of the fill table, and the
// pixel's loss term (its lists' constant plus sum x log2(x / Y), fp64), summed over the 256 pixels of the workgroup in a fixed order
// into kl[blockIdx.x].
__global__ __launch_bounds__(256) void ell_hv_h_kernel(const float* __restrict__ gw_s, const float* __restrict__ h_in, int p_pad, int k,
                                                       const int32_t* __restrict__ px, const int32_t* __restrict__ off,
                                                       const int32_t* __restrict__ pm, const float* __restrict__ klc, int npx,
                                                       float* __restrict__ num, int ld, int col0, double* __restrict__ kl) {
  __shared__ double red[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool own = i < npx;
  const int j = own ? px[i] : 0;
  float h[KP], s[KP];
#pragma unroll
  for (int kk = 0; kk < KP; ++kk) {
    h[kk] = (own && kk < k) ? h_in[(size_t)kk * p_pad + j] : 0.f;
    s[kk] = 0.f;
  }
  double l = own ? (double)klc[i] : 0.0;
  for (int e = own ? off[i] : 0, e1 = own ? off[i + 1] : 0; e < e1; ++e) {
    const int c = pm[2 * (size_t)e];
    const float xv = (float)pm[2 * (size_t)e + 1];
    float g[KP], y = 0.f;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      g[kk] = gw_s[(size_t)c * KP + kk];
      if (kk < k) y = fmaf(g[kk], h[kk], y);
    }
    const float r = xv / y;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) s[kk] = fmaf(g[kk], r, s[kk]);
    l += (double)xv * log2((double)xv / (double)y);
  }
#pragma unroll
  for (int kk = 0; kk < KP; ++kk)
    if (own && kk < k) num[(size_t)kk * ld + col0 + i] = s[kk];
  red[threadIdx.x] = l;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) kl[blockIdx.x] = red[0];
}

// After the W accumulation with H' (h: entry (kk, j) at kk * hs_k + j * hs_p - h[1 - src] or h_t): one thread per (W block, channel)
// group adds sum_j x / Y'_j H'_j to a_slab[block][:, channel], the entries it alone writes.  With the loss, one more workgroup adds
// the sum of the nkl partial sums kl (fixed order) to the KL field of the first H-step record.
__global__ __launch_bounds__(256) void ell_hv_post_kernel(const float* __restrict__ gw_s, const float* __restrict__ h, size_t hs_k, size_t hs_p,
                                                          int k, int pb, int n_pad, const int32_t* __restrict__ grp,
                                                          const int32_t* __restrict__ goff, const int32_t* __restrict__ wm, int ngrp, int wblocks,
                                                          float* __restrict__ a_slab, const double* __restrict__ kl, int nkl,
                                                          double* __restrict__ hpart) {
  if ((int)blockIdx.x == wblocks) {   // the loss workgroup
    __shared__ double red[256];
    double t = 0.0;
    for (int i = threadIdx.x; i < nkl; i += 256) t += kl[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    static_assert(ESPM_HP_KL == 0, "field-major records: field KL of block 0 is hpart[0]");
    if (threadIdx.x == 0) hpart[0] += red[0];
    return;
  }
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= ngrp) return;
  const int c = grp[g];
  const int e0 = goff[g], e1 = goff[g + 1];
  const int b = wm[2 * (size_t)e0] / pb;
  float gv[KP], acc[KP];
#pragma unroll
  for (int kk = 0; kk < KP; ++kk) {
    gv[kk] = gw_s[(size_t)c * KP + kk];
    acc[kk] = 0.f;
  }
  for (int e = e0; e < e1; ++e) {
    const int j = wm[2 * (size_t)e];
    const float xv = (float)wm[2 * (size_t)e + 1];
    float hv[KP], y = 0.f;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      hv[kk] = kk < k ? h[kk * hs_k + (size_t)j * hs_p] : 0.f;
      y = fmaf(gv[kk], hv[kk], y);
    }
    const float r = xv / y;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) acc[kk] = fmaf(r, hv[kk], acc[kk]);
  }
#pragma unroll
  for (int kk = 0; kk < KP; ++kk)
    if (kk < k) a_slab[((size_t)b * k + kk) * n_pad + c] += acc[kk];
}

int launch_ell_hv_h(const espm_mu_state* st, int src, int ld, hipStream_t stream) {
  const int npx = st->ell_hv_npx;
  hipLaunchKernelGGL(ell_hv_h_kernel, dim3((npx + 255) / 256), dim3(256), 0, stream, st->gw_s, st->h[src], st->p_pad, st->k, st->ell_hv_px,
                     st->ell_hv_px_off, st->ell_hv_pm, st->ell_hv_klc, npx, st->ell_fill_num, ld, st->ell_fill_n, st->ell_hv_kl);
  return check_hip(hipGetLastError(), "ell_heavy_h launch");
}

int launch_ell_hv_post(const espm_mu_state* st, const float* h, size_t hs_k, size_t hs_p, bool w, bool loss, hipStream_t stream) {
  const int wblocks = w ? (st->ell_hv_ngrp + 255) / 256 : 0;
  const int blocks = wblocks + (loss ? 1 : 0);
  if (blocks == 0) return ESPM_OK;
  const int pb = st->ell_pb > 0 ? st->ell_pb : ESPM_ELL_PB;
  hipLaunchKernelGGL(ell_hv_post_kernel, dim3(blocks), dim3(256), 0, stream, st->gw_s, h, hs_k, hs_p, st->k, pb, st->n_pad, st->ell_hv_grp,
                     st->ell_hv_grp_off, st->ell_hv_wm, st->ell_hv_ngrp, wblocks, st->a_slab, st->ell_hv_kl, (st->ell_hv_npx + 255) / 256,
                     st->hpart);
  return check_hip(hipGetLastError(), "ell_heavy_post launch");
}

}  // namespace espm
