/*
 * espm_mu.h - C ABI of libespm_mu.so: the SmoothNMF multiplicative-update hot path of
 * adriente/espm, written for AMD Instinct MI355X (gfx950 / CDNA4).
 *
 * The reference (pure Python/numpy, no FFI of its own) has exactly one compute path worth
 * a native boundary; the entry points below are what a binding for that path replaces.
 * Citations are file:line in the reference repository (adriente/espm @ v1.1.3):
 *
 *   espm_mu_step_h        <- espm/estimators/updates.py:83-156  multiplicative_step_h (KL branch)
 *                            + espm/estimators/dicotomy.py:4-55,111-173 (per-pixel simplex root)
 *                            + espm/utils.py:39-76 (Laplacian, as a stencil)
 *                            + espm/measures.py:456-504,524-548,560-577 (loss pieces of the INPUT state)
 *   espm_mu_h_finalize    <- espm/estimators/base.py:167-207, smooth_nmf.py:457-475 (loss assembly)
 *   espm_mu_w_accum       <- espm/estimators/updates.py:38-39,53-59 (R = X/(GWH), R H^T)
 *   espm_mu_w_reduce      <- (new) fixed-order reduction of the per-workgroup partial R H^T slabs
 *   espm_mu_w_finish      <- espm/estimators/updates.py:58-76 (G^T., simplex_W, clamp, fixed_W)
 *                            + updates.py:38 / base.py:189 (GW = G @ W) + base.py:323 (rel_W)
 *   (rel_H, base.py:324, is produced by espm_mu_step_h / espm_mu_h_finalize of the NEXT state evaluation)
 *   espm_mu_hstat         <- updates.py:139 (max_j H), updates.py:60 (sum_j H)
 *   espm_mu_step_hw       <- smooth_nmf.py:324-339 + :404-414 up to the sum over pixels: the H update and, with the new H, the
 *                            pixel contraction of the W update (updates.py:38-39, :53-59) in one launch
 *   espm_mu_iterate       <- espm/estimators/smooth_nmf.py:284-455 (_iteration, log_surrogate)
 *                            driven by base.py:313-394 (single GPU, no host sync)
 *   espm_mu_shard_*, espm_xchg_*, espm_mu_iterate_sharded
 *                         <- (new) pixel-row sharding over the GPUs of a node and its record exchange; no reference analogue
 *   espm_dichotomy_simplex<- espm/estimators/dicotomy.py:4-55 (module-level function)
 *   espm_simplex_root_f32 <- dicotomy.py:4-55 as the H update solves it: per pixel, fp32, in the shifted unknown (a launch of its own for tests)
 *   espm_mu_pack_x        <- base.py:243-247 (validate_data / hspy_comp transpose) as a layout step
 *   espm_mu_laplacian     <- espm/utils.py:39-76 applied to H (H @ L), measures.py:560-577
 *   espm_mu_w_reduce_finish, espm_mu_shard_combine_finish, espm_mu_w_reduce_pack
 *                         <- (new) the W-step after the accumulation in one call / launch (updates.py:58-76 folded into
 *                            the slab or rank-record reduction when W' needs nothing global)
 *   espm_mu_linesearch_terms, espm_mu_linesearch_terms_sharded
 *                         <- espm/estimators/surrogates.py:6-149 + smooth_nmf.py:376-381 (linesearch=True; a rank's rows)
 *   espm_mu_l2_step_h / _w, espm_mu_l2_w_partials / _finish
 *                         <- espm/estimators/updates.py:109-118, :31-36 (Frobenius branch, l2=True; the W step in two halves
 *                            around the sum over the ranks of a sharded image)
 *   state fields breg_sr_* <- updates.py:40-48, :120-125 (Bregman variant, algo = "bmd")
 *   state field h_rule = 1 <- updates.py:263-315 + dicotomy.py:57-82 (multiplicative_step_hq, algo = "l2_surrogate")
 *   h_rule = 2, pg_gamma_w, pg_q <- updates.py:317-395 + dicotomy.py:84-108 (proj_grad_step_h / _w, algo = "projected_gradient")
 *                            + smooth_nmf.py:382-401, :438-447 (its linesearch)
 *   espm_dichotomy_simplex_acc / _pg <- dicotomy.py:57-108 (module-level functions)
 *   espm_surrogate_terms  <- espm/estimators/surrogates.py:6-149 (module-level surrogates)
 *   espm_pixel_diagnostics<- (new) per-pixel Poisson deviance and Cramer-Rao bound of H given the spectra; no reference analogue
 *                            (hyperspy's model fitting reports them as red_chisq and the parameters' std)
 *   espm_channel_diagnostics <- (new) per-channel deviance, sum spectra and Fisher information of the spectra given the abundances
 *   espm_rebin_pixels, espm_binning_sums <- espm/datasets/eds_spim.py:746-798 (estimate_best_binning) on integer factors: the bin sums and
 *                            the four sums its risk estimate reduces to, from X on the device instead of a rebin and an upsample per candidate
 *   espm_thin_counts, espm_split_deviance <- (new) Poisson count splitting: a training and an independent held-out image from one measured
 *                            map, and the held-out deviance of a fit of the first; no reference analogue
 *   espm_poisson_sample, espm_sample_deviance <- espm/datasets/base.py:68 (np.random.poisson of the model on the host) as a rule on the
 *                            element's index: a count image drawn from a fitted model on the device, and the deviance of such draws
 *   espm_attribute_expected, espm_assign_counts <- espm/utils.py:396-414 (get_explained_intensity_W, the modelled intensity behind
 *                            every entry of W) for the MEASURED counts: the responsibilities of the components from a pass over X, and
 *                            (new) the image split into k integer images, one per component, that add up to it
 *   espm_weighted_marginals <- espm/datasets/eds_spim.py:364-384 (the channel windows of select_background_windows, masked_X = curr_X[mask])
 *                            as weighted sums of X, of the model and of the deviance term along either axis: line maps with a background
 *                            correction and a Poisson error bar, and the measured, modelled and residual spectrum of a region
 *   espm_residual_products <- (new) the Pearson residual matrix (X - Y) / sqrt(Y) applied to a block of vectors from either side: the
 *                            pass behind its leading singular triplets (a missing phase) and, against the independence model,
 *                            hyperspy's Poisson-normalised PCA scree plot; no reference analogue
 *   espm_pixel_ml         <- (new) per-pixel Poisson maximum-likelihood abundances given the spectra over a subset of the components,
 *                            EM with an optimality certificate and a per-pixel stop: the nested fits behind a likelihood-ratio
 *                            presence test; no reference analogue
 *   espm_pixel_ml_newton  <- (new) the same problem, certificate and stop by a safeguarded Newton step (EM's diagonal metric blended
 *                            into the Hessian, a fraction-to-boundary clamp, the EM successor after a rejected trial): tens of
 *                            passes where EM takes hundreds to thousands; no reference analogue
 *   espm_pixel_ml_pinned  <- (new) the same problem with one abundance held at a per-pixel value while the others are fitted, a
 *                            certificate of its own and the slope of the profile deviance: the evaluation behind profile-likelihood
 *                            intervals of the abundances (upper limits at the boundary); no reference analogue
 *   espm_pixel_ml_simplex <- (new) the same problem under sum h = 1, the pixel model of a simplex_H fit, with or without a pinned
 *                            abundance: a Frank-Wolfe certificate, the equality multiplier in the Newton step and in the EM
 *                            successor; presence tests and intervals of phase FRACTIONS; no reference analogue
 *   espm_lu_pl         <- espm/estimators/updates.py:179 -> scikit-learn's _initialize_nmf -> _randomized_range_finder: the LU
 *                            normaliser of its power iterations (scipy.linalg.lu(A, permute_l=True)[0]) on tall device matrices
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  All array pointers are DEVICE pointers owned by the
 *     caller (e.g. torch tensors); the library allocates nothing that outlives a call.
 *   - Every call only enqueues work on `stream` (a hipStream_t) and returns; no host sync.
 *   - Return value: 0 on success, negative espm_status otherwise; espm_mu_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - X is kept twice in HBM, once in the order each half-step streams it.  Dense stores: channel-major inside
 *     pixel blocks (p_pad / x_tile, n_cm, x_tile) for the H-step and pixel-major (p, n_pad) for the W-step, as u8
 *     (integer counts <= 255), bf16 or fp32, whichever is lossless.  Sparse count store (ESPM_X_ELL): 16-bit lists
 *     of the non-zero entries by pixel and by (pixel block, channel), described at the state fields below.
 *   - W, H, G, GW and every accumulator are fp32; loss sums are fp64.
 */
#ifndef ESPM_MU_H
#define ESPM_MU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* espm_stream_t; /* hipStream_t */

typedef enum espm_status {
  ESPM_OK = 0,
  ESPM_EINVAL = -1,       /* bad argument / shape (reference: ValueError / AssertionError) */
  ESPM_ENOSOLUTION = -2,  /* k * log_shift >= 1 (dicotomy.py:22-23 "No solution exists!") */
  ESPM_EHIP = -3,         /* HIP runtime error */
  ESPM_EUNSUPPORTED = -4  /* configuration not built (k > ESPM_MAX_K) */
} espm_status;

enum { ESPM_X_F32 = 0, ESPM_X_BF16 = 1, ESPM_X_U8 = 2 /* integer counts <= 255 */,
       ESPM_X_ELL = 3 /* integer counts, non-zero entries only (sparse count store, below) */ };
enum { ESPM_SRC_F32 = 0, ESPM_SRC_F64 = 1 };
enum { ESPM_LAYOUT_CM = 0 /* (n, p) channel-major */, ESPM_LAYOUT_PM = 1 /* (p, n) pixel-major */ };

/* The library is built three times from the same sources: libespm_mu.so (1..8 components, the strides below = 8),
 * libespm_mu_wide32.so (-DESPM_KP=32 -DESPM_MIN_K=17 -DESPM_MAX_K=32: 17..32 components; the dense stores only, H tiles of 128 pixels, on the
 * 8-bit and bf16 stores the matrix-core kernels only - espm/estimators/base.py:126-132 has no limit on n_components) and
 * libespm_mu_wide.so (-DESPM_KP=16 -DESPM_MIN_K=9 -DESPM_MAX_K=16: 9..16 components; the sparse store's LDS table then has
 * rows of 12 or 16 floats and must fit ESPM_ELL_LDS_MAX together with the numerators of a tile).  Same entry points, same state struct; every
 * size below that names KP follows the build. */
#ifndef ESPM_KP
#define ESPM_KP 8          /* padded component stride of GW (n_pad, KP) and H^T (p, KP): 8, 16 or 32 */
#endif
#ifndef ESPM_MAX_K
#define ESPM_MAX_K ESPM_KP /* components supported by the built kernels */
#endif
#ifndef ESPM_MIN_K
#define ESPM_MIN_K 1
#endif
#define ESPM_PPAD 512      /* p_pad is a multiple of this */
#define ESPM_NPAD 8        /* n_pad is a multiple of this */
#define ESPM_ELL_TILE 512  /* sparse store: pixels per H-step workgroup (8 lists of 64 pixels)               */
#define ESPM_ELL_PB 1024   /* sparse store at its full geometry: pixels per block of the W accumulation (state field ell_pb) */
#define ESPM_ELL_PBITS 10  /* log2(ESPM_ELL_PB)                                                             */
#define ESPM_ELL_UNIT_ROWS 8 /* sparse store: the unit rows of a list group are a multiple of this (16 entries: one per bank quad) */
#define ESPM_ELL_UNIT_MAX_N 4080 /* sparse store: H-step lists have unit rows when n <= this (index << 4 < 2^16, and at most 255 ones in any of the builder's 16 residue classes of a list: its 8-bit counters) */
#define ESPM_ELL_PAIR_MAX_K 6 /* sparse store H-step: list groups are walked in pairs (2 partial numerators) up to this k */
#define ESPM_ELL_STREAM_BYTES (256 << 20) /* sparse store: list bytes beyond which a caller sets espm_mu_state.ell_stream (the MI355X's last-level cache) */
#define ESPM_ELL_KEEP_BYTES 207000000 /* sparse store, streamed lists: the bytes of them a caller keeps in that cache all the same (espm_mu_state.ell_keep_h,
                                       * ell_keep_w): the best point of the sweep at 2048 x 512^2 - the H walk's 230.0 MB kept, the W walk's 233.5 MB
                                       * streamed, profiles/r07_keep_sweep.log - less 10 %: the cache is shared with whatever else runs */
#define ESPM_FUSED_MIN_PB 512 /* sparse store: W blocks (ell_pb) from which the fused launch is the default whatever their number           */
#define ESPM_FUSED_MIN_BLOCKS 192 /* ... and smaller blocks when there are at least this many (one per CU, or nearly: a 64-row shard of the
                                   * headline image has 256 of 128 pixels; config 2's 128 blocks leave half the chip to the two launches,
                                   * which then win: 27.6 against 35.2 us per iteration, profiles/r03e_c2_iter.log)                              */
#define ESPM_ELL_HEAVY_MIN 256   /* sparse store: counts from this on are heavy elements, kept outside the lists (espm_mu_state.ell_hv_*) */
#define ESPM_ELL_HEAVY_MAX (1 << 24) /* ... up to this (fp32 holds every integer up to it exactly)                                  */
#define ESPM_ELL_WTHREADS 1024 /* threads of a W-accumulation workgroup of the sparse store (16 waves)      */
#ifndef ESPM_ELL_BUCKETS
#define ESPM_ELL_BUCKETS 16    /* residue classes of the index by which a list's unit elements are placed in its unit rows (mu_ell_build.hip) */
#endif
#define ESPM_ELL_LDS_MAX (160 * 1024) /* LDS bytes the sparse H-step may use (GW table + numerators): a workgroup's LDS on gfx950 (144 KB until round 5) */
#define ESPM_NCM 16        /* channel rows of x_cm are padded to a multiple of this */
#define ESPM_W_DICOTOMY_TOL 1e-5f /* tolerance of the simplex multiplier of the W update: espm/conf.py dicotomy_tol, which the
                                     reference's multiplicative_step_w always uses (updates.py:61-68); the state's
                                     dicotomy_tol is the H update's (the estimator's argument, smooth_nmf.py) */
#define ESPM_TAIL_DEFER 1  /* espm_mu_state.tail_mode bits */
#define ESPM_TAIL_RIDE 2

/* per-workgroup partial record written by the H-step (doubles), stored field-major:
 * hpart[field * nblk + block] */
#define ESPM_HP_KL 0       /* sum X*log2(X/Y) over the block (input state)            */
#define ESPM_HP_REG 1      /* sum_k mu_k log(H_in + eps_reg)                           */
#define ESPM_HP_LAP 2      /* sum H_in * (H_in L)                                      */
#define ESPM_HP_BAD 3      /* count of non-finite H_out entries                        */
#define ESPM_HP_ROWSUM 4   /* [4, 4+KP): sum_j H_out[k, j]                             */
#define ESPM_HP_MAX (4 + ESPM_KP)      /* [4+KP, 4+2KP): max_j H_out[k, j]  (12 with KP = 8)           */
#define ESPM_HP_RELH (4 + 2 * ESPM_KP) /* (20) max |H_in - H_prev| / (H_in + tol mean H_in) over the block (base.py:324) */
#define ESPM_HP_PGQ (5 + 2 * ESPM_KP)  /* (21) projected-gradient rule only: sum <H' - H, grad> + gamma_H ||H' - H||^2 over the block */
#define ESPM_HP_RELW (6 + 2 * ESPM_KP)  /* (22) the block's share of rel_W of the W update that produced the input state (max over its slice of
                                         * the entries of W, base.py:323), where the launch carried that update's tail; else -1           */
#define ESPM_HP_NSCALAR 5  /* KL, REG, LAP, BAD, RELH                                  */
#define ESPM_HP_STRIDE (8 + 2 * ESPM_KP) /* (24) */

/* per-state statistics of one H buffer (doubles): produced by espm_mu_hstat / h_finalize */
#define ESPM_HS_ROWSUM 0   /* [0, KP)  */
#define ESPM_HS_MAX ESPM_KP /* [KP, 2 KP)  */
#define ESPM_HS_STRIDE (2 * ESPM_KP)

/* history record per evaluated state (doubles) */
#define ESPM_HI_KLX 0      /* xscale * sum X ln(X/Y)   (local pixels)                  */
#define ESPM_HI_REG 1      /* sum mu log(H+eps)        (local pixels)                  */
#define ESPM_HI_LAP 2      /* sum H*(HL)               (local pixels)                  */
#define ESPM_HI_SUMY 3     /* sum_k colsum(GW)_k * rowsum(H)_k  (uses the global rowsum in hstat) */
#define ESPM_HI_BAD 4      /* non-finite entries produced by the step that followed     */
#define ESPM_HI_REL_W 5    /* base.py:323 for the update that PRODUCED this state       */
#define ESPM_HI_REL_H 6    /* base.py:324 for the update that produced this state; evaluated by the H-step that
                              starts FROM this state (local max; max-reduce over ranks) */
#define ESPM_HI_STRIDE 8

/* Version of this header's binary interface: the layout of espm_mu_state and the meaning of its fields.  Every entry
 * point that takes a state checks st->struct_size == sizeof(espm_mu_state) and st->abi_version == ESPM_MU_ABI_VERSION
 * first and fails with ESPM_EINVAL otherwise: a binding whose copy of the layout has drifted is refused instead of
 * having its pointers misread.  A binding can also compare its layout field by field with espm_mu_state_layout(). */
#define ESPM_MU_ABI_VERSION 8

typedef struct espm_mu_state {
  uint32_t struct_size;   /* sizeof(espm_mu_state) as the CALLER sees it                  */
  uint32_t abi_version;   /* ESPM_MU_ABI_VERSION the caller was written against            */
  /* geometry */
  int32_t n;        /* energy channels: rows of X                                       */
  int32_t m;        /* columns of G; 0 means G = identity (then W is (n, k))            */
  int32_t k;        /* components, 1..ESPM_MAX_K                                        */
  int32_t p;        /* local pixels (= nx*ny when grid_mode = 1)                        */
  int32_t nx, ny;   /* local image rows, row length                                     */
  int32_t n_pad;    /* roundup(n, ESPM_NPAD)                                            */
  int32_t p_pad;    /* roundup(p, ESPM_PPAD)                                            */
  int32_t x_dtype;  /* ESPM_X_F32 | ESPM_X_BF16 | ESPM_X_U8 | ESPM_X_ELL                */
  int32_t tile_px;  /* H-step pixel tile per workgroup: 64 * {1,2,4,8}, see query       */
  int32_t nblk_w;   /* pixel blocks of the W accumulation (rows of a_slab)              */
  int32_t x_tile;   /* pixel-block width of the tile-major x_cm (multiple of tile_px)   */
  int32_t n_cm;     /* roundup(n, ESPM_NCM): channel rows per pixel block of x_cm       */
  int32_t h_variant; /* must be 0 (1 was the retired matrix-core H-step) */
  int64_t p_total;  /* pixels of the whole image over all ranks (= p on one GPU)        */
  /* flags */
  int32_t simplex_h, simplex_w;
  int32_t grid_mode;        /* 0: L = identity (shape_2d None, base.py:289-291), 1: 2-D stencil */
  int32_t compute_loss;     /* H-step also accumulates the KL term (1 log per element)  */
  /* scalars */
  float lambda_l, sigma_l, eps_reg, log_shift, dicotomy_tol, rel_tol;
  float xscale;     /* X_ = xscale * X_stored (normalize=True, base.py:264-267)         */
  float gw_floor;   /* lower clamp of GW entries, keeps X/(GW H) finite (updates.py:129-131) */
  /* data */
  const void* x_cm;         /* (p_pad / x_tile, n_cm, x_tile) u8|bf16|f32: channel-major inside pixel blocks, zero padded */
  const void* x_pm;         /* (p, n_pad) bf16|f32, zero padded                         */
  const float* g;           /* (n, m) row-major or NULL                                  */
  const float* colsum_g;    /* (m) or NULL                                               */
  float* w[2];              /* (m or n, k) row-major, ping-pong                          */
  float* gw_s;              /* (n_pad, KP): GW / xscale, pad rows = 1                    */
  double* colsum_gw;        /* (KP): column sums of GW over real rows                    */
  void* gw_a;               /* reserved (NULL): operands of the retired matrix-core H-step */
  float* gw_p;              /* reserved (NULL) */
  float* h[2];              /* (k, p_pad), ping-pong, pad columns must be positive       */
  float* h_t;               /* (p, KP): transposed copy of the newest H                  */
  const float* mu;          /* (k) or NULL                                               */
  const float* fixed_h;     /* (k, p_pad), entries >= 0 are imposed; or NULL             */
  const float* fixed_w;     /* (m or n, k) or NULL                                       */
  const int32_t* simplex_rows; /* (m or n) 0/1 mask of rows under simplex_W, NULL = all  */
  const float* halo_top;    /* (k, ny) image row above the local block or NULL           */
  const float* halo_bot;    /* (k, ny) image row below the local block or NULL           */
  /* workspaces */
  double* hpart;            /* (ESPM_HP_STRIDE, ceil(p / tile_px)) field-major              */
  double* hstat[2];         /* (ESPM_HS_STRIDE) statistics of h[0] / h[1] (global)       */
  float* a_slab;            /* (nblk_w, k, n_pad)                                        */
  float* a;                 /* (k, n_pad)                                                */
  float* w_scratch;         /* (2, m or n, k), zero before the first call (a ticket of the dictionary-G W finish lives there); NULL keeps the W update
                             * off its many-workgroup forms (A/B, tests) - the general one-workgroup finish then refuses an update (ESPM_EINVAL) */
  double* hist;             /* (hist_len, ESPM_HI_STRIDE), zero-initialised              */
  int32_t hist_len;
  int32_t cur;              /* index of the current W/H buffers (0/1), flipped by iterate */
  int32_t it;               /* number of completed iterations = history slot of the current state */
  /* Sparse count store (x_dtype = ESPM_X_ELL; x_cm / x_pm are then unused and may be NULL).  Only the non-zero
   * entries of X are kept, 16 bits each, as lists padded to the longest of 64 ("ELL"): the entries 2r and 2r+1
   * of the 64 lists of a wave form row r of 64 dwords (low half first), value 0 = padding.  A count that
   * exceeds its field is split over several entries with the same index (the kernels evaluate the loss term
   * x_i log2(x_i / Y) per entry; ell_klc restores sum x log2(x / Y) for split counts).
   *   H-step: one list per pixel; entry = count << ell_cbits | channel.  Inside every window of tile_px pixels
   *           (the pixels of one H-step workgroup) the lists are ordered by decreasing length: slot s of the
   *           window starting at pixel w0 is pixel w0 + pix_perm[w0 + s], and the 64 lists of a wave are 64
   *           consecutive slots, so they have about the same length (little padding).  Rows
   *           [ell_h_off[2 g], ell_h_off[2 g + 2]) belong to slots 64 g .. 64 g + 63.
   *   W-step: one list per (block of ell_pb = 2 tile_px pixels, channel); inside block b the 64 lists of a wave are
   *           the channels chan_perm[b][64 cg .. 64 cg + 63] (the block's channels by decreasing list length,
   *           -1 = none); entry = count << log2(ell_pb) | pixel - block start; rows
   *           [ell_w_off[2 i], ell_w_off[2 i + 2]) with i = b * n_cg + cg.  nblk_w = ceil(p / ell_pb).
   *   UNIT rows: most non-zero entries of a count image are ones.  The first rows [off[2 i], off[2 i + 1]) of
   *           a group hold only entries with count 1, in EVERY lane and position (no padding), stored without a
   *           count as index << 4 (the byte offset of a 16-byte table row): u = min over the 64 lists of their
   *           elements equal to 1, unit rows = ESPM_ELL_UNIT_ROWS * floor(u / (2 ESPM_ELL_UNIT_ROWS)); a list's
   *           2 * (unit rows) of a list's ones go there - which ones and in which order is the builder's choice
   *           (espm_mu_ell_fill places the ones of lane l with index = q mod 16 at positions = q - l mod 16, so
   *           that the 16 lanes of a ds_read_b128 group address 16 different bank quads of the table) - all its
   *           other elements go to the general rows [off[2 i + 1], off[2 i + 2]) in the count << bits | index
   *           form.  H-step lists have unit rows only when n <= ESPM_ELL_UNIT_MAX_N. */
  const uint32_t* ell_h;    /* (rows_h, 64) */
  const int32_t* ell_h_off; /* (2 p_pad / 64 + 1) */
  const float* ell_klc;     /* (p_pad): loss correction of split counts per pixel: sum over the elements of
                               x log2 x minus the sum over their entries x_i of x_i log2 x_i (0 without splits) */
  const uint32_t* ell_w;    /* (rows_w, 64) */
  const int32_t* ell_w_off; /* (2 nblk_w * n_cg + 1) */
  const int32_t* chan_perm; /* (nblk_w, 64 * n_cg) */
  int32_t ell_cbits;        /* index bits of an H-step entry: 2^ell_cbits >= n, <= 14 */
  int32_t n_cg;             /* channel groups: ceil(n / 64) */
  const int32_t* pix_perm;  /* (p_pad): slot -> pixel offset inside its tile_px window (H-step lists) */
  const float* g_t;         /* optional (m, n_pad): G transposed, zero padded; the W finish then reads G with
                               coalesced loads (NULL: it reads g with a stride of m) */
  /* Bregman variant of both updates (updates.py:40-48, :120-125; algo = "bmd"), G = identity only (the reference's own W
   * step needs a square G).  Sums of the STORED X, both or neither:
   *   H: num = sR / H, denum = colsum(GW) - GW^T (X / GWH) + sR / H      with sR_j = xscale * breg_sr_px[j] = sum_c X_cj
   *   W: W' = sR W / ((rowsum(H) - (X / GWH) H^T) W + sR), no simplex    with sR_c = xscale * breg_sr_ch[c] = sum_j X_cj */
  const float* breg_sr_px;  /* (p_pad) or NULL */
  const float* breg_sr_ch;  /* (n) or NULL */
  int32_t h_rule;           /* H update: 0 = log surrogate (multiplicative_step_h, updates.py:83-156), 1 = quadratic surrogate
                               of the Laplacian term (multiplicative_step_hq, updates.py:263-315: positive root of
                               a H'^2 + b H' - c = 0, its own simplex multiplier dicotomy.py:57-82; mu only enters the loss),
                               2 = projected gradient (proj_grad_step_h, updates.py:372-395: H - grad / gamma_H with
                               gamma_H in sigma_l, projection on the simplex dicotomy.py:84-108) */
  float pg_gamma_w;         /* > 0: the W update is the projected-gradient step W - grad / pg_gamma_w, clamped
                               (proj_grad_step_w, updates.py:353-370; no simplex over W); 0: multiplicative update */
  double* pg_q;             /* optional (hist_len, 2): terms of the projected gradient's linesearch (smooth_nmf.py:382-401,
                               :438-447; surrogates.py:153-170).  [t][0] = sum <H' - H, grad_H> + gamma_H ||H' - H||^2 of
                               the H update that STARTS from state t (written by espm_mu_h_finalize(.., slot = t));
                               [t][1] = the same for the W update that PRODUCED state t.  The caller adds the losses. */
  /* Sparse store, pixels without a single count.  The reference fills them with log_shift in every channel
   * (base.py:519-528); under simplex_H that fill alone decides their column of H.  The lists stay empty for such a
   * pixel; instead ell_klc[pixel] = -(1 + i) names entry i of ell_fill_px, and espm_mu_step_h first forms the fill's
   * numerator log_shift * sum_c GW_c / (GW_c . H_pixel) of the ell_fill_n listed pixels into ell_fill_num
   * (k, ell_fill_n), which the H-step's epilogue adds.  The fill's part in the W update and in the loss is O(log_shift)
   * and is left out.  ell_fill_n = 0: no such pixel, both pointers may be NULL. */
  const int32_t* ell_fill_px;
  float* ell_fill_num;
  int32_t ell_fill_n;
  /* Tail of the local W update (espm_mu_w_update_is_local: column sums of G W' -> colsum_gw, rel_W -> hist): one small
   * workgroup, 8 us as a launch of its own.  bit 0 (ESPM_TAIL_DEFER): espm_mu_w_reduce_finish / espm_mu_shard_combine_finish
   * leave it out.  bit 1 (ESPM_TAIL_RIDE): the next espm_mu_step_h / espm_mu_loss_only (sparse store) carries the tail of
   * the update that PRODUCED state `it` (w[1 - src] -> w[src]) as an extra workgroup and sums the partial column sums
   * itself; the caller sets the bit for that one call, or flushes with espm_mu_w_update_tail.  espm_mu_iterate does all
   * this internally and ignores the field. */
  int32_t tail_mode;
  /* Sparse store, default H rule: espm_mu_iterate and espm_mu_step_hw run both half-steps of an iteration in ONE launch -
   * the workgroup that has updated the ell_pb pixels of a block (two H tiles) goes straight on with that block's part of
   * R H^T, which needs no other pixel's new H (updates.py:38-39, :53-59); h_t is then not written.  no_fused = 1 keeps the
   * two launches (A/B, tests); 2 runs the fused kernel with a fixed assignment of its work units to waves instead of the
   * dynamic one (A/B only). */
  int32_t no_fused;
  /* Sparse store: pixels per block of the W accumulation = 2 tile_px (espm_mu_query): ESPM_ELL_PB = 1024 for an image that
   * fills the chip with 512-pixel H tiles, 128 .. 512 for smaller images and shards, so that there is about one block per
   * compute unit and one workgroup can own the block through both half-steps. */
  int32_t ell_pb;
  /* Sparse store: 1 = the lists (256 bytes per row of ell_h and ell_w: the rows[2] of espm_mu_ell_plan) do not fit the device's
   * last-level cache, i.e. exceed ESPM_ELL_STREAM_BYTES: the one-launch iteration then reads them with non-temporal loads, which
   * leave that cache to what IS read again (measured: -1.4 % at 2048 x 512^2, where the lists are 0.5 GB; +15 % if set on a
   * 64-row shard of it, whose lists stay in the cache from one iteration to the next).  A hint: results are the same bits
   * either way, and a launch without a streamed form (blocks below ESPM_ELL_PB pixels, the generic instances) ignores it.
   * 0 or 1; anything else is ESPM_EINVAL.  ABI 8: with 1 a part of the lists can be kept in that cache all the same - the lists are
   * fixed for a whole fit: ell_keep_h, ell_keep_w at the end of this struct (2048 x 512^2: the H walk's 230 MB kept behind the W walk's
   * 234 MB streamed, 118.5-119.4 -> 113.8-114.5 us per iteration, profiles/r07_keep_sweep.log). */
  int32_t ell_stream;
  /* Sparse store, heavy elements: integer counts ESPM_ELL_HEAVY_MIN .. ESPM_ELL_HEAVY_MAX (256 .. 2^24; fp32 holds every integer up
   * to 2^24 exactly) are kept outside the 16-bit lists, with their exact values; the lists, ell_klc and the permutations are those of
   * the image with these elements set to 0.  Two orders of the same elements:
   *   pixel-major (H half-step): the ell_hv_npx pixels that hold heavy elements, ascending, in ell_hv_px; pixel i's elements are
   *           ell_hv_pm[ell_hv_px_off[i] .. ell_hv_px_off[i + 1]), {channel, count} pairs by ascending channel.  Such a pixel is
   *           marked in ell_klc as entry ell_fill_n + i of the fill table, ell_klc = -(1 + ell_fill_n + i), and its own loss
   *           constant moves to ell_hv_klc[i]; ell_fill_num is then (k, ell_fill_n + ell_hv_npx) and ell_fill_px names the
   *           ell_fill_n fill pixels only.  Before every H update (and loss evaluation) a pass forms the heavy numerator
   *           sum_c x GW_c / (GW_c . H_pixel) into that column of ell_fill_num, which the H-step's epilogue adds like the fill's,
   *           and the pixels' loss terms ell_hv_klc[i] + sum x log2(x / Y), summed per 256 of them, into the workspace ell_hv_kl;
   *           after the launch one workgroup adds the sum of those partial sums (fixed order) to the KL field of the first hpart record.
   *   by (W block, channel) (W accumulation): group g holds the elements of channel ell_hv_grp[g] in the W block of ell_pb pixels
   *           that contains them, ell_hv_wm[ell_hv_grp_off[g] .. ell_hv_grp_off[g + 1]) as {pixel, count} by ascending pixel; groups
   *           by block, then channel.  After the accumulation one thread per group adds sum x / Y' H'_pixel to its entries of
   *           a_slab[block] (no atomics: a group owns them), so every reduction of the slabs sums them unchanged.
   * ell_hv_n = 0: no heavy element, every pointer below may be NULL and nothing runs. */
  int32_t ell_hv_n;              /* heavy elements                                          */
  int32_t ell_hv_npx;            /* pixels with heavy elements                              */
  int32_t ell_hv_ngrp;           /* (W block, channel) groups                               */
  const int32_t* ell_hv_px;      /* (ell_hv_npx)                                            */
  const int32_t* ell_hv_px_off;  /* (ell_hv_npx + 1)                                        */
  const int32_t* ell_hv_pm;      /* (ell_hv_n, 2) {channel, count}, pixel-major             */
  const float* ell_hv_klc;       /* (ell_hv_npx) the pixels' loss constants of their lists  */
  double* ell_hv_kl;             /* (ell_hv_npx) workspace: partial sums of the loss terms  */
  const int32_t* ell_hv_grp;     /* (ell_hv_ngrp) channel of each group                     */
  const int32_t* ell_hv_grp_off; /* (ell_hv_ngrp + 1)                                       */
  const int32_t* ell_hv_wm;      /* (ell_hv_n, 2) {pixel, count}, by (W block, channel)     */
  /* H-only iterations (espm_mu_iterate_h): a second record buffer of hpart's size.  Consecutive H-steps then write their records to
   * hpart and hpart_alt in turn, and each reduces what it needs of its predecessor's records itself: one launch per iteration
   * (espm_mu_h_chain_applies).  NULL: espm_mu_iterate_h runs espm_mu_step_h + espm_mu_h_finalize per iteration.  Nothing else reads it. */
  double* hpart_alt;
  /* Sparse store: (nblk_w, n_pad) floats - the sum of the counts that the LISTS hold of channel c in W block b (ell_pb pixels) at
   * [b * n_pad + c]; heavy elements are not in the lists and not in these sums, channels n .. n_pad - 1 hold 0.  Fixed when the store
   * is built (espm_mu_ell_block_counts; 2 MB at 2048 channels x 512^2 pixels).  The lean instances of the one-launch iteration at 5 components gather rows
   * of G W divided by their sums sigma_c (one 16-byte read per list entry) and owes the loss sum_c ell_blk_cnt[b][c] log2 sigma_c per
   * block: it needs this array whenever compute_loss is set and fails with ESPM_EINVAL without it.  Nothing else reads it. */
  const float* ell_blk_cnt;
  /* Sparse store with ell_stream = 1: the part of the lists that is KEPT in the last-level cache.  The lists are fixed for a whole fit,
   * so what stays on the die after one iteration need not come from memory in the next: ell_keep_h of the tile_px / 64 list groups of
   * every H tile and ell_keep_w of the n_cg channel groups of every W block are read with plain loads, the rest with non-temporal ones.
   * Which ones: index j of n is kept where floor((j + 1) keep / n) steps - spread evenly, the same in every tile and block (kernel:
   * ell_kept, mu_ell_kernel.hpp; a caller: espm_amd/ell.py, keep_policy, which fits the kept bytes into ESPM_ELL_KEEP_BYTES).
   * 0, 0: every list row non-temporal, as before ABI 8.  Ignored when ell_stream = 0; otherwise 0 <= ell_keep_h <= tile_px / 64 and
   * 0 <= ell_keep_w <= n_cg or ESPM_EINVAL.  Hints like ell_stream: the same bits at every setting. */
  int32_t ell_keep_h;
  int32_t ell_keep_w;
} espm_mu_state;

const char* espm_mu_version(void);
const char* espm_mu_last_error(void);
/* sizeof(espm_mu_state) and ESPM_MU_ABI_VERSION of the library, and its view of the layout as text:
 * "name:offset:size;" for every field in declaration order (arrays: the whole array), NUL-terminated, static storage. */
size_t espm_mu_state_size(void);
int espm_mu_abi_version(void);
const char* espm_mu_state_layout(void);

/* Fills n_pad, p_pad, tile_px, x_tile, nblk_w of `st` from n, p, k, x_dtype and the device's CU count. */
int espm_mu_query(espm_mu_state* st);

/* X (host layout, device memory) -> the two padded device layouts.  src is (n, p) when
 * src_layout = CM or (p, n) when PM (hyperspy's layout), leading dimension ld (elements). */
int espm_mu_pack_x(const void* src, int src_dtype, int src_layout, int64_t ld, int n, int p,
                   void* x_cm, void* x_pm, int x_dtype, int n_pad, int p_pad, int x_tile, int n_cm,
                   espm_stream_t stream);

/* Sparse count store (x_dtype = ESPM_X_ELL) from the dense pixel-major 8-bit matrix x_pm_u8 (p, n_pad) that
 * espm_mu_pack_x writes for x_dtype = ESPM_X_U8 (its x_cm argument may be NULL then).  `st` needs n, p, x_dtype =
 * ESPM_X_ELL and espm_mu_query.  Three steps, all buffers caller-allocated:
 *   count: cnt_px (2, p_pad) entries of each pixel's H-step list, then its elements equal to 1; cnt_bc (2, nblk_w,
 *          64 n_cg) the same for each (pixel block, channel) W-step list (natural channel order); ell_klc (p_pad).
 *   plan : chan_perm (nblk_w, 64 n_cg), pix_perm (p_pad; windows of st->tile_px pixels), ell_h_off (2 p_pad / 64 + 1),
 *          ell_w_off (2 nblk_w n_cg + 1) and rows[2] (device):
 *          rows of 64 dwords of the H-step and of the W-step lists.  The caller reads rows[] back, checks
 *          64 rows < 2^31 and allocates ell_h (rows[0], 64) and ell_w (rows[1], 64), ZERO-initialised.
 *   fill : writes the entries.  The dense x_pm_u8 can be released afterwards.  Optional, for speed: st->x_cm != NULL hands the fill the
 *          same 8-bit counts channel-major, [p_pad / ESPM_PPAD][n_cm][ESPM_PPAD] - espm_mu_pack_x's x_cm output with x_tile = ESPM_PPAD -
 *          from which the channel lists are read with 16-byte loads (the lists come out the same); reset st->x_cm to NULL afterwards. */
int espm_mu_ell_count(const espm_mu_state* st, const void* x_pm_u8, int32_t* cnt_px, int32_t* cnt_bc, float* ell_klc,
                      espm_stream_t stream);
/* espm_mu_state.ell_blk_cnt from the same 8-bit matrix (the heavy elements already taken out of it): blk_cnt (nblk_w, n_pad) floats,
 * caller-allocated, every entry written.  Needs of `st` what espm_mu_ell_count needs. */
int espm_mu_ell_block_counts(const espm_mu_state* st, const void* x_pm_u8, float* blk_cnt, espm_stream_t stream);
/* The same two steps with the lists' histograms of unit elements handed from count to fill, which saves the fill its first of two passes
 * over X: ESPM_ELL_BUCKETS bytes per list - its elements equal to 1 per residue class of their index (channel; pixel inside the block) mod
 * ESPM_ELL_BUCKETS, what the placement of the unit rows goes by.  bkt_px (p_pad, ESPM_ELL_BUCKETS) and bkt_bc (nblk_w, 64 n_cg,
 * ESPM_ELL_BUCKETS) bytes, caller-allocated, both or neither (NULL, NULL = the functions without _hist).  The lists come out the same. */
int espm_mu_ell_count_hist(const espm_mu_state* st, const void* x_pm_u8, int32_t* cnt_px, int32_t* cnt_bc, float* ell_klc, uint8_t* bkt_px,
                           uint8_t* bkt_bc, espm_stream_t stream);
int espm_mu_ell_fill_hist(const espm_mu_state* st, const void* x_pm_u8, const int32_t* chan_perm, const int32_t* pix_perm,
                          const int32_t* ell_h_off, const int32_t* ell_w_off, uint32_t* ell_h, uint32_t* ell_w, const uint8_t* bkt_px,
                          const uint8_t* bkt_bc, espm_stream_t stream);
int espm_mu_ell_plan(const espm_mu_state* st, const int32_t* cnt_px, const int32_t* cnt_bc, int32_t* chan_perm,
                     int32_t* pix_perm, int32_t* ell_h_off, int32_t* ell_w_off, int64_t* rows, espm_stream_t stream);
int espm_mu_ell_fill(const espm_mu_state* st, const void* x_pm_u8, const int32_t* chan_perm, const int32_t* pix_perm,
                     const int32_t* ell_h_off, const int32_t* ell_w_off, uint32_t* ell_h, uint32_t* ell_w,
                     espm_stream_t stream);
/* Heavy elements of the sparse store (espm_mu_state.ell_hv_*) from the dense image x (src_dtype ESPM_SRC_F32 / _F64, src_layout CM
 * (n, p) or PM (p, n), leading dimension ld: espm_mu_pack_x's source), in two steps around the caller's prefix sum:
 *   count: cnt_px (p) heavy elements of each pixel; sets them to 0 in the 8-bit copies x_pm_u8 (p, n_pad) and, if not NULL, x_cm_u8
 *          ([p_pad / ESPM_PPAD][n_cm][ESPM_PPAD]) that espm_mu_pack_x wrote, so that the lists built from them leave them out.
 *   fill : px_off (p + 1, the exclusive prefix sum of cnt_px) -> hv_pm (px_off[p], 2) {channel, count} pairs, pixel-major,
 *          ascending channel.  The pixels with elements and the (W block, channel) order are plain sorting (espm_amd/ell.py). */
int espm_mu_ell_heavy_count(const espm_mu_state* st, const void* x, int src_dtype, int src_layout, int64_t ld, uint8_t* x_pm_u8,
                            uint8_t* x_cm_u8, int32_t* cnt_px, espm_stream_t stream);
int espm_mu_ell_heavy_fill(const espm_mu_state* st, const void* x, int src_dtype, int src_layout, int64_t ld, const int32_t* px_off,
                           int32_t* hv_pm, espm_stream_t stream);

/* statistics (row sums, row maxima) of st->h[which] into st->hstat[which] (local pixels). */
int espm_mu_hstat(const espm_mu_state* st, int which, espm_stream_t stream);

/* gw_s, colsum_gw from g, w[which] (updates.py:107). */
int espm_mu_build_gw(const espm_mu_state* st, int which, espm_stream_t stream);

/* H update: reads h[src], writes h[1-src] and h_t, partial sums to hpart.
 * write_h = 0 evaluates the loss pieces of the input state only. */
int espm_mu_step_h(const espm_mu_state* st, int src, int write_h, espm_stream_t stream);

/* Reduces hpart: history slot `slot` gets the loss pieces of h[src] and (slot > 0) rel_H of the update
 * that produced h[src]; hstat[1-src] gets the statistics of the new H (local; the caller max/sum-reduces
 * over ranks when sharded). */
int espm_mu_h_finalize(const espm_mu_state* st, int src, int slot, espm_stream_t stream);

/* Loss pieces of the state (w[src], h[src]) into history slot `slot`; H is not updated. */
int espm_mu_loss_only(const espm_mu_state* st, int src, int slot, espm_stream_t stream);

/* A_slab[b] = sum over the pixels of block b of R[:, j] H[:, j]^T with R = X / (GW H), H = h_t. */
int espm_mu_w_accum(const espm_mu_state* st, espm_stream_t stream);
/* espm_mu_step_h(st, src, 1) and espm_mu_w_accum as ONE launch where espm_mu_fused_applies(st) (see no_fused above), else
 * as those two calls: reads h[src]; writes h[1 - src], the records of hpart and a_slab.  (Fused: one record per block of
 * 1024 pixels in every other record slot, zeros - neutral for every field - in between, so that espm_mu_h_finalize and
 * the reduction calls read the records as they always do; h_t is left alone.) */
int espm_mu_step_hw(const espm_mu_state* st, int src, espm_stream_t stream);
int espm_mu_fused_applies(const espm_mu_state* st);
/* a = sum_b a_slab[b] in fixed order (one pass, bit-reproducible). */
int espm_mu_w_reduce(const espm_mu_state* st, espm_stream_t stream);
/* espm_mu_w_reduce and espm_mu_h_finalize(st, src, slot) in ONE launch (the reduction of the H-step's records
 * rides in an extra workgroup): for callers that sequence the half-steps themselves, after espm_mu_step_h(src, 1)
 * and espm_mu_w_accum. */
int espm_mu_w_reduce_finalize(const espm_mu_state* st, int src, int slot, espm_stream_t stream);
/* W update from a (sharded: the all-rank sum written by espm_mu_shard_combine) and hstat[hsrc] (global
 * row sums of the new H): reads w[src], writes w[1-src], gw_s, colsum_gw and rel_W into history slot `slot`. */
int espm_mu_w_finish(const espm_mu_state* st, int src, int hsrc, int slot, espm_stream_t stream);

/* The rest of the W-step after espm_mu_w_accum in one call: slab reduction (with espm_mu_h_finalize(st, src, slot)
 * riding in its launch when with_finalize != 0) and the W update w[src] -> w[1-src] with the row sums of the new H
 * h[1-src]; rel_W goes to history slot + 1.  When W' needs nothing global (G = identity, no simplex_W, n >= 64) the
 * reduction workgroups finish their own entries of W and a one-workgroup tail forms colsum(GW') and rel_W (w_scratch
 * holds the partials).  With the simplex over W, G = identity, every row in the simplex (no simplex_rows), the default
 * multiplicative rule and n_pad a multiple of 32, the multipliers follow from per-component sums over the channels
 * (dicotomy.py:111-173 applied to f(delta) = S / delta + n0 eps - 1): the reduction also leaves those sums per 32 channels
 * and a second many-workgroup launch finds the multipliers and updates W (same tail; no_fused = 1 keeps the one-workgroup
 * finish for A/B).  Otherwise this is espm_mu_w_reduce[_finalize] + espm_mu_w_finish. */
int espm_mu_w_reduce_finish(const espm_mu_state* st, int src, int slot, int with_finalize, espm_stream_t stream);

/* n_iter full iterations on one GPU, no host synchronisation; updates st->cur / st->it.
 * History slot t holds the loss pieces of state t (slot 0 = initial state) and the relative
 * changes of the update that produced it.  A final loss-only H-step fills the last slot when
 * final_loss != 0. */
int espm_mu_iterate(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream);
/* n_iter H-only iterations (W held: what the reference computes with fixed_W = W, updates.py:75-76 - the H rule every iteration,
 * rel_W = 0): w[], gw_s and colsum_gw are not touched; st->cur flips with every iteration as the index of the current H only - W
 * stays in the buffer it was in (a caller that reads w[st->cur] afterwards keeps the same W in both) - and st->it advances.  No host
 * synchronisation.
 * History slot t gets the loss pieces of state t and rel_H of the update that produced it; rel_W of the slots it + 1 .. it + n_iter
 * is written as 0.  A final loss-only H-step fills the last slot when final_loss != 0.  Never the fused launch of espm_mu_step_hw.
 * Where espm_mu_h_chain_applies(st) an iteration is ONE launch: the H-step reduces the row sums and maxima it needs from its
 * predecessor's records itself (the records alternate between hpart and hpart_alt) and an extra workgroup writes the predecessor's
 * history row and hstat; one espm_mu_h_finalize closes the batch.  Otherwise espm_mu_step_h + espm_mu_h_finalize per iteration.  Same
 * bits either way.
 * espm_mu_h_chain_applies: 1 for the default H rule (h_rule = 0, no Bregman variant) with compute_loss and hpart_alt set, on the sparse
 * store without heavy elements (1..16 components) and on the 8-bit, bf16 and fp32 stores up to 12 components; else 0
 * (a negative espm_status for a state the library refuses). */
int espm_mu_iterate_h(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream);
int espm_mu_h_chain_applies(const espm_mu_state* st);
/* 1 when the W update needs nothing global (G = identity, no simplex over W, ...): the slab / record reduction updates W
 * itself and a tail workgroup finishes (tail_mode above); 0: espm_mu_w_finish does the update, there is no tail. */
int espm_mu_w_update_is_local(const espm_mu_state* st);
/* Which form the unsharded W half-step takes for this state, as espm_mu_iterate / espm_mu_w_reduce_finish sequence it (the local
 * update and the simplex split run inside the slab reduction's launches) and, behind those two, as espm_mu_w_finish launches it.
 * Answered from the plan that the launch itself switches on.  No predicate depends on the pixel count.
 *   ESPM_W_FORM_LOCAL          the reduction workgroups update their own entries of W (what espm_mu_w_update_is_local says)
 *   ESPM_W_FORM_SIMPLEX_SPLIT  simplex over every row of W with G = identity: slab reduction + bracket sums, then a many-workgroup update
 *   ESPM_W_FORM_DICT_COLUMNS   dictionary G with at most 32 columns over at most 2048 padded channels: one launch, a workgroup per component
 *   ESPM_W_FORM_DICT_TWO_LAUNCH  dictionary G without simplex / projected gradient / Bregman, m k <= 8192: update per entry, then rows of G W'
 *   ESPM_W_FORM_ONE_WG_REGISTERS  one workgroup that keeps its rows of W in registers (1..16 components)
 *   ESPM_W_FORM_ONE_WG_GENERAL   one workgroup, nothing register-resident: everything else, and all of the 17..32 build
 * (ESPM_W_GCOL=0, ESPM_W_GSPLIT=0 and ESPM_W_FINISH_GENERAL=1 in the environment, read once per process, move a state down this list.)
 * detail (may be NULL): 0 except for ESPM_W_FORM_ONE_WG_REGISTERS, where it packs the kernel instance -
 *   bits 0..11 threads of the workgroup (512 or 1024), bits 12..15 rows of W per thread (1, 2, 4), bits 16..19 channels per thread
 *   in the phase that forms G^T A (1, 2, 4; equal to the rows with G = identity), bit 20 set when G^T A is the all-threads one
 *   (dictionary G, m k <= 512, k <= 8) and not one wave per entry.  ESPM_W_DETAIL_* below unpack it.
 * A negative espm_status for a state the library refuses. */
#define ESPM_W_FORM_LOCAL 1
#define ESPM_W_FORM_SIMPLEX_SPLIT 2
#define ESPM_W_FORM_DICT_COLUMNS 3
#define ESPM_W_FORM_DICT_TWO_LAUNCH 4
#define ESPM_W_FORM_ONE_WG_REGISTERS 5
#define ESPM_W_FORM_ONE_WG_GENERAL 6
#define ESPM_W_DETAIL_THREADS(d) ((d) & 0xfff)
#define ESPM_W_DETAIL_ROWS(d) (((d) >> 12) & 0xf)
#define ESPM_W_DETAIL_CHANNELS(d) (((d) >> 16) & 0xf)
#define ESPM_W_DETAIL_GTA_ALL_THREADS(d) (((d) >> 20) & 1)
int espm_mu_w_update_form(const espm_mu_state* st, int* detail);
/* The tail of the update w[src] -> w[1 - src] that produced state slot + 1, as a launch of its own (after a finish call
 * with ESPM_TAIL_DEFER when no H-step will carry it). */
int espm_mu_w_update_tail(const espm_mu_state* st, int src, int slot, espm_stream_t stream);

/* Sharded image (pixel rows split over ranks).  Per iteration every rank packs one
 * record [A | hstat of the new H | first and last owned image row of the new H], the caller
 * all-gathers the records (RCCL), and shard_combine sums A over ranks in fixed order, forms the
 * global row sums / maxima in hstat[hnew].  The halo rows for the next H-step are read in place
 * from the neighbours' records: offsets k*n_pad*4 + ESPM_HS_STRIDE*8 (+ k*ny*4 for the last row). */
size_t espm_mu_shard_record_bytes(const espm_mu_state* st);
int espm_mu_shard_pack(const espm_mu_state* st, int hnew, void* record, espm_stream_t stream);
/* espm_mu_w_reduce_finalize(st, src, slot) + espm_mu_shard_pack(st, 1 - src, record) in ONE launch: the slab reduction
 * writes A straight into the record, the finalize workgroup puts the statistics of the new H h[1-src] there (the
 * LOCAL ones; st->a and st->hstat[1-src] are not written) and copies its boundary rows. */
int espm_mu_w_reduce_pack(const espm_mu_state* st, int src, int slot, void* record, espm_stream_t stream);
int espm_mu_shard_combine(const espm_mu_state* st, const void* records, int world, int hnew,
                          espm_stream_t stream);
/* espm_mu_shard_combine(.., hnew = 1 - src) + espm_mu_w_finish(st, src, 1 - src, slot + 1) in one call; the sum over
 * the ranks and the W update share a launch when W' needs nothing global (see espm_mu_w_reduce_finish). */
int espm_mu_shard_combine_finish(const espm_mu_state* st, const void* records, int world, int src, int slot,
                                 espm_stream_t stream);

/* ---- one-shot record exchange between the ranks of a node (SURVEY 8b "espm_allreduce", 8e) --------------------------
 * Every rank owns a mailbox in uncached device memory, mapped into every peer through hipIpc (espm_xchg_handle ->
 * exchange the 64-byte handles by any means -> espm_xchg_connect).  espm_xchg_post copies the record staged at
 * espm_xchg_staging() into slot [seq & 1][rank] of EVERY rank's mailbox over the direct links and raises a flag there;
 * espm_xchg_wait returns (on the stream) once the flags of all ranks have reached seq - bounded: a peer that never
 * delivers is counted (espm_xchg_timeouts), not waited for.  espm_xchg_records(parity) is then what an all-gather would
 * have produced: world records in rank order.  Sequence numbers start at 1 and grow by one per exchange on every rank.
 * Contexts are opaque and owned by the library (the one allocation it makes: peers must be able to map it). */
typedef struct espm_xchg espm_xchg;
#define ESPM_XCHG_HANDLE_BYTES 64
int espm_xchg_create(int world, int rank, size_t record_bytes, espm_xchg** out);
int espm_xchg_handle(const espm_xchg* x, void* handle_out /* ESPM_XCHG_HANDLE_BYTES */);
int espm_xchg_connect(espm_xchg* x, const void* handles /* world * ESPM_XCHG_HANDLE_BYTES, rank order */);
void* espm_xchg_staging(const espm_xchg* x);
const void* espm_xchg_records(const espm_xchg* x, int parity);
int espm_xchg_post(espm_xchg* x, uint32_t seq, espm_stream_t stream);
int espm_xchg_wait(espm_xchg* x, uint32_t seq, espm_stream_t stream);
int espm_xchg_timeouts(const espm_xchg* x, uint32_t* count_out);   /* host-synchronous read of the give-up counter */
/* How a flag follows its record's stores: 0 (default) a relaxed system-scope store behind the drain of the write-through data
 * stores and the workgroup's barrier; 1 a release store at system scope.  The initial value is 1 when the environment holds
 * ESPM_XCHG_ORDER=release at espm_xchg_create.  Every rank must use the same order only in the sense that each protects its
 * OWN records; mixing is harmless.  (csrc/mu_xchg.hip: the ordering contract.) */
int espm_xchg_set_order(espm_xchg* x, int release);
int espm_xchg_order(const espm_xchg* x);
int espm_xchg_destroy(espm_xchg* x);

/* The sharded W step after the accumulation in ONE launch (where espm_mu_w_update_is_local; otherwise the four calls
 * espm_mu_w_reduce_pack -> espm_xchg_post -> espm_xchg_wait -> espm_mu_shard_combine_finish): every workgroup of the slab
 * reduction delivers its 32 entries of A to all ranks itself, waits for the same piece of every rank, sums them in rank
 * order and updates its entries of W; the statistics of the new H block go to every rank, its boundary rows to the
 * neighbours.  Pieces and statistics travel as 8-byte granules {value, sequence number} in an area of the mailbox of their
 * own (value and "it is there" in one store); afterwards the records of espm_xchg_records(x, seq & 1) hold what the NEXT
 * launch reads in place - the neighbours' boundary rows (and this rank's own statistics) - not the pieces of A, which went
 * straight into st->a.  The grid need not be resident at once: workgroups are dispatched in index order, each posts before it
 * waits, and waits only for the workgroup of its own index on the other ranks (csrc/mu_w_exchange.hip). */
int espm_mu_shard_exchange_finish(const espm_mu_state* st, espm_xchg* x, uint32_t seq, int src, int slot, espm_stream_t stream);

/* espm_mu_iterate with HIP events on the launch stream around the launches of every iteration (diagnostics: bench.py's roofline line).
 * first_ms[i]: iteration i's first launch (the H update; with the W accumulation where the fused kernel applies), rest_ms[i]: what
 * follows it up to the new W.  Host arrays of n_iter floats, 1 <= n_iter <= 4096; synchronises the stream before it returns.  The loop
 * is the one espm_mu_iterate runs (same launches, same order, enqueued from C: the device never waits for the host). */
int espm_mu_iterate_timed(espm_mu_state* st, int n_iter, float* first_ms, float* rest_ms, espm_stream_t stream);

/* n_iter iterations of a SHARDED image (pixel rows split over the ranks of x) without host synchronisation and without a
 * host-side collective: per iteration espm_mu_step_hw, espm_mu_w_reduce_pack into the staged record, espm_xchg_post /
 * _wait, espm_mu_shard_combine_finish on the gathered records; the halo rows of the next H-step are the neighbours'
 * records in the mailbox.  *seq is the exchange counter (in: last used, out: last used); every rank makes the same calls. */
int espm_mu_iterate_sharded(espm_mu_state* st, espm_xchg* x, uint32_t* seq, int n_iter, int final_loss, espm_stream_t stream);

/* nu (p) with sum_i max(num_ij / (nu_j + den_ij), log_shift) = 1.  num (k, p), den (k, den_cols)
 * with den_cols in {1, p}, fp64 device arrays.  status_out (device int32): number of columns
 * that violate the preconditions (dicotomy.py:17-19). */
int espm_dichotomy_simplex(const double* num, const double* den, int k, int p, int den_cols,
                           double log_shift, double tol, int maxit, double* nu_out,
                           int32_t* status_out, espm_stream_t stream);

/* The H update's per-pixel multiplier search as a launch of its own: the fp32 routine espm_mu_step_h / espm_mu_step_hw inline
 * (dicotomy.py:4-55 per column, solved in the shifted unknown delta = nu + min{den_i : num_i > 0}; csrc/mu_common.hpp: simplex_root).
 * num, den (k, p) fp32 device arrays -> delta_out (p), e_out (k, p) = the shifted denominators: the update is
 * max(num / (delta + e), log_shift).  fast_exit != 0: the confirming evaluation is left out where the Newton step's predicted
 * residual is inside tol (what the H update does).  status_out as in espm_dichotomy_simplex.  k within this library's range. */
int espm_simplex_root_f32(const float* num, const float* den, int k, int p, float log_shift, float tol, int maxit, int fast_exit,
                          float* delta_out, float* e_out, int32_t* status_out, espm_stream_t stream);

/* The other two multipliers of espm/estimators/dicotomy.py as module-level functions (fp64 device arrays, per-column
 * convergence): acc (dicotomy.py:57-82): sum_k max(sqrt((b_kj + nu_j)^2 + 4 a c_kj) - nu_j - b_kj, 2 a eps) = 2 a with b
 * (k, b_cols in {1, p}), minus_c (k, p) >= 0; pg (dicotomy.py:84-108): sum_k max(a_kj + nu_j, eps) = 1 with a (k, p). */
int espm_dichotomy_simplex_acc(double a, const double* b, const double* minus_c, int k, int p, int b_cols, double log_shift,
                               double tol, int maxit, double* nu_out, int32_t* status_out, espm_stream_t stream);
int espm_dichotomy_simplex_pg(const double* a, int k, int p, double log_shift, double tol, int maxit, double* nu_out,
                              espm_stream_t stream);

/* Frobenius ("l2") branch of the step functions, espm/estimators/updates.py:109-118 (H) and :31-36 (W); in the reference
 * reachable by calling multiplicative_step_h / _w with l2=True (espm/tests/test_updates.py:457-568) and, for the W step,
 * from a fit with algo="l2_surrogate", l2=True (smooth_nmf.py:404-413).  f32 store, xscale = 1; the H step also needs
 * lambda_L = 0, mu = NULL (the W step does not look at them).  work: (2, KP, KP) device floats (GW^T GW, then H H^T);
 * scratch: device doubles for the partial Gram sums (>= KP * KP, more = more workgroups).
 *   l2_step_h: H' = max(H * (GW^T X) / ((GW^T GW) H + nu), eps), simplex_h / fixed_h as in espm_mu_step_h; h[src] -> h[1-src].
 *   l2_step_w: W' = max(W / (G^T G W H H^T) * (G^T (X H^T)), eps), fixed_w; H = h_t (the caller keeps it current);
 *              gtg = G^T G (m, m) when G is given (a property of G alone: formed once by the caller); w[src] -> w[1-src]. */
int espm_mu_l2_step_h(const espm_mu_state* st, int src, float* work, double* scratch, int scratch_doubles, espm_stream_t stream);
int espm_mu_l2_step_w(const espm_mu_state* st, int src, const float* gtg, float* work, double* scratch, int scratch_doubles,
                      espm_stream_t stream);
/* The W step in two halves, for a sharded image: _partials leaves this rank's X H^T in st->a ((k, n_pad) fp32) and its
 * H H^T in work[KP*KP ..] (KP x KP fp32) - both plain sums over the rank's pixels, which the caller adds over the ranks -
 * and _finish forms W' from them.  espm_mu_l2_step_w is the two in a row. */
int espm_mu_l2_w_partials(const espm_mu_state* st, float* work, double* scratch, int scratch_doubles, espm_stream_t stream);
int espm_mu_l2_w_finish(const espm_mu_state* st, int src, const float* gtg, const float* work, espm_stream_t stream);

/* Terms of the linesearch on the Laplacian surrogate (espm/estimators/surrogates.py:65-149, smooth_nmf.py:376-381)
 * between two H buffers, Ht = h[hold] (before the update) and H = h[hnew]: out (4 + ESPM_KP device doubles) =
 * [sum Ht (Ht L), sum (Ht L) H, sum H (H L), sum (Ht - H)^2, dg_0 .. dg_7] with dg_k = sum_j Ht log(Ht / H) - Ht + H.
 * The caller forms d = 1/2 (2 out[1] - out[0] + gamma t3) - 1/2 out[2] with t3 = sum_k max_j H_kj dg_k (log surrogate,
 * Bregman) or t3 = out[3] (quadratic surrogate) - lambda_L = 1 as the reference calls it - and lowers gamma by 1.05
 * when d > 0, else raises it by 1.5.  Uses st->hpart as scratch: call it between
 * espm_mu_h_finalize and the next espm_mu_step_h.  One GPU only. */
int espm_mu_linesearch_terms(const espm_mu_state* st, int hold, int hnew, double* out, espm_stream_t stream);

/* The same for a rank of a sharded image: the terms of its block of image rows (the caller sums the `out` of the ranks, in
 * rank order).  The image rows above / below the block come from the neighbours' boundary rows: those of the new H from
 * st->halo_top / halo_bot, those of the H before the update from old_halo_top / old_halo_bot ((k, ny) fp32 each - the
 * previous exchange's records still hold them, the exchange being double buffered); null exactly where st's are. */
int espm_mu_linesearch_terms_sharded(const espm_mu_state* st, int hold, int hnew, const float* old_halo_top, const float* old_halo_bot,
                                     double* out, espm_stream_t stream);

/* The same terms without a state (module-level surrogates, espm/estimators/surrogates.py): h_old, h_new (k, ld) fp32 with p
 * used columns, grid (nx, ny) when grid_mode != 0 else L = identity; part: scratch of (4 + KP) * ceil(p / 512) doubles. */
int espm_surrogate_terms(const float* h_old, const float* h_new, int k, int p, int64_t ld, int nx, int ny, int grid_mode, double* part,
                         int part_doubles, double* out, espm_stream_t stream);

/* out = H @ L for the 5-point Laplacian on an (nx, ny) grid (k, nx*ny) with leading dim ld. */
int espm_mu_laplacian(const float* h, int k, int nx, int ny, int64_t ld, float* out,
                      espm_stream_t stream);

/* ---- initialisation on the device (host side: espm_amd/init_device.py) ----------------------------------
 * The LU normaliser of the randomized range finder behind the reference's NNDSVD initialisation
 * (espm/estimators/updates.py:179 -> sklearn _initialize_nmf -> _randomized_range_finder, power_iteration_normalizer "LU":
 * `Q, _ = scipy.linalg.lu(A, permute_l=True)`), called 2 * n_iter = 14 times per fit on matrices of n_components + 10 columns.
 * out (m, r) contiguous = P L of A = P L U, partial pivoting with LAPACK's pivot choice (largest modulus, first row on ties).
 * a: (m, r) with leading dimension ld, dtype ESPM_SRC_F32 / ESPM_SRC_F64 (out has the same); m >= r, r <= 64.
 * scratch: espm_lu_pl_scratch_bytes(m, r, dtype) bytes of device memory, contents irrelevant.  r + 1 launches on `stream`. */
size_t espm_lu_pl_scratch_bytes(int m, int r, int dtype);
int espm_lu_pl(const void* a, int dtype, int m, int r, int64_t ld, void* out, void* scratch, size_t scratch_bytes, espm_stream_t stream);

/* ---- fp64 mode (csrc/mu_fp64.hip; MUEngine(precision="fp64"), NMFEstimator.set_precision("fp64")) ------------------------------
 * The log_surrogate multiplicative updates in fp64 with the reference's simplex bisection (dicotomy.py:4-55, :111-173: global stop).
 * Plain fp64 device arrays, no espm_mu_state: W (M, k), G W (n, k) and R H^T (n, k) row-major, H (k, p), X (n, p) channel-major in
 * the store x_type (ESPM_F64_X_*), every value exact; the effective X is (double) x * xscale.  Reductions run in a fixed order
 * (per-workgroup partials, then one workgroup): a fit is bit-identical from run to run.  Only the narrow build (1..8 components)
 * has the kernels; the wide builds return ESPM_EUNSUPPORTED from every one of these entry points. */
#define ESPM_F64_MAX_K 8
#define ESPM_F64_BLOCK 256     /* pixels per H-pass workgroup; entries per workgroup of the other reductions                   */
#define ESPM_F64_CHUNK 2048    /* channels of G W staged in LDS per round of the H pass (k = 8: 128 KB)                         */
#define ESPM_F64_WCHUNK 4096   /* pixels per workgroup of the W accumulation                                                  */
#define ESPM_F64_MAXIT 127     /* bisection sweeps at most (the step bitmask is 128 bits)                                     */
#define ESPM_F64_X_U8 0
#define ESPM_F64_X_BF16 1
#define ESPM_F64_X_F32 2
#define ESPM_F64_X_F64 3

/* Scratch (doubles) the H pass, espm_f64_hstat, espm_f64_rel and espm_f64_w_accum need for p pixels / count entries. */
int64_t espm_f64_scratch_doubles(int n, int p, int k, int64_t count);
/* G W (n, k) = G (n, m) W (m, k), or W itself with g == NULL (m = n); its column sums (k) and *small = 1 when an entry of G W is
 * below log_shift (the loss then clamps G W, measures.py:493-504).  One launch plus one workgroup. */
int espm_f64_gw(const double* g, const double* w, int n, int m, int k, double log_shift, double* gw, double* colsum, int32_t* small,
                espm_stream_t stream);
/* out (2k): [0, k) sum_j max(H_ij, log_shift), [k, 2k) max_j max(H_ij, log_shift) (updates.py:98-105, :139). */
int espm_f64_hstat(const double* h, int k, int p, double log_shift, double* scratch, double* out, espm_stream_t stream);
/* One pass over X for the state (G W, H): hist_row[0..3) = sum(Y - max(X, eps) log Y) over the clamped factors, sum mu_i log(H + eps_reg),
 * sum H * (H L) (base.py:197-203, measures.py:524-577).  mode 0: only that; 1: also h_out = the H update without a simplex
 * (updates.py:83-156, fixed_h entries >= 0 kept); 2: also num, den (k, p) of the update for espm_f64_bisect.  nx * ny == p: the
 * 5-point grid Laplacian, nx == 0: the identity.  hstat: espm_f64_hstat of h (its maxima are read when lambda_L != 0). */
int espm_f64_h_pass(const void* x, int x_type, int n, int p, double xscale, const double* gw, const double* colsum_gw,
                    const int32_t* gw_small, const double* h, int k, const double* hstat, const double* mu, double eps_reg,
                    double lambda_L, double sigma, int nx, int ny, double log_shift, int mode, const double* fixed_h, double* h_out,
                    double* num, double* den, double* scratch, double* hist_row, espm_stream_t stream);
/* The simplex multiplier of every pixel by the reference's bisection with its global stop, in two launches: every column bisects
 * to maxit and ANDs the bitmask of the steps at which its |f| <= tol into mask (2 words); then every column recomputes its midpoint
 * to the lowest common step and writes h_out = max(num / (den + nu), log_shift) (fixed_h entries >= 0 kept).  *status counts the
 * columns that violate the reference's preconditions (dicotomy.py:17-19, :141-144).  maxit <= ESPM_F64_MAXIT. */
int espm_f64_bisect(const double* num, const double* den, int k, int p, double log_shift, double tol, int maxit,
                    const double* fixed_h, double* h_out, uint64_t* mask, int32_t* status, espm_stream_t stream);
/* *out = max |a - b| / (a + tol mean(a)) over count entries (base.py:323-324). */
int espm_f64_rel(const double* a, const double* b, int64_t count, double tol, double* scratch, double* out, espm_stream_t stream);
/* rh (n, k) = (X / Y) max(H, eps)^T with Y = G W max(H, eps) (updates.py:50-59). */
int espm_f64_w_accum(const void* x, int x_type, int n, int p, double xscale, const double* gw, const double* h, int k, double log_shift,
                     double* scratch, double* rh, espm_stream_t stream);
/* The W update from rh (updates.py:58-76): w_out = max(W (G^T rh) / (colsum(G) rowsum(H) + nu), log_shift), nu by the reference's
 * bisection over the rows (rows != NULL: the physics model's rows, a mask of M bytes with nrows set; else nrows = M) when
 * simplex != 0; fixed_w entries >= 0 kept.
 * g == NULL: the identity (M = n).  hstat: espm_f64_hstat of the H the update uses.  One workgroup. */
int espm_f64_w_finish(const double* rh, const double* g, const double* colsum_g, int n, int m, int k, const double* w,
                      const double* hstat, int simplex, const uint8_t* rows, int nrows, double log_shift, double tol, int maxit,
                      const double* fixed_w, double* w_out, int32_t* status, espm_stream_t stream);

/* ---- fp64 mode, sparse store (csrc/mu_fp64_sparse.hip; x_store = "sparse" of the fp64 engine, built by espm_amd/sparse64.py) ------
 * A count image (non-negative integers up to ESPM_F64S_MAX_COUNT, n <= ESPM_F64S_MAX_N channels) kept as its non-zero elements,
 * one dword each, count << 16 | index, the raw count (the kernels multiply by xscale), in two orders:
 *   H order  by pixel.  The lists of the 64 consecutive pixels 64 g .. 64 g + 63 ("group" g) are interleaved dword-wise: element r
 *            of pixel 64 g + l is h_elem[h_off[g] + 64 r + l]; index = channel, ascending within a list; a list shorter than the
 *            longest of its group is padded with 0 (no element has count 0).  h_off: ceil(p / 64) + 1 dword offsets (int64).
 *   W order  by (block b of ESPM_F64S_WBLOCK pixels, channel c), plain CSR: list b * n + c is w_elem[w_off[b n + c] .. w_off[b n + c + 1]),
 *            index = pixel - b * ESPM_F64S_WBLOCK, ascending.  w_off: ceil(p / ESPM_F64S_WBLOCK) * n + 1 offsets (int64).
 * Both orders hold the same elements.  Lines without a count are not in the store; the engine records them (base.py:519-528 fills
 * them with log_shift) and the kernels apply that fill, every filled entry being log_shift * xscale:
 *   ec (n_ec channel indices, ascending) / ec_flag (n bytes)           the empty channels
 *   ep (pixel indices, ascending) / ep_flag (p bytes) / ep_off (ceil(p / ESPM_F64S_WBLOCK) + 1 offsets into ep, per W block)
 *                                                                      the empty pixels; all NULL (n_ec = 0) without the fill.
 * The reference's zeros that are not zeros: the loss clamps X, so a zero entry of a kept line adds -log_shift log Y: the H pass sums
 * log Y over every channel of a pixel without reading X (fp32 log of the fp64 Y, fp64 sum; its 1e-7 relative error enters the loss at
 * 1e-21) and takes the elements' own fp64 logs off it.  An empty channel's row adds log_shift xscale G W[c, :] / Y to every pixel's
 * numerator (fp32 reciprocal: 1e-7 of a 1e-14 term) and is the whole of rh[c, :], which the W pass therefore computes in fp64 over
 * every pixel.  An empty pixel's column is the whole of that pixel's numerator: fp64 in both passes.
 * Same contracts as espm_f64_h_pass / espm_f64_w_accum otherwise; fixed-order reductions; ESPM_EUNSUPPORTED from the wide builds. */
#define ESPM_F64S_MAX_COUNT 65535
#define ESPM_F64S_MAX_N 65536
#define ESPM_F64S_HBLOCK 512       /* pixels (threads) per H-pass workgroup                                                    */
#define ESPM_F64S_WBLOCK 65536     /* pixels per block of the W order                                                          */
#define ESPM_F64S_LDS_BYTES 163840 /* G W (n k doubles) is staged in LDS by the H pass up to this size, read through L2 above   */

/* Scratch (doubles) of the two entry points below; the engine allocates the larger of this and espm_f64_scratch_doubles. */
int64_t espm_f64_sparse_scratch_doubles(int n, int p, int k);
int espm_f64_sparse_h_pass(const uint32_t* h_elem, const int64_t* h_off, const int32_t* ec, int n_ec, const uint8_t* ep_flag, int n, int p,
                           double xscale, const double* gw, const double* colsum_gw, const int32_t* gw_small, const double* h, int k,
                           const double* hstat, const double* mu, double eps_reg, double lambda_L, double sigma, int nx, int ny,
                           double log_shift, int mode, const double* fixed_h, double* h_out, double* num, double* den, double* scratch,
                           double* hist_row, espm_stream_t stream);
int espm_f64_sparse_w_accum(const uint32_t* w_elem, const int64_t* w_off, const uint8_t* ec_flag, const int32_t* ep, const int32_t* ep_off,
                            int n, int p, double xscale, const double* gw, const double* h, int k, double log_shift, double* scratch,
                            double* rh, espm_stream_t stream);

/* ---- pixel diagnostics (csrc/mu_diag.hip; espm_amd.measures.pixel_diagnostics, NMFEstimator.pixel_diagnostics) ---------------
 * Where a fitted model fails and how well every abundance is known, in one fp64 pass over X.  Plain device pointers, no
 * espm_mu_state.  x: the image as it was measured, dtype ESPM_DIAG_X_*, (n, p) for x_layout ESPM_LAYOUT_CM or (p, n) for
 * ESPM_LAYOUT_PM, leading dimension ld (elements).  d (n, k) row-major: the spectra G W in counts; h (k, p).
 * With Y = max(d h, log_shift), per pixel j:
 *   dev[j]       = 2 sum_c (x ln(x / y) - x + y), the first term 0 where x == 0: the Poisson (KL) deviance
 *   F_j          = d^T diag(1 / y[:, j]) d, the expected Fisher information of h[:, j] with the spectra held
 *   h_std[:, j]  = sqrt(diag(C_j)), C = F^-1, or with simplex != 0 the bound under sum_i h_i = 1:
 *                  C = F^-1 - F^-1 1 1^T F^-1 / (1^T F^-1 1) (exactly 0 for k = 1)
 * F_j is factorised by the root-free Cholesky F = L diag(piv) L^T; a pivot that is not above k * 2^-52 * max diag(F_j) makes that
 * pixel's column of h_std NaN and counts in *n_singular (may be NULL; zeroed by the call) - no error.  dev (p), h_std (k, p).
 * k = 1..ESPM_DIAG_MAX_K; one launch on `stream`, nothing but that integer count is accumulated atomically.  Only the narrow
 * build has the kernels; the wide builds return ESPM_EUNSUPPORTED. */
#define ESPM_DIAG_MAX_K 8
#define ESPM_DIAG_BLOCK 256    /* pixels (threads) per workgroup                                                              */
#define ESPM_DIAG_CHUNK 256    /* channels of d staged in LDS per round (k = 8: 16 KB)                                        */
#define ESPM_DIAG_X_U8 0
#define ESPM_DIAG_X_U16 1
#define ESPM_DIAG_X_F32 2
#define ESPM_DIAG_X_F64 3
int espm_pixel_diagnostics(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int k,
                           double log_shift, int simplex, double* dev, double* h_std, int32_t* n_singular, espm_stream_t stream);

/* ---- channel diagnostics (csrc/mu_diag_chan.hip; espm_amd.measures.spectral_diagnostics, NMFEstimator.spectral_diagnostics) ----
 * The transpose side of the pixel diagnostics: in which energy channels a fitted model fails and how well every spectrum is known,
 * in one fp64 pass over X that reduces over the pixels.  x, x_dtype (ESPM_DIAG_X_*), x_layout, ld, d (n, k), h (k, p) and log_shift
 * are exactly as for espm_pixel_diagnostics.  With Y = max(d h, log_shift), per channel c (all outputs fp64):
 *   dev[c]       = 2 sum_p (x ln(x / y) - x + y), the first term 0 where x == 0: the residual spectrum
 *   xsum[c]      = sum_p x, the measured sum spectrum (exact for counts: the sums stay below 2^53)
 *   ysum[c]      = sum_p y, the modelled sum spectrum
 *   m_tri[c, t]  (n, k (k + 1) / 2): the lower triangle, row by row ((0,0), (1,0), (1,1), (2,0), ...), of
 *                  M_c = sum_p h_p h_p^T / y_cp, the expected Fisher information of row c of d with the abundances held.  The
 *                  information of W in d = G W follows without another pass: F = sum_c (g_c g_c^T) (x) M_c.
 * A workgroup takes ESPM_CDIAG_BLOCK channels (one per thread) and ESPM_CDIAG_PCHUNK pixels and writes its partial sums to
 * `scratch` (device memory, espm_channel_diagnostics_scratch(n, p, k) bytes: chunks x (3 + k (k + 1) / 2) x n doubles); a second
 * launch on `stream` adds the chunks in ascending order.  Nothing is accumulated atomically: two calls give the same bits, and so
 * do the two layouts of one image.  k = 1..ESPM_DIAG_MAX_K.  ESPM_EINVAL for a null pointer, a layout or dtype that does not
 * exist, ld below the row length, n or p below 1, or scratch_bytes below what the query returns (the message names both sizes).
 * Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED, and their query returns 0. */
#define ESPM_CDIAG_BLOCK 256     /* channels (threads) per workgroup                                                          */
#define ESPM_CDIAG_PCHUNK 2048   /* pixels per workgroup: 2048 channels x 512^2 pixels are 8 x 128 workgroups                  */
int espm_channel_diagnostics(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int k,
                             double log_shift, double* dev, double* xsum, double* ysum, double* m_tri, void* scratch,
                             size_t scratch_bytes, espm_stream_t stream);
size_t espm_channel_diagnostics_scratch(int n, int p, int k);

/* ---- pixel binning (csrc/mu_binning.hip; espm_amd.binning, NMFEstimator.fit_binned) ----
 * The image is ny x nx pixels, row-major (pixel y * nx + x), n channels: x, x_dtype (ESPM_DIAG_X_*), x_layout and ld as for the
 * diagnostics, with p = ny * nx.  A bin (by, bx), both >= 1, puts pixel (y, x) into bin (y / by, x / bx) of a grid of
 * ceil(ny / by) x ceil(nx / bx) bins; the factors need not divide the image (the last bin row and column hold fewer pixels, n_g of
 * them) and a factor above the axis is the whole axis.  S_gc is the sum of x over the pixels of bin g in channel c.
 *   espm_rebin_pixels   out[c, g] = S_gc in the input's layout on the binned grid - (n, bins) with rows out_ld apart for
 *                       ESPM_LAYOUT_CM, (bins, n) for ESPM_LAYOUT_PM - as out_dtype ESPM_DIAG_X_F32 or ESPM_DIAG_X_F64.  Integer input is
 *                       summed exactly in integers, floating-point input in fp64; rounded once on the store.  One launch.
 *   espm_binning_sums   bins: a HOST array of n_bins (by, bx) pairs.  out (device, 2 + 2 n_bins doubles): T1 = sum x and T2 = sum x^2
 *                       over the cube, then per candidate A = sum_gc S_gc^2 / n_g and C = sum_gc S_gc / n_g - what the risk estimate
 *                       of eds_spim.py:787-793 is made of: with K = p, L = n, var = C / (K L), bias = (T2 - T1 - A + C) / (K L),
 *                       risk = var K / L + bias.  One pass over X per candidate and one for the totals, each by ESPM_BIN_PARTS
 *                       workgroups that write their partial sums to `scratch` (device, espm_binning_sums_scratch(n, ny, nx, n_bins)
 *                       bytes: (2 + 2 n_bins) x ESPM_BIN_PARTS doubles, and 128 x ESPM_BIN_PARTS more
 *                       through which a pixel-major candidate with few, large bins goes in slabs of image rows that a second launch
 *                       joins); a last launch adds the partial sums in ascending order.
 * Nothing is accumulated atomically and every order of additions follows from the shapes alone: two calls give the same bits.
 * ESPM_EINVAL, before the device is touched, for a null pointer, a layout or dtype that does not exist, ld or out_ld below the row
 * length, n, ny or nx below 1, 2^31 pixels or more, a factor below 1, n_bins below 1, or scratch_bytes below what the query returns
 * (the message names both sizes).  Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED, and their query
 * returns 0. */
#define ESPM_BIN_BLOCK 256     /* threads per workgroup: columns of a strip (channel-major), 64 channels x 4 (pixel-major)       */
#define ESPM_BIN_PARTS 2048    /* workgroups, and partial sums per slot of the scratch, of every launch of espm_binning_sums  */
int espm_rebin_pixels(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int ny, int nx, int by, int bx, void* out,
                      int out_dtype, int64_t out_ld, espm_stream_t stream);
int espm_binning_sums(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int ny, int nx, const int32_t* bins, int n_bins,
                      double* out, void* scratch, size_t scratch_bytes, espm_stream_t stream);
size_t espm_binning_sums_scratch(int n, int ny, int nx, int n_bins);

/* ---- count splitting (csrc/mu_split.hip; espm_amd.splitting, NMFEstimator.fit_split) ----
 * If x ~ Poisson(l) and x_a ~ Binomial(x, q), then x_a ~ Poisson(q l) and x_b = x - x_a ~ Poisson((1 - q) l), independent: one count
 * image gives a training image and a held-out image of the same specimen.  Plain device pointers, no espm_mu_state.  x, x_layout and ld
 * as for the diagnostics, x_dtype ESPM_DIAG_X_U8 or ESPM_DIAG_X_U16; x holds the pixels j0 .. j0 + p - 1 of an image of p_total pixels
 * (the whole image: j0 = 0, p_total = p).
 * THE RULE (the split is defined by it, not by the kernels).  The image is logically (n, p_total), channel-major: element (c, j) has the
 * 64-bit index e = c * p_total + j - in either layout, in any slab.  Draw d = 0 .. x - 1 of element e is word (d mod 4) of
 * Philox4x32-10 (Salmon et al. 2011) with the counter (e low 32, e high 32, d div 4, 0) and the key (seed low 32, seed high 32); count
 * d goes to part A iff its word < q_threshold, 1 <= q_threshold <= 2^32 - 1: the fraction is q_threshold / 2^32 exactly.  x_a is the
 * number of such d, x_b = x - x_a.
 *   espm_thin_counts     xa, xb (xb may be NULL): the two parts in x's dtype and layout, rows out_ld apart.  One launch.  A zero entry
 *                        costs its read, another one ceil(x / 4) Philox calls; an entry of ESPM_SPLIT_HEAVY or more is drawn by its
 *                        whole wave, each lane taking blocks of four draws.
 *   espm_split_deviance  d (n, k) row-major and h (k, p): the model of the TRAINING part (G W and H of a fit of x_a).  x_a is regenerated
 *                        from (x, seed) by the rule - x_b is never stored.  With Y = max(d h, log_shift) and r = (2^32 - q_threshold) /
 *                        q_threshold, per pixel j (terms x ln(x / .) are 0 where x == 0):
 *                          dev_a[j] = 2 sum_c (x_a ln(x_a / Y) - x_a + Y)          the in-sample deviance
 *                          dev_b[j] = 2 sum_c (x_b ln(x_b / (r Y)) - x_b + r Y)    the held-out deviance
 *                          cnt_b[j] = sum_c x_b                                    (int64: exact)
 *                        All arithmetic in fp64, a pixel per thread, the sums in channel order; k = 1..ESPM_SPLIT_MAX_K.  One launch.
 * Nothing is accumulated atomically: two calls give the same bits, and so do the two layouts of one image.  ESPM_EINVAL, before the
 * device is touched and with the offending values in the message, for a null pointer, a layout that does not exist, a dtype other than
 * u8 / u16, ld or out_ld below the row length, n or p below 1, a slab outside 0 .. p_total, q_threshold outside 1 .. 2^32 - 1, k
 * outside 1..ESPM_SPLIT_MAX_K, log_shift not positive.  Only the narrow build has the kernels; the wide builds return
 * ESPM_EUNSUPPORTED. */
#define ESPM_SPLIT_BLOCK 256   /* threads per workgroup: entries of a row (thinning), pixels (deviance)                          */
#define ESPM_SPLIT_HEAVY 256   /* counts from which the wave shares an entry's draws (16-bit images only)                       */
#define ESPM_SPLIT_MAX_K 32
int espm_thin_counts(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int64_t p_total, int64_t j0, int64_t q_threshold,
                     uint64_t seed, void* xa, void* xb, int64_t out_ld, espm_stream_t stream);
int espm_split_deviance(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int64_t p_total, int64_t j0, int64_t q_threshold,
                        uint64_t seed, const double* d, const double* h, int k, double log_shift, double* dev_a, double* dev_b,
                        int64_t* cnt_b, espm_stream_t stream);

/* ---- Poisson sampling (csrc/mu_sample.hip; espm_amd.sampling, NMFEstimator.simulate / calibrate_deviance / bootstrap) ----
 * A count image drawn from a model: d (n, k) row-major, the spectra G W in counts, and h (k, p), the abundances of the pixels j0 .. j0 + p - 1
 * of an image of p_total pixels (the whole image: j0 = 0, p_total = p).  Plain device pointers, no espm_mu_state.
 * THE RULE (the sample is defined by it, not by the kernels).  The image is logically (n, p_total), channel-major: element (c, j) has the
 * 64-bit index e = c * p_total + j - in either layout, in any slab - as in count splitting.
 *   rate     y = sum_i d[c, i] h[i, j] in fp64, i ascending from 0, starting from +0; every product and every sum is rounded on its own (NO
 *            fused multiply-add), so that a plain host loop gets the same bits of y and no libm function enters the rule.  y not finite
 *            or negative: the entry is 0 and counted INVALID.  y > ESPM_SAMPLE_MAX_RATE: the entry is the dtype's maximum and counted
 *            SATURATED; no draw is made for it.
 *   words    block b of element e is Philox4x32-10 (Salmon et al. 2011) with the counter (e low 32, e high 32, b, replicate + 1) and the key
 *            (seed low 32, seed high 32); replicate = 0 .. 2^32 - 2, so the fourth counter word is never 0: count splitting has 0 there,
 *            and thinning a simulated image with the same seed shares no word with the sampler.
 *   unit     a word w gives N(w) = #{ i in 0 .. 11 : w >= T_i } ~ Poisson(1), with T_i = floor(2^32 sum_{j <= i} e^-1 / j!):
 *              5e2d58d8 bc5ab1b1 eb715e1d fb239797 ff1025f5 ffd90f3b fffa8b71 ffff540c ffffed1f fffffe21 ffffffd4 fffffffc
 *            (mean 1 + 1.4e-9, variance 1 + 1.3e-8).
 *   count    m = floor(y), thr = floor((y - m) 2^32), both exact in fp64.  With word_i = word (i mod 4) of block (i div 4) and
 *            N0 = N(word_0):
 *              x = sum_{i < m} N(word (i mod 4) of block (4 + i div 4))  +  #{ i in 1 .. N0 : word_i < thr }
 *            - m unit pieces, and a Poisson(1) thinned to the fractional part (N0 <= 12: blocks 0 .. 3 serve it).  x ~ Poisson(y) up to
 *            the 2^-32 quantisation of the fraction.  An x above the output dtype's maximum is stored as that maximum and counted SATURATED.
 *   espm_poisson_sample   x: the replicate as x_dtype ESPM_DIAG_X_U8 or ESPM_DIAG_X_U16, (n, p) for ESPM_LAYOUT_CM or (p, n) for
 *                        ESPM_LAYOUT_PM, rows ld apart.  counts[0] = saturated entries, counts[1] = invalid entries (zeroed by the call,
 *                        on `stream`).  One launch: a pixel per thread, an entry of m >= ESPM_SAMPLE_HEAVY unit pieces is drawn by its whole
 *                        wave.  The values use no atomics; the two counters are integer sums: exact, the same from call to call.
 *   espm_sample_deviance  dev (n_rep, p): for replicate r = replicate0 .. replicate0 + n_rep - 1 and pixel j, with Y = max(y, log_shift)
 *                        (a NaN rate stays NaN) and x the rule's draw as espm_poisson_sample stores it at 16 bits (invalid: 0,
 *                        saturated: 65535), dev = 2 sum_c (x ln(x / Y) - x + Y), the first term 0 where x == 0.  The image is never
 *                        stored.  The sums run in channel order in the pixel's own thread: two calls give the same bits.  One launch.
 * k = 1..ESPM_SAMPLE_MAX_K.  ESPM_EINVAL, before the device is touched and with the offending values in the message, for a null pointer,
 * k outside 1..ESPM_SAMPLE_MAX_K, n or p below 1, a slab outside 0 .. p_total, n x p_total beyond a 64-bit index, ld below the row
 * length, a dtype other than u8 / u16, a layout that does not exist, replicate (or replicate0 + n_rep - 1) outside 0 .. 2^32 - 2,
 * n_rep below 1, log_shift not positive.  Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED. */
#define ESPM_SAMPLE_BLOCK 256        /* pixels (threads) per workgroup                                                          */
#define ESPM_SAMPLE_HEAVY 256        /* unit pieces from which the wave shares an entry's draws                                 */
#define ESPM_SAMPLE_MAX_RATE 65535   /* rates above it are not drawn: the entry saturates                                       */
#define ESPM_SAMPLE_MAX_K 32
int espm_poisson_sample(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, uint64_t seed, int64_t replicate,
                        void* x, int x_dtype, int x_layout, int64_t ld, int64_t* counts, espm_stream_t stream);
int espm_sample_deviance(const double* d, const double* h, int k, int n, int p, int64_t p_total, int64_t j0, uint64_t seed, int64_t replicate0,
                         int n_rep, double log_shift, double* dev, espm_stream_t stream);

/* ---- count attribution (csrc/mu_attrib.hip; espm_amd.attribution, NMFEstimator.attribute_counts / assign_counts) ----
 * How many of the MEASURED counts stand behind every component of a model d (n, k) row-major, the spectra G W in counts, and h (k, p).
 * Plain device pointers, no espm_mu_state; x, x_layout and ld as for the diagnostics.  y_cj = sum_i d[c, i] h[i, j].
 *   espm_attribute_expected  x as x_dtype ESPM_DIAG_X_* (u8, u16, f32, f64).  With Y = max(y, log_shift), all arithmetic in fp64:
 *                          num_h[i, j]  (k, p) = h[i, j] sum_c x_cj d[c, i] / Y_cj: the counts of pixel j attributed to component i (the EM
 *                                         responsibilities, the numerator of the multiplicative update of h); the sum runs in channel order
 *                                         in the pixel's own thread
 *                          ratio[c, i]  (n, k) = sum_j x_cj h[i, j] / Y_cj: d o ratio are the counts of channel c attributed to component i,
 *                                         and with d = G W, W o (G^T ratio) those behind every entry of W.  A workgroup takes
 *                                         ESPM_ATTRIB_BLOCK channels and ESPM_ATTRIB_PCHUNK pixels and writes its partial sums to `scratch`
 *                                         (device memory, espm_attribute_expected_scratch(n, p, k) bytes: chunks x k x n doubles); a last
 *                                         launch adds the chunks in ascending order
 *                          counts[j]    (p) = sum_c x_cj: int64_t (exact) for u8 / u16 x, double for f32 / f64 x
 *                        An entry with x == 0 costs its read only.  Three launches on `stream` (one pass over x per side, the reduction).
 *                        Nothing is accumulated atomically: two calls give the same bits, and so do the two layouts of one image.
 *   espm_assign_counts   x as ESPM_DIAG_X_U8 or ESPM_DIAG_X_U16, the pixels j0 .. j0 + p - 1 of an image of p_total pixels (the whole image:
 *                        j0 = 0, p_total = p), as for espm_thin_counts; h holds those p pixels.  parts: k images in x's dtype and layout,
 *                        image i at parts + i * part_stride (elements), rows out_ld apart; their sum is x exactly.  counts[0] (zeroed by
 *                        the call, on `stream`): the number of invalid entries.
 * THE RULE of espm_assign_counts (the parts are defined by it, not by the kernel).  The image is logically (n, p_total), channel-major:
 * element (c, j) has the 64-bit index e = c * p_total + j - in either layout, in any slab - as in count splitting.
 *   rates    s_0 = d[c, 0] * h[0, j], s_i = s_(i-1) + d[c, i] * h[i, j] in fp64: every product and every sum is rounded on its own (NO fused
 *            multiply-add), so that a plain host loop gets the same bits.  a = s_(k-1).
 *   invalid  x > 0 and a not a finite number above 0: all x counts go to component 0 and the entry is counted INVALID.
 *   words    count t = 0 .. x - 1 of a valid entry takes word (t mod 4) of Philox4x32-10 (Salmon et al. 2011) with the counter
 *            (e low 32, e high 32, 0x80000000 | (t div 4), 0) and the key (seed low 32, seed high 32).  Count splitting has t div 4 < 2^14 in
 *            the third word and Poisson sampling never 0 in the fourth: attributing a thinned or a simulated image under the same seed
 *            shares no word with the call that made it.
 *   count    with u = ((double)w * 2^-32) * a (the first product exact, the second rounded once), the count goes to the smallest i with
 *            u < s_i, and to k - 1 if there is none.
 * By the Poisson splitting theorem the parts of x ~ Poisson(a) are independent Poisson(d[c, i] h[i, j]) images.  One launch: channel-major x
 * a pixel per thread (h in registers, d through LDS), pixel-major x a channel per thread (d in registers, h through LDS); a zero entry
 * costs its read and its k stores, another one k products and ceil(x / 4) Philox calls; an entry of ESPM_ATTRIB_HEAVY or more is drawn
 * by its whole wave.  The parts use no atomics; the counter is an integer sum: exact, the same from call to call.
 * k = 1..ESPM_ATTRIB_MAX_K.  ESPM_EINVAL, before the device is touched and with the offending values in the message, for a null pointer,
 * k outside 1..ESPM_ATTRIB_MAX_K, n or p below 1, a dtype or layout that does not exist (espm_assign_counts: a dtype other than u8 / u16),
 * ld or out_ld below the row length, part_stride below one image, a slab outside 0 .. p_total, n x p_total beyond a 64-bit index,
 * scratch_bytes below what the query returns, log_shift not positive.  Only the narrow build has the kernels; the wide builds return
 * ESPM_EUNSUPPORTED, and their query returns 0. */
#define ESPM_ATTRIB_BLOCK 256     /* threads per workgroup: pixels, or channels                                                  */
#define ESPM_ATTRIB_PCHUNK 1024   /* pixels per workgroup of the channel side of espm_attribute_expected                         */
#define ESPM_ATTRIB_WALK 512      /* channels (channel-major) or pixels (pixel-major) a workgroup of espm_assign_counts walks    */
#define ESPM_ATTRIB_HEAVY 256     /* counts from which the wave shares an entry's draws (16-bit images only)                     */
#define ESPM_ATTRIB_MAX_K 32
int espm_attribute_expected(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int k,
                            double log_shift, double* num_h, double* ratio, void* counts, void* scratch, size_t scratch_bytes,
                            espm_stream_t stream);
size_t espm_attribute_expected_scratch(int n, int p, int k);
int espm_assign_counts(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int64_t p_total, int64_t j0, const double* d,
                       const double* h, int k, uint64_t seed, void* parts, int64_t part_stride, int64_t out_ld, int64_t* counts,
                       espm_stream_t stream);

/* ---- weighted marginals (csrc/mu_marginals.hip; espm_amd.marginals, NMFEstimator.line_maps / region_spectra) ----
 * Weighted sums of the image, of its model and of the deviance term along one axis, for g weight vectors at once: weights over the
 * channels give maps (an energy window, a background-corrected line, a top-hat filter), weights over the pixels give spectra (a phase
 * mask, a label map, abundances used as soft masks).  Plain device pointers, no espm_mu_state; x, x_dtype (ESPM_DIAG_X_*: u8, u16,
 * f32, f64), x_layout, ld, d (n, k) row-major, h (k, p) and log_shift exactly as for espm_pixel_diagnostics.
 *   side ESPM_MARG_PIXELS    wgt (g, n) row-major, one weight per channel; xs, ys, dev (g, p): the sums run over the channels
 *   side ESPM_MARG_CHANNELS  wgt (g, p) row-major, one weight per pixel;   xs, ys, dev (g, n): the sums run over the pixels
 * THE RULE (the outputs are defined by it), all in fp64.  Per entry (c, j) with the count x:
 *   y = 0; y = fma(d[c, i], h[i, j], y) for i ascending; Y = fmax(y, log_shift); r = 1.0 / Y; t = Y - x; if x > 0: t = fma(x, log(x * r), t)
 *   - the term exactly as the diagnostics form it.  Per group q, with w = wgt[q, the entry's summed index]:
 *   xs_q = fma(w, x, xs_q); ys_q = fma(w, Y, ys_q); dv_q = fma(w, t, dv_q);        the stored dev is 2 dv.
 * ORDER.  The pixel side adds the channels in ascending order, from 0, in the pixel's own thread.  The channel side adds the pixels
 * of a chunk of ESPM_MARG_PCHUNK in ascending order, from 0, and writes the partial sums to `scratch` (device memory,
 * espm_weighted_marginals_scratch(side, n, p, g) bytes: chunks x 3 x g x n doubles, whatever k is; 0 for the pixel side, whose
 * `scratch` may be NULL); a second launch adds the chunks in ascending order, from 0.  Nothing is accumulated
 * atomically: two calls give the same bits, and so do the two layouts of one image.  With all weights 1.0 the outputs are bit-equal
 * to espm_pixel_diagnostics' dev (pixel side) and to espm_channel_diagnostics' dev, xsum, ysum (channel side).
 * k == 0: no model.  d, h, ys and dev must be NULL; only xs is formed and an entry with x == 0 costs its read only (the raw line maps).
 * A summed index whose g weights are all 0 is skipped by the whole workgroup without reading x there: a narrow window costs its own
 * rows, not the whole image.  (Where x's rows run along the summed axis it is read 64, 32 or 16 consecutive indices at a time - one or
 * two cache lines of a row - and it is such a piece that is skipped when none of its indices has a weight.)  That changes no bit:
 * fma(0, v, a) == a for finite v, and x, Y and t are finite for finite x since Y >= log_shift > 0.  Non-finite x or weights are the
 * caller's to refuse.  The side ESPM_MARG_CHANNELS takes at most 65535 * ESPM_MARG_BLOCK channels.
 * No espm_mu_state is involved and its layout is untouched: ESPM_MU_ABI_VERSION stays (it versions that layout, not the list of entry
 * points; a binding finds a missing entry point when it resolves the symbol).
 * ESPM_EINVAL, before the device is touched and with the offending values in the message, for a null pointer, a side, layout or dtype
 * that does not exist, g outside 1..ESPM_MARG_MAX_G, k outside 0..ESPM_MARG_MAX_K, n or p below 1, ld below the row length, log_shift
 * not positive where k > 0, model or output pointers inconsistent with k, scratch_bytes below what the query returns (the message names
 * both sizes).  Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED, and their query returns 0. */
#define ESPM_MARG_MAX_G 8       /* weight vectors per call                                                                       */
#define ESPM_MARG_MAX_K 8       /* components of the model (ESPM_DIAG_MAX_K); 0: no model                                        */
#define ESPM_MARG_BLOCK 256     /* threads per workgroup: pixels, or channels                                                    */
#define ESPM_MARG_PCHUNK 2048   /* pixels per workgroup of the channel side: ESPM_CDIAG_PCHUNK                                   */
enum { ESPM_MARG_PIXELS = 0,    /* weights (g, n) over channels -> outputs (g, p)                                                */
       ESPM_MARG_CHANNELS = 1 };/* weights (g, p) over pixels   -> outputs (g, n)                                                */
int espm_weighted_marginals(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int side, const double* wgt, int g,
                            const double* d, const double* h, int k, double log_shift, double* xs, double* ys, double* dev, void* scratch,
                            size_t scratch_bytes, espm_stream_t stream);
size_t espm_weighted_marginals_scratch(int side, int n, int p, int g);

/* ---- residual products (csrc/mu_residual.hip; espm_amd.residuals, NMFEstimator.residual_components) ----
 * The Pearson residual matrix E = (X - Y) / sqrt(Y), Y = D H, applied to g dense vectors at once from either side, with the Pearson
 * chi^2 of every pixel or channel: the pass a subspace iteration for E's leading singular triplets is made of (a missing phase is a
 * singular value far above sqrt(n) + sqrt(p); against the independence model it is correspondence analysis, hyperspy's
 * Poisson-normalised PCA).  E is never stored.  Plain device pointers, no espm_mu_state; x, x_dtype (ESPM_DIAG_X_*: u8, u16, f32,
 * f64), x_layout, ld, d (n, k) row-major and h (k, p) exactly as for espm_weighted_marginals.  A model is required: k = 1..ESPM_RESID_MAX_K.
 *   side ESPM_RESID_PIXELS    vec (g, n) row-major, one value per channel; out (g, p), out[q, j] = sum_c vec[q, c] e_cj  (E^T U);
 *                             chi2 (p,) = sum_c e_cj^2
 *   side ESPM_RESID_CHANNELS  vec (g, p) row-major, one value per pixel;   out (g, n), out[q, c] = sum_j vec[q, j] e_cj  (E V);
 *                             chi2 (n,) = sum_j e_cj^2
 * chi2 and unmodelled may each be NULL.
 * THE RULE (the outputs are defined by it), all in fp64.  Per entry (c, j) with the count x:
 *   y = 0; y = fma(d[c, i], h[i, j], y) for i ascending; floored = !(y >= log_shift);
 *   e = floored ? 0.0 : (x - y) / sqrt(y)   - a subtraction, an IEEE square root and an IEEE division, one rounding each (no
 *   reciprocal square root).  Per vector q, with v = vec[q, the entry's summed index]:  out_q = fma(v, e, out_q);  chi2 = fma(e, e, chi2).
 * An entry with `floored` and x > 0 adds 1 to *unmodelled (int64, zeroed by the call): counts the model has no rate for
 * (espm_attribute_expected's unattributed ones).  They leave E: a single one at Y = log_shift would carry e ~ 1e7 and own the whole
 * decomposition.  The count is a sum of integers - the same in any order - and the call's only atomic.
 * ORDER, as for the weighted marginals.  The pixel side adds the channels in ascending order, from 0, in the pixel's own thread.  The
 * channel side adds the pixels of a chunk of ESPM_RESID_PCHUNK in ascending order, from 0, and writes the partial sums to `scratch`
 * (device memory, espm_residual_products_scratch(side, n, p, g) bytes: chunks x (g + 1) x n doubles; 0 for the pixel side, whose
 * `scratch` may be NULL); a second launch adds the chunks in ascending order, from 0.  No value is accumulated atomically: two calls
 * give the same bits, and so do the two layouts of one image.  Non-finite x, vectors or models are the caller's to refuse.
 * No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays.
 * ESPM_EINVAL, before the device is touched and with the offending values in the message, for a null pointer, a side, layout or dtype
 * that does not exist, g outside 1..ESPM_RESID_MAX_G, k outside 1..ESPM_RESID_MAX_K, n or p below 1, ld below the row length, log_shift
 * not positive, scratch_bytes below what the query returns (the message names both sizes), more than 65535 * ESPM_RESID_BLOCK channels
 * on the side ESPM_RESID_CHANNELS.  Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED, and their query
 * returns 0. */
#define ESPM_RESID_MAX_G 8       /* vectors per call                                                                              */
#define ESPM_RESID_MAX_K 8       /* components of the model (ESPM_DIAG_MAX_K)                                                     */
#define ESPM_RESID_BLOCK 256     /* threads per workgroup: pixels, or channels                                                    */
#define ESPM_RESID_PCHUNK 2048   /* pixels per workgroup of the channel side: ESPM_MARG_PCHUNK                                    */
enum { ESPM_RESID_PIXELS = 0,    /* vectors (g, n) over channels -> out (g, p), chi2 (p,)                                         */
       ESPM_RESID_CHANNELS = 1 };/* vectors (g, p) over pixels   -> out (g, n), chi2 (n,)                                         */
int espm_residual_products(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, int side, const double* vec, int g,
                           const double* d, const double* h, int k, double log_shift, double* out, double* chi2, int64_t* unmodelled,
                           void* scratch, size_t scratch_bytes, espm_stream_t stream);
size_t espm_residual_products_scratch(int side, int n, int p, int g);

/* ---- pixel ML (csrc/mu_pixel_ml.hip; espm_amd.presence, NMFEstimator.presence_maps) ----
 * The maximum-likelihood abundances of every pixel given the spectra, over a subset of the components, by EM with an optimality
 * certificate and a stop of the pixel's own: the two nested fits a likelihood-ratio test of "is component j in this pixel" compares.
 * An ITERATING image pass: the image is walked once per EM pass, the pixel's state stays in its thread.  Plain device pointers, no
 * espm_mu_state; x, x_dtype (ESPM_DIAG_X_*: u8, u16, f32, f64), x_layout, ld and d (n, k) row-major exactly as for
 * espm_pixel_diagnostics.  mask: the component set M, bit j for component j.  s: a HOST array of k doubles, s[j] = sum_c d[c, j]
 * (read during the call, passed to the kernel by value); s[j] > 0 is required for every j in M.
 * THE RULE (the outputs are defined by it), all in fp64, for the pixel with the counts x:
 *   N = 0; N = N + x_c for c ascending.  N == 0: the pixel is done at once with h = 0, dev = 0, gap = 0 and 0 passes.
 *   start (passes == 0 on entry): h_j = 0 for j not in M; for j in M an h_j that is not > 0 becomes N / (|M| s_j) * 1e-3.
 *   one pass:
 *     1  S = 0; S = fma(s_j, h_j, S) for j in M ascending; f = N / S; h_j = h_j * f            (the scale of least deviance on the ray)
 *     2  per channel c ascending: y = 0; y = fma(d[c, j], h_j, y) for j = 0 .. k - 1; floored = !(y >= log_shift);
 *        y = floored ? log_shift : y; i = 1 / y; w = x_c * i; t = y - x_c; if x_c > 0: t = fma(x_c, log(w), t); dev = dev + t;
 *        q_j = fma(d[c, j], w, q_j)                                  (espm_pixel_diagnostics' expression and floor; dev ends as 2 dev)
 *     3  r_j = q_j / s_j for j in M
 *     4  gap = 2 N (max_{j in M} r_j - 1): the pixel's deviance is above its minimum over {h >= 0, support in M} by at most gap
 *        wherever no entry with counts is floored (convexity, and sum_j s_j h_j = N at h and at the optimum)
 *     5  gap <= tol: the pixel is DONE - h (as scaled in 1), dev, gap and passes are stored and never touched again, done = 1, and
 *        its floored entries with x_c > 0 add to counters[ESPM_PML_UNMODELLED].  Otherwise h_j = h_j r_j (the EM step: the deviance
 *        never rises) and passes goes up by one.
 *     S, dev or gap not finite, or S not > 0: the pixel stops with done = 2 and h as the pass found it (dev, gap as computed), and adds
 *     to counters[ESPM_PML_NONFINITE].
 * A call runs AT MOST n_pass passes for every pixel with done == 0 and is RESUMABLE: the state of a pixel is h_inout (k, p), passes (p,)
 * int32 and done (p,) uint8, which the caller zeroes (passes, done) and fills (h_inout: the start) before the first call; two calls
 * with n_pass = a and b leave bit for bit what one call with a + b leaves.  A pixel still not done after the call holds the h the
 * next pass starts from, and in dev and gap the values of its last pass (of the h before that pass's EM step).  dev, gap (p,) fp64.
 * counters: 3 uint64 on the device.  counters[ESPM_PML_NOT_DONE] is zeroed by the call and receives the number of pixels with
 * done == 0 after it - the one integer a host loop reads between calls; the other two are ADDED to as pixels stop (the caller zeroes
 * them before the first call), so their totals do not depend on how the passes were split into calls.
 * One pixel per thread, ESPM_DIAG_BLOCK pixels per workgroup, d staged through LDS ESPM_DIAG_CHUNK channels at a time; a workgroup
 * leaves the pass loop when all its pixels are done.  No value is accumulated atomically but the three integer counts: a pixel's
 * results do not depend on its neighbours, on the layout, on the dtype that holds its counts, or on the split into calls or slabs.
 * ESPM_EINVAL, before the device is touched, for a null pointer, a layout or dtype that does not exist, n or p below 1, ld below the
 * row length, log_shift or tol not positive, n_pass below 1, a mask that is empty or has bits at or above k, and s[j] not > 0 (or not
 * finite) for a j in the mask; ESPM_EUNSUPPORTED for k outside 1..ESPM_PML_MAX_K.  Only the narrow build has the kernels; the wide
 * builds return ESPM_EUNSUPPORTED.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
#define ESPM_PML_MAX_K 8         /* components of the model (ESPM_DIAG_MAX_K)                                                     */
enum { ESPM_PML_NOT_DONE = 0,    /* pixels with done == 0 after the call (zeroed by the call)                                     */
       ESPM_PML_UNMODELLED = 1,  /* entries with counts whose model is below log_shift, of the pixels that became done (added to)   */
       ESPM_PML_NONFINITE = 2,   /* pixels stopped at a value that is not finite (added to)                                       */
       ESPM_PML_COUNTERS = 3 };
int espm_pixel_ml(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k, uint32_t mask,
                  double log_shift, double tol, int n_pass, double* h_inout, double* dev, double* gap, int32_t* passes, uint8_t* done,
                  uint64_t* counters, espm_stream_t stream);

/* ---- pixel ML, Newton (csrc/mu_pixel_ml_newton.hip; espm_amd.presence with method="newton") ----
 * The problem, the certificate, the stop and every output of espm_pixel_ml, reached by a safeguarded Newton step: the EM rule above
 * stays the defined default, this one is for the images whose tails EM walks for thousands of passes.  The certificate is a property
 * of the point and not of the path that reached it, so it stays the stop rule: every pixel that is done is certified to tol exactly
 * as under EM.  Arguments as for espm_pixel_ml, plus state: caller-owned DEVICE scratch of ESPM_PMLN_STATE_BYTES(k, p) bytes
 * (state_bytes: what the caller allocated), (k + ESPM_PMLN_STATE_EXTRA, p) doubles - rows 0 .. k - 1: e, the EM successor of the last
 * accepted point; row k: dev_acc, its deviance; row k + 1: tau, the blend; row k + 2: trial (0 or 1).  The kernel initialises the
 * state of a pixel that enters with passes == 0 (e = 0, dev_acc = +inf, tau = 1e-2, trial = 0); the caller never fills it, and keeps
 * it, with h_inout, passes and done, from call to call.
 * THE RULE, for the pixel with the counts x; N, the start and steps 1 - 4 are espm_pixel_ml's, and in the walk of step 2, per
 * channel c ascending: v = w * i (x_c / y^2); for a = 0 .. k - 1: t = d[c, a] * v; A_ab = fma(t, d[c, b], A_ab) for b = 0 .. a.
 *     5  S, dev or gap not finite, or S not > 0: the stop of espm_pixel_ml (done = 2, h as the pass found it, dev and gap as computed).
 *        REJECT, if trial and not dev <= dev_acc: h = e, trial = 0, tau = min(10 tau, 1); passes goes up by one; the reported dev and
 *        gap stay those of the accepted point.
 *        ACCEPT, otherwise: dev_acc = dev; dev and gap are reported.  gap <= tol: the pixel is DONE exactly as in espm_pixel_ml (h as
 *        scaled in 1).  Otherwise, in this order: if trial, tau = max(tau / 10, 1e-8); e_j = h_j r_j (the EM successor);
 *        g_j = s_j - q_j; B = A over M with B_jj = fma(tau, s_j / h_j, A_jj); B = L diag(p) L^T by the root-free Cholesky of
 *        espm_pixel_diagnostics, components outside M as rows of the identity; L z = -g, z = z / p, L^T delta = z;
 *        h_j = max(h_j + delta_j, 0.01 h_j, 1e-30 N / s_j) for j in M and trial = 1 - or, if a pivot p_j is not > 0 or not finite,
 *        h = e and trial = 0.  passes goes up by one.
 * Why each piece: a step clamped at exactly 0 is rejected for ever on a pixel with several abundances at the boundary (the clamp at
 * 0.01 h is a fraction-to-boundary rule: a coordinate reaches the boundary geometrically, and can leave it again); A alone is singular
 * where a pixel has fewer counts than components (s_j / h_j is the metric in which the EM step is a gradient step: blended in, B is
 * positive definite, and tau grows after a rejection and shrinks after a success); and after a rejected trial the stored EM
 * successor is a step that cannot raise the deviance.  The accepted deviances of a pixel never increase.
 * RESUMABLE as espm_pixel_ml is, state included: two calls with n_pass = a and b leave bit for bit what one call with a + b leaves.
 * A pixel still not done after the call holds the h its next pass starts from (a trial, or an EM successor), and in dev and gap the
 * values of its last ACCEPTED point.  Counters, geometry, independence of neighbours, layout, dtype and slabs, and the refusals are
 * espm_pixel_ml's; ESPM_EINVAL also for a null state or state_bytes below ESPM_PMLN_STATE_BYTES(k, p).  Only the narrow build has the
 * kernels; the wide builds return ESPM_EUNSUPPORTED.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
#define ESPM_PMLN_STATE_EXTRA 3  /* rows of state beyond the k of e: dev_acc, tau, trial                                          */
#define ESPM_PMLN_STATE_BYTES(k, p) ((size_t)((k) + ESPM_PMLN_STATE_EXTRA) * (size_t)(p) * sizeof(double))
int espm_pixel_ml_newton(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                         uint32_t mask, double log_shift, double tol, int n_pass, double* h_inout, double* dev, double* gap, int32_t* passes,
                         uint8_t* done, uint64_t* counters, void* state, size_t state_bytes, espm_stream_t stream);

/* ---- pixel ML, pinned (csrc/mu_pixel_ml_pinned.hip; espm_amd.presence.ml_unmix_pinned, intervals; NMFEstimator.abundance_intervals) ----
 * One point of the PROFILE likelihood of an abundance: the pixel's best Poisson fit over the component set M with component `pin`
 * (not in M) held at the pixel's own value t[q] - the deviance g(t) whose level set {t: g(t) - min deviance <= chi2_1 quantile} is the
 * profile-likelihood interval of h_pin, and whose value at t = 0 is the reduced fit of the presence test.  Arguments as for
 * espm_pixel_ml_newton, plus pin, t (p,) and slope (p,), DEVICE arrays of doubles; the state has the Newton layout
 * (ESPM_PMLN_STATE_BYTES(k, p); the kernel initialises it for a pixel that enters with passes == 0).  mask MAY be empty (k = 1, or the
 * caller's choice): then the pixel is done in its first pass.
 * THE RULE, all in fp64, for the pixel with the counts x; N as in espm_pixel_ml:
 *   t[q] negative or not finite: the pixel stops at once with done = 2, adds to counters[ESPM_PML_NONFINITE], and h, dev, gap, slope
 *     and passes stay as the call found them (dev, gap, slope 0 where passes == 0).
 *   at EVERY entry: h_pin = t[q] (never updated by a step); h_j = 0 for j outside M and not pin; N == 0: h_j = 0 for j in M.
 *   start (passes == 0 on entry): for j in M an h_j that is not > 0 becomes N / (|M| s_j) * 1e-3; e = 0, dev_acc = +inf, tau = 1e-2,
 *     trial = 0.
 *   one pass:
 *     (no scale onto the ray: step 1 of the other two rules is dropped - with a pinned term the scale of least deviance has no closed
 *      form - so h is the same before and after the walk)
 *     2  the walk of espm_pixel_ml_newton's step 2 over all k components, the pinned one included in y: y, the floor, w, dev, q_j for
 *        every j, and the triangle A
 *     3  for j in M ascending: r_j = q_j / s_j; rmax = max(rmax, r_j) from -inf; lin = fma(s_j - q_j, h_j, lin) from 0
 *     4  gap = 2 fma(N, max(rmax - 1, 0), lin); slope = 2 (s_pin - q_pin)
 *        THE CERTIFICATE: the deviance f is convex in h_M, its gradient is 2 (s_i - q_i), so for the minimiser h* over {h_M >= 0}
 *        f(h) - f(h*) <= grad . (h - h*) = 2 sum_M (s_i - q_i) h_i + 2 sum_M (q_i / s_i - 1) s_i h*_i
 *                     <= 2 lin + 2 max(rmax - 1, 0) sum_M s_i h*_i, and at the optimum (complementary slackness, h*_i (s_i - q*_i) = 0)
 *        sum_M s_i h*_i = sum_M h*_i q*_i = sum_c x_c (y*_c - t d_c,pin) / y*_c <= N.  It holds wherever no entry with counts is
 *        floored, as the certificates of the other two rules.  With M empty gap = 0.
 *        THE SLOPE: by the envelope theorem d/dt min_{h_M} f = df/dh_pin at the inner optimum = 2 (s_pin - q_pin); at a point that is
 *        certified and not optimal it is approximate - a hint for a root finder that keeps a bracket.
 *     5  dev or gap not finite: done = 2, h as it stands, dev, gap and slope as computed, counters[ESPM_PML_NONFINITE].
 *        REJECT / ACCEPT, the stop gap <= tol, tau, the EM successor e_j = h_j r_j (monotone: the pinned term is a fixed background of
 *        the EM model), B = A over M with B_jj = fma(tau, s_j / h_j, A_jj), the root-free Cholesky with every component outside M -
 *        the pinned one too - a row of the identity, the step and the clamps at 0.01 h_j and 1e-30 N / s_j: espm_pixel_ml_newton's
 *        step 5 word for word, with h for its scaled h and h_pin = t[q] after every step.  dev, gap and slope are reported for
 *        ACCEPTED points only.
 *   N == 0 needs no case of its own: h_M = 0, the first pass finds q = 0 and gap = 0 and the pixel is done with
 *   dev = 2 sum_c max(t d_c,pin, log_shift) and 0 passes.
 * RESUMABLE as espm_pixel_ml_newton is (h_inout, dev, gap, slope, passes, done and state carry a pixel from call to call: n_pass = a
 * then b leaves the bits of a + b).  THE CALLER'S done IS HONOURED: a pixel that enters with done != 0 is neither read nor written
 * (h_inout, dev, gap, slope, passes, state: bit-untouched), and a workgroup with no pixel entered returns at once - how a root finder
 * retires the pixels whose endpoint it has found.  Counters, geometry, independence of neighbours, layout, dtype and slabs (a slab
 * slices t and slope as it slices h) as for espm_pixel_ml.  No float atomics.
 * ESPM_EINVAL, before the device is touched: espm_pixel_ml_newton's refusals but for the empty mask, and pin outside 0 .. k - 1, pin
 * inside mask, s[pin] not > 0 (or not finite), a null t or slope.  ESPM_EUNSUPPORTED for k outside 1..ESPM_PML_MAX_K.  Only the narrow
 * build has the kernels; the wide builds return ESPM_EUNSUPPORTED.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
int espm_pixel_ml_pinned(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                         uint32_t mask, int pin, const double* t, double log_shift, double tol, int n_pass, double* h_inout, double* dev,
                         double* gap, double* slope, int32_t* passes, uint8_t* done, uint64_t* counters, void* state, size_t state_bytes,
                         espm_stream_t stream);

/* ---- pixel ML, simplex (csrc/mu_pixel_ml_simplex.hip; espm_amd.presence with method="simplex" / simplex=True; NMFEstimator.presence_maps,
 *      abundance_intervals on a simplex_H fit) ----
 * The pixel problem of a simplex_H fit: the pixel's best Poisson fit over the component set M with the fitted abundances held to
 * sum_M h = total - total = 1 where nothing is pinned (pin = -1), total = 1 - t[q] with component `pin` (not in M) held at t[q] in
 * [0, 1].  Abundances are phase FRACTIONS here and the spectra carry the intensity: there is no free scale per pixel.  Arguments, state
 * (ESPM_PMLN_STATE_BYTES(k, p), initialised by the kernel for a pixel that enters with passes == 0), counters and outputs as for
 * espm_pixel_ml_pinned; pin = -1 means no pinned component, and then t and slope may be null (slope is not written).  mask may be
 * empty only with a pinned component.
 * THE RULE, all in fp64, for the pixel with the counts x; s_j the column sums of d, m = |M|:
 *   t[q] negative, above 1 or not finite (pin >= 0): the pixel stops at once with done = 2, adds to counters[ESPM_PML_NONFINITE], and
 *     h, dev, gap, slope and passes stay as the call found them (dev, gap, slope 0 where passes == 0).
 *   total = 1 - t[q] (1 with pin = -1).
 *   start (passes == 0 on entry): for j in M ascending h_j = max(h_j, 1e-3 total / m), sum = sum + h_j; then h_j = h_j (total / sum);
 *     with m == 1 or total == 0, h_j = total exactly.  e = 0, dev_acc = +inf, tau = 1e-2, trial = 0.
 *   at EVERY entry: h_pin = t[q] (never updated by a step); h_j = 0 for j outside M and not pin.
 *   one pass:
 *     (no scale onto the ray: the sum is constrained, nothing is free to scale)
 *     2  the walk of espm_pixel_ml_pinned's step 2: y over all k components, the floor, w, dev, q_j for every j, the triangle A
 *     3  for j in M ascending, g_j = s_j - q_j: lin = fma(g_j, h_j, lin), hq = fma(h_j, q_j, hq) from 0; gmin = min(gmin, g_j) from +inf
 *     4  gap = 2 (lin - total gmin), the product rounded on its own (no fma: exactly 0 at a vertex and with m == 1); 0 with M empty.
 *        slope = 2 (g_pin - lin / total); 2 (g_pin - gmin) where total == 0; 2 g_pin with M empty.
 *        THE CERTIFICATE (a Frank-Wolfe gap): the deviance f is convex in h_M with the gradient 2 g, so for the minimiser h* over
 *        {h_M >= 0, sum_M h = total}: f(h) - f(h*) <= grad . (h - h*) = 2 lin - 2 sum_M g_i h*_i <= 2 lin - 2 total gmin, a linear
 *        function over the scaled simplex being least at a vertex.  No bound on N enters it.  It is a property of the point and holds
 *        wherever no entry with counts is floored, as the certificates of the other rules.
 *        THE SLOPE: d/dt min f = df/dh_pin + nu d(total)/dt with nu the multiplier of the sum constraint, and at the inner optimum
 *        2 g_i = -nu wherever h_i > 0, so nu = -2 lin / total (envelope theorem); approximate at a point that is certified and not optimal.
 *     5  dev or gap not finite: done = 2, h as it stands, dev, gap and slope as computed, counters[ESPM_PML_NONFINITE].
 *        REJECT, if trial and not dev <= dev_acc: h_M = e, trial = 0, tau = min(10 tau, 1); the pass is counted.
 *        ACCEPT, otherwise: dev, gap and slope are reported.  gap <= tol: DONE (done = 1; the floored entries with counts add to
 *        counters[ESPM_PML_UNMODELLED]).  Else, if hq == 0 (no count that M models - an empty pixel, or counts only where no
 *        component of M reaches: f is linear in h_M with the gradient 2 s): h = total at the j in M of the least s_j (lowest index on
 *        ties), 0 on the rest of M; e = h, dev_acc = dev, trial = 0; the pass is counted, and the next one certifies with gap = 0.
 *        Else, in this order: if trial, tau = max(tau / 10, 1e-8);
 *        THE EM SUCCESSOR e (the multiplicative H step under the simplex, regularisers off: monotone): n_j = (h_j q_j) (1 / total), j in M;
 *        over P = {n_j > 0}: nu = max_P (n_j - s_j); at most 64 times: i_j = 1 / (s_j + nu), c_j = n_j i_j, psi = sum c_j,
 *        dps = fma(c_j, i_j, dps), next = nu + (psi - 1) / dps, stop unless next > nu, nu = next (psi is convex and decreasing and
 *        psi(nu_0) >= 1: the iteration rises monotonically to the root); e_j = total (n_j (1 / (s_j + nu))), 0 on the rest of M,
 *        se = sum e_j, e_j = e_j (total / se);
 *        THE TRIAL: over the active set {j in M, h_j > 0} (an abundance at exactly 0 stays there, as under EM) B = A with
 *        B_jj = fma(tau, max(q_j, s_j) / h_j, A_jj) - the EM surrogate's curvature is q_j / h_j; the max keeps B definite where a
 *        component sees no counts -, every other component a row of the identity; ONE root-free Cholesky B = L diag(p) L^T and two
 *        solves, u = B^-1 (-g), v = B^-1 1 (both 0 off the active set; the middle step multiplies by 1 / p_j); mult = sum u / sum v; delta_j = fma(-mult, v_j, u_j) - the
 *        Newton step of the blended model with the sum held; trial_j = max(h_j + delta_j, 0.01 h_j), sc = sum trial_j,
 *        h_j = trial_j (total / sc); trial = 1, dev_acc = dev.  A pivot that is not positive or not finite, or an h_j that is not
 *        finite: h_M = e, trial = 0 instead.  The pass is counted.
 *   sum_M h_j = total to within m ulps of total after every step (one rounding in each of the m products, m - 1 in the sum behind the
 *   scale); h_pin = t[q] bit for bit; rows outside M and pin exactly 0.
 * RESUMABLE, THE CALLER'S done HONOURED, counters, geometry, independence of neighbours, layout, dtype and slabs as for
 * espm_pixel_ml_pinned.  No float atomics.
 * ESPM_EINVAL, before the device is touched: espm_pixel_ml_pinned's refusals with pin = -1 allowed, and an empty mask with pin = -1,
 * pin < -1, a null t or slope with pin >= 0.  ESPM_EUNSUPPORTED for k outside 1..ESPM_PML_MAX_K.  Only the narrow build has the kernels;
 * the wide builds return ESPM_EUNSUPPORTED.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
int espm_pixel_ml_simplex(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* s, int k,
                          uint32_t mask, int pin, const double* t, double log_shift, double tol, int n_pass, double* h_inout, double* dev,
                          double* gap, double* slope, int32_t* passes, uint8_t* done, uint64_t* counters, void* state, size_t state_bytes,
                          espm_stream_t stream);

/* ---- spectra ML pass (csrc/mu_spectra_ml.hip; espm_amd.spectra_ml, NMFEstimator.element_presence) ----
 * What one pass of the maximum-likelihood fit of W given H needs from the image (the rule itself is small dense algebra above this
 * pass: espm_amd/spectra_ml.py): the sums of espm_channel_diagnostics under the OBSERVED weights, in one fp64
 * pass over X that reduces over the pixels.  x, x_dtype (ESPM_DIAG_X_*), x_layout, ld, d (n, k), h (k, p) and log_shift are exactly
 * as for espm_channel_diagnostics.  Per entry: y = sum_j d[c, j] h[j, p] (fma, j ascending); floored = !(y >= log_shift);
 * y = floored ? log_shift : y; i = 1 / y; w = x * i; v = w * i.  Per channel c (all outputs fp64):
 *   dev[c]       = 2 sum_p (x ln(w) - x + y), the first term 0 where x == 0
 *   xsum[c]      = sum_p x (exact for counts), ysum[c] = sum_p y
 *   q[c, j]      (n, k): sum_p w h[j, p] - Q = (X / Y) H^T; with a dictionary G^T Q is the numerator of the multiplicative W step
 *   a_tri[c, t]  (n, k (k + 1) / 2): the lower triangle, row by row as m_tri, of A_c = sum_p v h_p h_p^T, the observed information
 *                  of row c of d with the abundances held; that of W in d = G W is F_obs = sum_c (g_c g_c^T) (x) A_c.
 *   *unmodelled  (device, zeroed by the call): the entries with x > 0 that are floored - an integer sum, the only thing accumulated
 *                  atomically.
 * Geometry, scratch layout (espm_spectra_ml_pass_scratch(n, p, k) bytes: chunks x (3 + k + k (k + 1) / 2) x n doubles) and the
 * second launch that adds the chunks in ascending order are espm_channel_diagnostics': two calls, the two layouts of one image,
 * every dtype that holds the same values and rows padded by ld give the same bits (a split of the pixels into slabs does not: the
 * chunk sums change).  k = 1..ESPM_DIAG_MAX_K.  ESPM_EINVAL, before the device is touched, for a null pointer, a layout or dtype
 * that does not exist, ld below the row length, n or p below 1, log_shift not positive, or scratch_bytes below what the query
 * returns (the message names both sizes); ESPM_EUNSUPPORTED for k outside 1..ESPM_DIAG_MAX_K.  Only the narrow build has the kernels;
 * the wide builds return ESPM_EUNSUPPORTED, and their query returns 0.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
int espm_spectra_ml_pass(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h, int k,
                         double log_shift, double* dev, double* xsum, double* ysum, double* q, double* a_tri, int64_t* unmodelled,
                         void* scratch, size_t scratch_bytes, espm_stream_t stream);
size_t espm_spectra_ml_pass_scratch(int n, int p, int k);

/* ---- spectra ML pass, batched (csrc/mu_spectra_ml.hip; espm_amd.spectra_ml.intervals, NMFEstimator.concentration_intervals) ----
 * espm_spectra_ml_pass for n_models models d[b] (n, k), b = 0 .. n_models - 1, of ONE resident image and ONE h, in one pass launch
 * and one reduction launch: the model index is the third grid dimension, the kernel body, the tile code, the accumulation order and
 * the ascending chunk reduction are the single pass's own (one device function that both kernels call).  Model b's dev[b] (n,),
 * ysum[b] (n,), q[b] (n, k), a_tri[b] (n, k (k + 1) / 2) and unmodelled[b] are BIT-EQUAL to what espm_spectra_ml_pass gives at d[b],
 * whatever n_models, the order of the models and the flags of the others.  (xsum does not depend on the model: not an output.)
 * active (device, (n_models,) bytes; null: every model): a workgroup of either launch whose model has active[b] == 0 returns at
 * entry, before it touches x - a RETIRED model costs a launch slot and nothing else, and its outputs and its counter are left
 * exactly as they were.  The counters of the active models are zeroed by the call (a launch of n_models threads ahead of the pass).
 * This is what lets many fits of one image run in lockstep, each retiring on its own, without re-packing the problems.
 * Scratch: espm_spectra_ml_pass_batch_scratch(n, p, k, n_models) bytes = n_models x espm_spectra_ml_pass_scratch(n, p, k), model b's
 * partial sums at b x that.  X is re-read once per model (the pass is bound by its arithmetic, not by X).  No float atomics.
 * ESPM_EINVAL, before the device is touched: the single pass's refusals (active may be null), n_models outside
 * 1..ESPM_SML_MAX_MODELS, scratch_bytes below what the query returns (the message names both sizes); ESPM_EUNSUPPORTED for k outside
 * 1..ESPM_DIAG_MAX_K.  Only the narrow build has the kernels; the wide builds return ESPM_EUNSUPPORTED, and their query returns 0
 * (as it does for arguments out of range).  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
#define ESPM_SML_MAX_MODELS 65535   /* models of one call: the third grid dimension */
int espm_spectra_ml_pass_batch(const void* x, int x_dtype, int x_layout, int64_t ld, int n, int p, const double* d, const double* h,
                               int k, int n_models, const uint8_t* active, double log_shift, double* dev, double* ysum, double* q,
                               double* a_tri, int64_t* unmodelled, void* scratch, size_t scratch_bytes, espm_stream_t stream);
size_t espm_spectra_ml_pass_batch_scratch(int n, int p, int k, int n_models);

/* ---- channel ML step (csrc/mu_channel_ml.hip; espm_amd.channel_ml, NMFEstimator.spectrum_presence, spectrum_intervals) ----
 * The maximum-likelihood spectra d (n, k) >= 0 given the abundances h (k, p), WITHOUT a dictionary: the problem decouples per
 * channel.  Channel c is one pixel problem of espm_pixel_ml_newton / espm_pixel_ml_pinned with the roles of the factors swapped:
 * its observations are the p pixels of row c of X, its design is h^T, its "spectrum sums" are s_j = sum_p h[j, p] (the same for every
 * channel) and its count total is N_c = xsum[c].  The walk over the observations is espm_spectra_ml_pass_batch, which delivers per
 * (model, channel) exactly the sums a pixel kernel holds after its walk: dev (already doubled), q (k) and the lower triangle of A.
 * This entry point is everything those kernels do BETWEEN two walks, for n_models x n problems at once, one thread per problem:
 *     loop:  espm_spectra_ml_pass_batch(d, active) -> dev_in, q, a_tri;   espm_channel_ml_step(...) -> the next d, done, active
 * All device arrays but s and pin, which are HOST arrays (k doubles, n_models int32: checked, then passed by value):
 *   dev_in (n_models, n), q (n_models, n, k), a_tri (n_models, n, k (k + 1) / 2): the batched pass's outputs at the d this call finds
 *     (not read with start != 0, and may be null then); xsum (n,): espm_spectra_ml_pass's sum_p x, which no model changes
 *   mask: the component set, the same for every model; pin[b]: -1 - model b fits all of mask by the FREE-SCALE rule
 *     (espm_pixel_ml_newton's); j, a component of mask - model b holds component j at t[b, c] and fits M = mask less j by the PINNED
 *     rule (espm_pixel_ml_pinned's; M may be empty).  t (n_models, n) and slope (n_models, n) are read and written for pinned models
 *     only, and may be null where every pin is -1.  Components outside mask are held at 0.
 *   d (n_models, n, k), in and out: the point the pass evaluated, replaced by the point the next pass evaluates
 *   state: caller-owned, ESPM_CML_STATE_BYTES(k, n, n_models) bytes, (n_models, 2 k + ESPM_CML_STATE_EXTRA, n) doubles - rows
 *     0 .. k - 1: the last ACCEPTED point (what dev and gap belong to), k .. 2 k - 1: e, its EM successor, then dev_acc, tau, trial
 *   dev, gap, slope (n_models, n) doubles, passes (n_models, n) int32, done (n_models, n) bytes: the outputs per problem, of the last
 *     accepted point, exactly as the pixel entry points keep them
 *   active (n_models,) bytes and live (n_models,) int64, both written: live[b] = the problems of model b with done == 0 after the call
 *     (zeroed by the call, then added to per workgroup: integers), active[b] = (live[b] != 0), set by a second launch of n_models
 *     threads behind the first on `stream` - the flags espm_spectra_ml_pass_batch skips a retired model by.
 * start != 0, PASS 0 of every problem with done == 0 (the caller zeroes done; nothing of a pass is consumed, none is counted):
 *   a pinned t[b, c] that is negative or not finite: done = 2, d as it was.  Otherwise the rule's own start: d_pin = t; d_j = 0
 *   outside M and pin; N_c == 0: d_M = 0 and, for the free rule, done = 1 at once (the row of zeros, dev = gap = 0); a start in M that
 *   is not > 0 becomes N_c / (|M| s_j) * 1e-3; the free rule then scales onto the ray (below).  e = 0, dev_acc = +inf, tau = 1e-2,
 *   trial = 0, the accepted point = the start, dev = gap = slope = 0, passes = 0.  (A pinned problem with N_c == 0 needs no case of
 *   its own: its first pass finds q = 0, gap = 0 and is done with dev = 2 sum_p max(t h[pin, p], log_shift) and 0 passes.)
 * start == 0, per problem with done == 0, h = d[b, c], in fp64 and in this order:
 *   for j in M ascending: r_j = q_j / s_j; rmax = max(rmax, r_j) from -inf; lin = fma(s_j - q_j, h_j, lin) from 0
 *   free:   gap = 2 N_c (rmax - 1)                              pinned: gap = 2 fma(N_c, max(rmax - 1, 0), lin), slope = 2 (s_pin - q_pin)
 *   (the certificates of espm_pixel_ml and espm_pixel_ml_pinned: dev is above its minimum over the set by at most gap)
 *   dev_in or gap not finite: done = 2, dev, gap and slope as computed.
 *   REJECT, if trial and not dev_in <= dev_acc: h = e (h_pin stays), trial = 0, tau = min(10 tau, 1); passes goes up by one; dev, gap,
 *   slope and the accepted point stay.
 *   ACCEPT, otherwise: dev, gap, slope and the accepted point are this point's.  gap <= tol: done = 1, d keeps the point.  Otherwise
 *   espm_pixel_ml_newton's step 5 word for word: if trial, tau = max(tau / 10, 1e-8); e_j = h_j r_j; B = A over M with
 *   B_jj = fma(tau, s_j / h_j, A_jj), components outside M (the pinned one too) rows of the identity; the root-free Cholesky
 *   B = L diag(p) L^T; L z = q - s, z = z / p, L^T delta = z; h_j = max(h_j + delta_j, 0.01 h_j, 1e-30 N_c / s_j) on M and trial = 1 -
 *   or, if a pivot is not > 0 or not finite, h = e and trial = 0; dev_acc = dev_in; passes goes up by one.
 *   THE RAY (free rule only, after the start, a rejection and a step): S = fma(s_j, h_j, S) over M ascending; S not > 0 or not finite:
 *   done = 2, h as the step left it; else h = h (N_c / S) - what espm_pixel_ml_newton does at the head of its pass.
 *   d[b, c] = h.
 * THE CALLER'S done IS HONOURED: a problem that enters with done != 0 is neither read nor written (d, state, dev, gap, slope, passes:
 * bit-untouched; its d row keeps its final point), and a workgroup with none entered returns at entry.  A problem's results depend on
 * its own sums only: a model alone gives the bits it gives inside any batch.  No float atomics.
 * ESPM_EINVAL, before the device is touched: a null pointer (dev_in, q, a_tri with start == 0; t, slope with a pinned model; every
 * other always), n below 1 or above 65535 x ESPM_CDIAG_BLOCK, n_models outside 1..ESPM_SML_MAX_MODELS, an empty mask or bits at or
 * above k, a pin[b] that is neither -1 nor a component of mask, tol not positive, s[j] not > 0 (or not finite) for a j in mask,
 * state_bytes below ESPM_CML_STATE_BYTES(k, n, n_models).  ESPM_EUNSUPPORTED for k outside 1..ESPM_DIAG_MAX_K.  Only the narrow build
 * has the kernels; the wide builds return ESPM_EUNSUPPORTED.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
#define ESPM_CML_STATE_EXTRA 3   /* rows of state beyond the 2 k of the accepted point and e: dev_acc, tau, trial               */
#define ESPM_CML_STATE_BYTES(k, n, n_models) ((size_t)(n_models) * (size_t)(2 * (k) + ESPM_CML_STATE_EXTRA) * (size_t)(n) * sizeof(double))
int espm_channel_ml_step(int n, int k, int n_models, int start, const double* dev_in, const double* q, const double* a_tri,
                         const double* xsum, const double* s, uint32_t mask, const int32_t* pin, const double* t, double tol, double* d,
                         void* state, size_t state_bytes, double* dev, double* gap, double* slope, int32_t* passes, uint8_t* done,
                         uint8_t* active, int64_t* live, espm_stream_t stream);

/* ---- LDS of the sparse H-step (csrc/mu_ell_plan.hpp: plan_h_ell; espm_amd.ell.lds_bytes_h, the store choice of espm_amd.store) ----
 * Dynamic LDS, in bytes, that the H-step of the sparse count store (x_dtype = ESPM_X_ELL) takes for n_pad channels and k components
 * at the full tile (tile_px = ESPM_ELL_TILE) without the copy of colsum(GW') that a riding W tail adds: the G W table plus the
 * region of the partial numerators.  The store fits where this is at most ESPM_ELL_LDS_MAX.  Answered from the plan the launch
 * itself lays out its LDS by, so the two cannot disagree.  (size_t)-1 for a k this build has no sparse kernels for (each build its
 * own 1..8 or 9..16; the 17..32 build has none).  No device is touched.  No espm_mu_state is involved: ESPM_MU_ABI_VERSION stays. */
size_t espm_mu_ell_h_lds_bytes(int n_pad, int k);

#ifdef __cplusplus
}
#endif
#endif /* ESPM_MU_H */
