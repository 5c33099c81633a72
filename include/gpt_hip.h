/*
 * gpt_hip.h -- C ABI of libgpt_hip.so: the MI355X (gfx950) implementation of gptools'
 * covariance-build + Cholesky log-marginal-likelihood hot path.
 *
 * Plain C, no torch / numpy types: pointers, sizes and scalars only.  Matrices are row-major
 * (C order, like the numpy arrays the reference passes around).  Every entry point returns an
 * int status:
 *      0            success
 *     >0            LAPACK convention: the leading minor of that order is not positive
 *                   definite (the Python layer raises numpy.linalg.LinAlgError, which
 *                   GaussianProcess.update_hyperparameters turns into +inf exactly like
 *                   gaussian_process.py:1391-1406)
 *     <0            GPT_E_* below
 * gpt_last_error() returns a thread-local human-readable message for the last failure.
 *
 * Citations "ref: file:line" are into the reference tree (markchil/gptools).
 *
 * There are two layers:
 *   (1) context API, host pointers in / host scalars out, device state stays resident in HBM
 *       between calls -- this is what a ctypes/cffi binding inside gptools would call;
 *   (2) device API (gpt_dev_*), raw device pointers + the context's stream -- used by callers
 *       that own device memory themselves (the one-process-per-GPU block-cyclic Cholesky in
 *       gptools_amd/dist.py passes torch.Tensor.data_ptr() values).
 *
 * Gradients of the log marginal likelihood come in two forms, both after a fit and both at the cost of K_tot^-1 plus passes over
 * the pairs: gpt_ll_grad, analytic, for squared-exponential terms (what the reference differentiates), and gpt_ll_grad_diff, for
 * every kernel and product the fits take, by central differences of the pair function taken per pair.
 */
#ifndef GPT_HIP_H_
#define GPT_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPT_OK 0
#define GPT_E_ARG (-1)      /* bad argument / shape                       -> ValueError           */
#define GPT_E_VALUE (-2)    /* Matern52 derivative order > 1              -> ValueError  (ref: kernel/matern.py:545-546) */
#define GPT_E_NOTIMPL (-3)  /* unsupported hyper_deriv                     -> NotImplementedError (ref: kernel/matern.py:543-544) */
#define GPT_E_HIP (-4)      /* HIP runtime error                          -> RuntimeError         */
#define GPT_E_NOMEM (-5)    /* device allocation failed                   -> MemoryError          */
#define GPT_E_STATE (-6)    /* call out of order (e.g. predict before fit) -> RuntimeError         */

/* kernel_id values (ref: kernel/squared_exponential.py:31, kernel/matern.py:468,
 * kernel/noise.py:27, kernel/noise.py:112) */
#define GPT_KERNEL_SE 0
#define GPT_KERNEL_M52 1
#define GPT_KERNEL_DIAGNOISE 2
#define GPT_KERNEL_ZERO 3
#define GPT_KERNEL_RQ 4          /* RationalQuadraticKernel, params [sigma_f, alpha, l_1 .. l_D]
                                  * (ref: gptools/kernel/rational_quadratic.py:30-164 through ChainRuleKernel.__call__,
                                  * kernel/core.py:691-816); derivative orders of a pair may sum to GPT_RQ_MAXORD at most
                                  * (GPT_E_VALUE beyond; the reference has no limit, but walks every set partition of the
                                  * derivative multiset: Bell(12) = 4.2 million per pair); no hyper-parameter derivatives */
#define GPT_RQ_MAXORD 16
#define GPT_KERNEL_MATERN 5      /* MaternKernel (general order nu), params [sigma_f, nu, l_1 .. l_D] (ref: kernel/matern.py:251-465
                                  * through ChainRuleKernel.__call__); same limit on the derivative orders of a pair; nu must
                                  * lie in (0, 60) (GPT_E_VALUE otherwise: beyond it the closed form the device evaluates,
                                  * 2^(1-nu)/Gamma(nu) y^((nu-m)/2) K_(nu-m)(sqrt y), overflows in its factors before the
                                  * product is formed.  The reference accepts any nu and evaluates the same form through
                                  * scipy.special.kv, with the same fate: run here (round 5), MaternKernel(nu = 70) already returns nan for
                                  * a pair 1e-6 apart at l = 0.3 (50: still 1.0), nu = 130 nan / inf for every pair closer than
                                  * 0.02, nu = 160 nan throughout) */

#define GPT_KERNEL_PRODUCT 6     /* k1 * k2 of two of the kernels above (SE, Matern52, RQ, Matern), GPT_KERNEL_PERIODIC or GPT_KERNEL_SPECTRAL, ref: kernel/core.py:587-671: the product
                                  * rule over the derivative orders of a pair, sum over sub-multi-indices a of prod_slots C(n, a)
                                  * k1^(a) k2^(n - a), evaluated per pair on the device (gpt_kpairs2 / gpt_kbuild2 / gpt_fit_terms);
                                  * combined derivative order of a pair <= GPT_RQ_MAXORD; no hyper-parameter derivatives
                                  * (NotImplementedError in the reference too) */
#define GPT_KERNEL_GIBBS_TANH 7  /* GibbsKernel1dTanh, num_dim 1, params [sigma_f, l_1, l_2, l_w, x_0] (ref: kernel/gibbs.py:229-466):
                                  * k = sigma_f^2 sqrt(2 l(x) l(x') / (l(x)^2 + l(x')^2)) exp(-(x - x')^2 / (l(x)^2 + l(x')^2)),
                                  * l(x) = (l_1 + l_2)/2 - (l_1 - l_2)/2 tanh((x - x_0)/l_w).  Derivative order <= 1 per point
                                  * (GPT_E_NOTIMPL beyond: "Derivatives greater than [1, 1] are not supported!"); num_dim != 1 or
                                  * a wrong parameter count GPT_E_ARG; no hyper-parameter derivatives (GPT_E_NOTIMPL) */
#define GPT_KERNEL_GIBBS_DTANH 8 /* GibbsKernel1dDoubleTanh, the same with params [sigma_f, l_c, l_m, l_e, l_a, l_b, x_a, x_b]
                                  * (ref: kernel/gibbs.py:508-558): l(x) = a tanh((x - x_a)/l_a) + b tanh((x - x_b)/l_b) + c,
                                  * a = (l_m - l_c)/2, b = (l_e - l_m)/2, c = (l_c + l_e)/2 */
#define GPT_KERNEL_GIBBS_CUBIC 9 /* GibbsKernel1dCubicBucket, the same with params [sigma_f, l_1, l_2, l_3, x_0, w_1, w_2, w_3]
                                  * (ref: kernel/gibbs.py:603-692): l(x) is l_1 left of the bucket, l_2 inside it (centre x_0, width
                                  * w_2), l_3 right of it, joined by cubic sections of widths w_1 and w_3.  Evaluated as the reference
                                  * writes it: the five section values (two for l') each times its 0/1 mask, summed -- so w_1 = 0 or
                                  * w_3 = 0 is NaN everywhere, negative widths overlap or leave gaps exactly as there */
#define GPT_KERNEL_GIBBS_QUINTIC 10 /* GibbsKernel1dQuinticBucket, the same 8 params with quintic joins (ref: kernel/gibbs.py:695-801) */
#define GPT_KERNEL_GIBBS_EXPGAUSS 11 /* GibbsKernel1dExpGauss with G Gaussians, 3 G + 2 params [sigma_f, l_0, mu_1 .. mu_G,
                                  * sigma_1 .. sigma_G, beta_1 .. beta_G] (ref: kernel/gibbs.py:804-902):
                                  * l(x) = l_0 exp(sum_i beta_i exp(-(x - mu_i)^2 / (2 sigma_i^2))).  1 <= G <= GPT_GIBBS_MAX_GAUSS
                                  * (the parameters travel by value in the kernel arguments); a parameter count that is not 3 G + 2
                                  * or a G beyond the cap is GPT_E_ARG */
#define GPT_GIBBS_MAX_GAUSS 8    /* most Gaussians of GPT_KERNEL_GIBBS_EXPGAUSS */
#define GPT_KERNEL_GIBBS_BSPLINE 12 /* GibbsKernel1dBSpline, cubic, with nt knots: 2 nt + 3 params [sigma_f, t_1 .. t_nt,
                                  * C_1 .. C_{nt+2}] (ref: kernel/gibbs.py:905-992, splines.py:5-146): l(x) = sum_i C_i B_{i,3}(x),
                                  * the cubic B-spline on the knots with three copies of t_1 and t_nt appended; l = l' = 0 outside
                                  * [t_1, t_nt] (the kernel is then NaN or 0 as in the reference), the last span closed on the
                                  * right, repeated knots allowed.  nt = (nparams - 3) / 2: an even parameter count, nt < 2 or
                                  * nt > GPT_GIBBS_MAX_KNOTS (the parameters travel by value in the kernel arguments) is GPT_E_ARG;
                                  * knots that are not in increasing order (a NaN knot among them) GPT_E_VALUE, "Knots must be in
                                  * increasing order!", before anything is launched */
#define GPT_GIBBS_MAX_KNOTS 11   /* most knots of GPT_KERNEL_GIBBS_BSPLINE */
#define GPT_KERNEL_GIBBS_GP 13   /* GibbsKernel1dGP with m points and a nested 1-D squared-exponential kernel (ref: kernel/gibbs.py:995-1095),
                                  * 2 m + 2 params [sigma_f, l, x_1 .. x_m, c_1 .. c_m]: l(x) = sum_j c_j exp(-(x - x_j)^2 / (2 l^2)),
                                  * the mean of the nested noiseless GP in closed form.  The c_j are its WEIGHTS, not the class's
                                  * hyperparameters y_j: c = sigma_n^2 (sigma_n^2 E + 1e2 eps I)^-1 y with E_ij = exp(-(x_i - x_j)^2 /
                                  * (2 l^2)), an m x m solve the caller does once per hyperparameter vector (gptools_amd/kernel/gibbs.py,
                                  * GPWarp.weights).  m = (nparams - 2) / 2: an odd parameter count, m < 1 or m > GPT_GIBBS_MAX_GP_POINTS
                                  * (the parameters travel by value in the kernel arguments) is GPT_E_ARG.  A non-finite or non-positive
                                  * l is not refused: it gives NaN (or what the arithmetic gives) like the other length scales */
#define GPT_GIBBS_MAX_GP_POINTS 12 /* most points of GPT_KERNEL_GIBBS_GP */
#define GPT_KERNEL_PERIODIC 14   /* PeriodicKernel, the exp-sine-squared covariance (no counterpart in the reference), 2 D + 1 params
                                  * [sigma_f, l_1 .. l_D, p_1 .. p_D]:
                                  *   k = sigma_f^2 prod_d exp(-2 sin^2(pi tau_d / p_d) / l_d^2),  tau = x - x'.
                                  * Derivative observations of any order up to a COMBINED order of GPT_PERIODIC_MAXORD per dimension,
                                  * ni_d + nj_d <= 16 (GPT_E_VALUE beyond, before anything is launched: for training points from the
                                  * largest order of each coordinate, 2 max_i n_id; for test points and pair lists from the orders
                                  * given); other dimensions do not count, the kernel is separable.  A period that is not finite and
                                  * positive, a length scale that is NaN, zero or so small that 1 / l^2 overflows: GPT_E_VALUE.
                                  * l_d = +inf is legal and masks dimension d out (1 / l^2 = 0: the factor is exactly 1.0, every
                                  * derivative in d exactly 0.0; MaskedKernel hands p_d = 1 there).  tau is reduced in units of the
                                  * period, t = tau / p - rint(tau / p), before any sine is taken: the kernel is periodic to rounding.
                                  * A product factor beside SE, Matern52, RationalQuadratic, Matern or another Periodic (the locally
                                  * periodic model SE * Periodic), with the product's own cap on the summed orders of a pair; beside a
                                  * Gibbs factor GPT_E_ARG.  No hyper-parameter derivatives (GPT_E_NOTIMPL); gpt_ll_grad_diff covers it */
#define GPT_PERIODIC_MAXORD 16   /* largest ni_d + nj_d of one dimension for GPT_KERNEL_PERIODIC */
#define GPT_KERNEL_SPECTRAL 15   /* SpectralKernel, ONE component of the spectral mixture kernel of Wilson & Adams (ICML 2013; no counterpart
                                  * in the reference), 2 D + 1 params [sigma_f, mu_1 .. mu_D, l_1 .. l_D]:
                                  *   k = sigma_f^2 exp(-sum_d tau_d^2 / (2 l_d^2)) cos(2 pi sum_d mu_d tau_d),  tau = x - x'
                                  * -- one cosine of the dot product.  A mixture of Q components is a model of Q terms (gpt_fit_terms,
                                  * up to GPT_MAX_TERMS).  mu = 0 is the squared exponential.  Derivative observations of any order up
                                  * to a COMBINED order of GPT_SPECTRAL_MAXORD per dimension, ni_d + nj_d <= 16 (GPT_E_VALUE beyond,
                                  * before anything is launched, by the rule of GPT_KERNEL_PERIODIC).  A frequency mu_d that is not
                                  * finite, a length scale that is NaN, zero or so small that 1 / l^2 overflows: GPT_E_VALUE; mu_d may
                                  * have any sign.  l_d = +inf is legal and drops the envelope in dimension d (1 / l^2 = 0; every
                                  * l_d = +inf: the pure cosine kernel); mu_d = 0 and l_d = +inf masks dimension d out -- it contributes
                                  * exactly 1.0 without a derivative order and exactly 0.0 with one (MaskedKernel).  The phase
                                  * sum_d mu_d tau_d is kept in cycles and reduced by its nearest integer before any sine is taken.
                                  * A product factor beside SE, Matern52, RationalQuadratic, Matern, Periodic or another Spectral,
                                  * with the product's own cap on the summed orders of a pair; beside a Gibbs factor GPT_E_ARG.
                                  * No hyper-parameter derivatives (GPT_E_NOTIMPL); gpt_ll_grad_diff covers it */
#define GPT_SPECTRAL_MAXORD 16   /* largest ni_d + nj_d of one dimension for GPT_KERNEL_SPECTRAL */

/* MaskedKernel (ref: kernel/core.py:1011-1149): a kernel that acts on a subset of the num_dim coordinates and is exactly 0.0 for a
 * pair with a derivative order in any other coordinate.
 *   - A masked SE / Matern52 / RationalQuadratic / Matern kernel has no id of its own.  It IS the kernel at num_dim whose
 *     masked-out coordinates have the length scale +infinity in the parameter array (1/l = 1/l^2 = 0 exactly): the distance ignores
 *     those coordinates and every derivative order in them multiplies the pair by zero -- 0.0, never NaN or inf, coincident points
 *     included (the Matern pair function guards its r = 0 classes behind a flag make_kparams raises for an infinite length scale).
 *     The hyper-parameter indices of such an array are the expanded array's, not the base kernel's: gpt_ll_grad is not offered.
 *   - A 1-D Gibbs kernel on coordinate d of a num_dim <= GPT_GIBBS_ON_DIM_MAX_D model: kernel id GPT_KERNEL_ON_DIM(id, d) with the
 *     parameters of the plain id.  Accepted wherever a PRODUCT FACTOR is (gpt_kpairs2, gpt_kbuild2, kernel_ids / kernel_ids2 of
 *     gpt_fit_terms and gpt_fit_batch_terms): the factor is evaluated from coordinate d of the two points and that coordinate's
 *     orders, and is 0.0 when any other coordinate carries an order.  A masked Gibbs kernel on its own is its product with the
 *     constant unit factor SE [1, inf .. inf].  The plain ids keep their meaning: num_dim 1, and a Gibbs id WITHOUT a coordinate
 *     at num_dim > 1 is refused as before; d >= num_dim, a non-Gibbs id, num_dim > GPT_GIBBS_ON_DIM_MAX_D or a use outside a product
 *     (gpt_kpairs, gpt_kbuild, gpt_fit, gpt_fit_sum, a term of gpt_fit_terms without a second factor; at num_dim 1 too) is
 *     GPT_E_ARG.  The Gibbs order rule (orders <= 1, GPT_E_NOTIMPL beyond) applies to coordinate d alone -- training points, test
 *     points and pair lists alike: n = [1, 1] or [0, 2] with the Gibbs factor on coordinate 0 is a first / no derivative for it,
 *     the rest belongs to the other factor and to that factor's own rules; the cap on the summed orders of a pair in a product
 *     (GPT_RQ_MAXORD) and the Matern52 rule (a point's orders sum to <= 1) keep looking at whole rows. */
#define GPT_GIBBS_ON_DIM_MAX_D 3
#define GPT_KERNEL_ON_DIM(id, d) ((id) + 256 * ((d) + 1))
#define GPT_KERNEL_BASE_ID(kid) ((kid) >= 256 ? (kid) % 256 : (kid))      /* the plain id of either form */
#define GPT_KERNEL_DIM_OF(kid) ((kid) >= 256 ? (kid) / 256 - 1 : -1)      /* the coordinate, -1 for a plain id */

#define GPT_MAX_DIM 16      /* largest supported num_dim */
#define GPT_WARP_LINEAR 1    /* input warp layer w = (x - a)/(b - a) per dimension (ref: kernel/warping.py:367-402) */
#define GPT_WARP_BETA 2      /* input warp layer w = I_x(alpha, beta), the beta CDF, per dimension (ref: kernel/warping.py:315-365) */
#define GPT_WARP_MAX_LAYERS 4
#define GPT_WS_BLOCK 9216    /* doubles of factorisation workspace per 128 columns (d_invd arguments) */

typedef struct gpt_ctx gpt_ctx;

int gpt_version(void);
const char *gpt_last_error(void);

/* ---- context ------------------------------------------------------------------------------ */
/* One context = one GPU + one main HIP stream (+ an internal high-priority panel stream used for
 * look-ahead).  stream == NULL: the library creates its own non-blocking stream; otherwise the
 * caller's hipStream_t is used for all work (pass torch.cuda.current_stream().cuda_stream). */
int gpt_ctx_create(int device_id, void *stream, gpt_ctx **out);
int gpt_ctx_destroy(gpt_ctx *ctx);
/* Options (gpt_ctx_set_option):
 *   "nb_outer"     outer block width of the factorisation, multiple of 128; 0 = by size (256 up to n = 5120, 384 up to
 *                  12288, 640 above)
 *   "lookahead"    0/1: factor panel k+1 on the high-priority panel stream while the main stream applies panel k
 *   "purg_rows"    while more rows than this remain the panel stream applies panel k to the columns of panel k+1 itself
 *                  (6144; 0 = the main stream always does)
 *   "gemm_prio"    >= 0 forces one wave priority (0..3) for every GEMM main loop of the context (the panel-side context of
 *                  gptools_amd/dist.py); -1 (default): 2 on the panel stream, 0 elsewhere
 *   "fuse_trsm"    panels with at most this many rows under a leaf use the fused diagonal-block + TRSM kernel (8192)
 *   "fuse_rows64"  fused leaves with at most this many rows under them run 64-row consumer workgroups, one substitution
 *                  strip per SIMD (2048 = what fits the CUs reserved for the panel stream; 0 = always 128-row workgroups)
 *   "fuse_rows32", "fuse_rows16"  ... 32-row (2048) / 16-row (0 = never) consumer workgroups below that many rows: two / one strip
 *                  waves per CU -- every strip wave requests the same fragments of the diagonal block and a CU turns out ~32 bytes of
 *                  vector-load requests per cycle (round 5, bit-identical: N = 4096 1.158 -> 1.152 ms, N = 8192 4.346 -> 4.31 ms)
 *   "merge_urgent" 1 (default, with edge_flags): the two trailing updates per panel are one launch with a partial edge flag
 *                  (while it has at least 512 64x64 tiles: it needs an order table); "purg_rows" is then not applied
 *   "edge_flags"   1 (default): the per-panel dependencies of the look-ahead are flag words in device memory (last workgroup
 *                  of the producer raises it; a bounded in-kernel wait or a one-wave wait kernel on the consumer side)
 *                  instead of events; 0: events.  Used by an evaluation only while it is the only one in flight in the
 *                  process (idle contexts do not count; see gpt_concurrency_hint) on a context that owns its streams; off by
 *                  itself under rocprofv3 counter collection, for n > 12288, and for the rest of the process once a wait has
 *                  timed out (250 ms: the evaluation is then repeated on events)
 *   "tail_wait"    1 (default since round 6): the main stream's last launch of a panel awaits the NEXT panel's flag at its end instead of
 *                  a wait kernel in front of the next launch (C3 -19 us, C2 -15 us); not while "profile_gemm" times the launches (a
 *                  launch that waits at its end reports the wait as its duration); 0: always the wait kernel
 *   "skip_pad_rows" 1 (default): the trailing updates of a fit (gpt_fit*, gpt_fit_matrix) compute only the rows 0 ... N of the padded
 *                  factor of order NP = round_up(N + 1, 128) -- the data rows and the augmented row.  The up to 127 padding rows below are
 *                  zero left of a unit diagonal and stay so: the tiles that start below row N are not launched, and the tile row that
 *                  holds row N stores nothing below it (N = 8192: one 64-row tile row in 122 ... 2 per launch, C3 -0.06 ms).  Rows <= N,
 *                  ll, alpha, predictions and gradients are bit-identical to 0, which updates all NP rows; the padding entries can
 *                  differ in the sign of zero.  Not under "graph" (a captured factorisation is replayed for every N of one NP)
 *   "alpha_invalidate" (measurement aid) the next gpt_get_alpha recomputes alpha
 *   "eager_alpha"  1: every gpt_fit* also enqueues alpha = K_tot^-1 y behind its factorisation (the reference computes alpha in every
 *                  evaluation, gaussian_process.py:1462) and lands it in pinned memory under the call's own synchronisation;
 *                  gpt_get_alpha is then a host copy.  0 (default): alpha on first use (gpt_get_alpha, gpt_predict, gpt_ll_grad)
 *   "defer_pad"    1 (default): an eager evaluation whose N is a multiple of 512 (>= 1024) factors the last 128 columns of the padded
 *                  matrix -- the augmented row and the padding only -- on the main stream beside the substitution of alpha, which
 *                  follows the last real leaf at once (same bits); 0: everything on the panel stream, alpha behind it
 *   "binv_launches" 1 (measurement aid): the 512-wide block inverses by rounds 2-4's recursion over 15 launches instead of the one
 *                  launch of trinv512_kernel (solve.hip); results agree to rounding
 *   "splitk"       gpt_predict with std / cov at few points: the GEMMs of a triangular solve with at most 128 right-hand sides
 *                  and the V V^T of a covariance of at most 256 points, when k >= 1024 and they have fewer 32x32 tiles than this
 *                  (512), are split along k into up to 32 chunks of at least 256, summed in chunk order by a second kernel --
 *                  repeatable bit for bit, rounding differs from the unsplit sum; 0 = never split
 *   "helper_tf"    assumed rate of the helper stream (0.1 TFLOP/s per 24 CUs, 45) that takes a slice of the large trailing
 *                  updates on the reserved CUs when n > "helper_min_n" (12288); 0 = off
 *   "gemm_pad"     bytes of dummy dynamic LDS of the main-stream GEMM (residency cap)
 *   "dev_gemm_pad" the same for the device API's GEMM launches on this context (gpt_dev_gemm_nt, _stair, _gridstair), 0 = none
 *                  (default).  Measured in round 6 (profiles/r06_chain_contention.txt): with 24576 (two workgroups of a trailing
 *                  update per CU instead of five) an isolated m = 16384, k = 512 update keeps its rate (48.7 against 48.9 TFLOP/s)
 *                  and the serial chain beside it runs at 1.43 x its stand-alone time instead of 1.95 x -- but the partitioned
 *                  engines' staircase updates lose 10 % with it and the modelled 8-rank time does not improve: off
 *   "graph"        0/1: replay the factorisation from a captured hipGraph
 *   "timing"       0/1: record per-phase HIP events (gpt_last_timings)
 *   "profile_gemm" 0/1: HIP-event timing of each large GEMM launch (gpt_gemm_profile_read)
 *   "tile"         0 by launch size (default), 32, 64: force the GEMM macro-tile (bit-identical results either way)
 *   "debug_poison" 0/1 (test aid): gpt_ll_grad*, gpt_loo and gpt_loo_grad_diff fill their scratch matrices with NaN before use
 *   "edge_test_stall" 1 (test aid): the next evaluation's first flag is withheld once, so that the bounded wait, the repeat on
 *                  event edges and the switch of the process to event edges can be tested
 *   measured and off by default: "ramp", "inner" (1: left-looking panels, 2: once at most 4608 rows
 *   remain), "defer_rows", "nb_early", "nb_switch_rows".
 *   Removed in round 6 with the code behind them (each lost its A/B twice; NOTES_r04.md / NOTES_r05.md have the numbers, the
 *   history up to round 5's last commit the sources): "fuse_upd" / "fuse_upd_rows", "pair_rows", "leaf256", "tile" = 65 / 128 / 129,
 *   the environment switches GPT_GEMM_LOOP and GPT_GEMM_MIXED.
 *   Removed after round 6, frozen at their defaults because nothing set them (NOTES_r02.md, NOTES_r04.md, NOTES_r06.md and
 *   DESIGN.md section 4 have the A/B numbers): "early_rows", "late_rows", "late_pad", "late_pad_rows" (off), "panel_prio" (2),
 *   "head_wait_wgs" (33), "purg_rows_flags" (0), "merge_min_tiles" (512), "inner_rows" (4608), and the environment switches
 *   GPT_LATE_STREAM, GPT_RESERVE_EARLY, GPT_EDGE_WAITVALUE and GPT_EDGE_UNBOUNDED (every flag wait is bounded, always).
 *   gpt_ctx_set_option refuses unknown keys.
 * Environment: GPT_RESERVE_CUS (CUs the main stream leaves to the panel stream, default 32), GPT_TILE_ORDER
 * ("rows,cols,mode": supertile shape and deal of the GEMM's XCD-aware tile order, default 64,8,1), GPT_GRAD_TIMING,
 * GPT_EDGE_FLAGS=0 (event edges only: set it for jobs that share one GPU between several processes), GPT_GEMM_SMALL (64x64-tile count under which a GEMM launch uses 32x32 tiles, 512),
 * GPT_JITTER (test aid: random delay kernels in front of every dense launch), GPT_ALPHA_NARROW (measurement aid: gpt_get_alpha
 * by 128-wide substitution steps instead of the 512-wide block inverses), GPT_POTF2_LA=0 (the 128-column diagonal-block kernels
 * with the lock-step body of rounds 1-3 instead of the look-ahead body; results agree to rounding, not bit for bit). */
int gpt_ctx_set_option(gpt_ctx *ctx, const char *key, int64_t value);
int gpt_ctx_synchronize(gpt_ctx *ctx);
void *gpt_ctx_stream(gpt_ctx *ctx);
/* Number of flag edges (common.hpp: EdgeSig -- cross-stream dependencies carried by a word in device memory instead of an
 * event) the context has raised so far; diagnostics / tests. */
int64_t gpt_ctx_edge_count(gpt_ctx *ctx);
/* Announce (delta = +1) / retract (delta = -1) that the caller is about to run evaluations on several contexts of this
 * process concurrently (GaussianProcess.ll_batch: one host thread per context; ref gaussian_process.py:723-735, 1607-1692
 * are the reference's pool.map sites this replaces).  While the count is positive every evaluation keeps its look-ahead on
 * event edges (a kernel spinning on a flag must not share the hardware queues with a second chain).  Optional: without it
 * the library notices the overlap itself (the first two evaluations are serialised, then the process stays on event edges
 * while evaluations keep overlapping and for 100 ms after the last overlap).  Returns the new count. */
int gpt_concurrency_hint(int delta);

/* ---- Kernel.__call__ ---------------------------------------------------------------------- */
/* Replaces  Kernel.__call__(Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False) -> (M,) float64
 *   ref: kernel/core.py:220-257 (contract), kernel/squared_exponential.py:82-174,
 *        kernel/matern.py:512-555 -> kernel/_matern.pyx:14-32 -> kernel/src/matern.c:165-186
 *        (`double matern52(const double*, const double*, const int32_t*, const int32_t*, int32_t,
 *          const double*)`, kernel/include/matern.h:24-26), kernel/noise.py:76-110,123-152.
 * Element-wise pair list: row m of the four (M, D) inputs gives out[m].  params = the kernel's
 * full parameter vector ([sigma_f, l_1..l_D] for SE / Matern52, [sigma_n] for the noise kernels).
 * hyper_deriv = -1 for None.  noise_n: DiagonalNoiseKernel.n (D ints) or NULL (zeros).
 * All pointers are host pointers. */
int gpt_kpairs(gpt_ctx *ctx, int kernel_id, const double *params, int nparams,
               const double *Xi, const double *Xj, const int32_t *ni, const int32_t *nj,
               int64_t M, int D, int hyper_deriv, int symmetric, const int32_t *noise_n,
               double *out);

/* The same pair list for the PRODUCT of two native kernels (ProductKernel.__call__, ref: kernel/core.py:587-671). */
int gpt_kpairs2(gpt_ctx *ctx, int kernel_id1, const double *params1, int nparams1, int kernel_id2, const double *params2,
                int nparams2, const double *Xi, const double *Xj, const int32_t *ni, const int32_t *nj, int64_t M, int D,
                double *out);

/* ---- GaussianProcess.compute_Kij ---------------------------------------------------------- */
/* Replaces  GaussianProcess.compute_Kij(Xi, Xj, ni, nj, noise, hyper_deriv, k) -> (M, P)
 *   ref: gaussian_process.py:1535-1605.  Xj == NULL means Xj = Xi, nj = ni, symmetric = True
 *   (ref :1580-1585).  The (M*P, D) tiled temporaries of ref :1591-1594 are never formed: one
 *   fused kernel evaluates pair (i, j) from X rows held in registers/LDS and writes K[i*P + j].
 * K_out: host (M, P) row-major. */
int gpt_kbuild(gpt_ctx *ctx, int kernel_id, const double *params, int nparams,
               const double *Xi, const int32_t *ni, int64_t M,
               const double *Xj, const int32_t *nj, int64_t P, int D,
               int hyper_deriv, const int32_t *noise_n, double *K_out);

/* compute_Kij for the product of two native kernels (Xj == NULL: symmetric). */
int gpt_kbuild2(gpt_ctx *ctx, int kernel_id1, const double *params1, int nparams1, int kernel_id2, const double *params2,
                int nparams2, const double *Xi, const int32_t *ni, int64_t M, const double *Xj, const int32_t *nj, int64_t P,
                int D, double *K_out);

/* ---- GaussianProcess.add_data (device residency) ------------------------------------------ */
/* Uploads the training inputs the later calls use (ref: gaussian_process.py:376-503 defines the
 * host layout: X (N, D) float64, n (N, D) int).  Invalidates any factorisation. */
int gpt_set_data(gpt_ctx *ctx, const double *X, const int32_t *n, int64_t N, int D);

/* Linear transform of the latent values: observations y = T f(X) + noise (ref: gaussian_process.py:376-503 argument
 * `T` of add_data; :1443-1446, :966-970).  T is (Ny, N) row-major over the N resident points.  With a transform set,
 * gpt_fit expects y, err_y of length Ny and factors K_tot = T (K + noise_var I) T^T + diag(err_y^2) + diag_add I
 * (Ny x Ny; the products are fp64-MFMA GEMMs on the device), and gpt_predict applies T to the training side of
 * Kstar.  gpt_set_data drops the transform; T == NULL removes it. */
int gpt_set_T(gpt_ctx *ctx, const double *T, int64_t Ny);

/* Input warp of the model kernel (ref: kernel/warping.py:464-531, WarpedKernel around a native model): k(w(x), w(x')) with an
 * elementwise warp w made of `nlayers` layers (1 .. GPT_WARP_MAX_LAYERS, layer 0 applied first), `types[l]` one of GPT_WARP_*,
 * `params` nlayers x 2 D doubles -- layer l, dimension d: (a_d, b_d) of the linear warp, (alpha_d, beta_d) of the beta warp.
 * While layers are set, gpt_kbuild / gpt_kbuild2 (for the kernels gpt_fit takes; the noise kernels are never warped), gpt_fit /
 * gpt_fit_sum / gpt_fit_terms (with and without T) and gpt_predict (hence gpt_cov_sample) evaluate the kernel on w(X), and an
 * entry whose row (column) point carries derivative order 1 in dimension d is multiplied by w_d'(x_d): the chain rule.  Only
 * orders 0 and 1 have that form: an order above 1 in the resident data, in X* or in gpt_kbuild's points is GPT_E_VALUE
 * ("Derivative orders greater than one are not supported!"), found on the host before anything is launched.
 * The beta warp wants its input in [0, 1]: NaN outside (and for alpha <= 0 or beta <= 0), exactly 0 / 1 at the ends.
 * The call warps the resident points (O(N D) on the device: warp_points_kernel) and drops the resident factorisation; the
 * layers hold until gpt_set_data or gpt_set_warp(ctx, 0, NULL, NULL).  Needs gpt_set_data first (GPT_E_STATE).
 * gpt_set_warp(ctx, 0, ...) with no layers set changes nothing (the resident factorisation stays).
 * Not available while layers are set (GPT_E_NOTIMPL, gpt_last_error says so): gpt_ll_grad, gpt_ll_grad_diff, gpt_predict_batch, gpt_plan_create /
 * gpt_plan_run over this context, and gpt_fit_batch* unless gpt_set_warp_batch gave the batch its own warps. */
int gpt_set_warp(gpt_ctx *ctx, int nlayers, const int *types, const double *params);

/* The warps of a BATCH: warp parameters are hyperparameters and differ from element to element.  `params` holds nbatch x nlayers x
 * 2 D doubles (element-major, then as gpt_set_warp); the layer types are shared.  One launch fills nbatch x N x D warped points and
 * nbatch x N slope factors; the next gpt_fit_batch* -- which must have the same nbatch (GPT_E_ARG otherwise) -- builds element b
 * from its own and consumes them: element b carries the bits gpt_set_warp + gpt_fit_terms give for that element alone.  The
 * context's single layers and resident factorisation are untouched.  nlayers == 0 or nbatch == 0 drops a pending set.
 * gpt_predict_batch answers GPT_E_NOTIMPL for a batch that was fitted with warps.  Orders above 1 in the data: GPT_E_VALUE. */
int gpt_set_warp_batch(gpt_ctx *ctx, int nbatch, int nlayers, const int *types, const double *params);

/* ---- GaussianProcess.compute_K_L_alpha_ll ------------------------------------------------- */
/* Replaces the T-free body of GaussianProcess.compute_K_L_alpha_ll   ref: gaussian_process.py:1428-1467
 *   K_tot = K + noise_var*I + diag(err_y^2) + diag_add*I          (ref :1431-1451; diag_add = diag_factor*eps)
 *   L     = cholesky(K_tot, lower)                                (ref :1452, LAPACK dpotrf)
 *   z     = L^-1 y  ;  ll_data = -1/2 z.z - sum(log L_ii) - N/2 log(2 pi)    (ref :1462-1467)
 * y is the mean-subtracted target (ref :1455-1461); the log-prior (ref :1469) is added by the
 * caller.  K_tot / L stay resident in HBM; alpha (ref :1462) is computed on demand by
 * gpt_get_alpha.  err_y: (N,) host.  Only `params` need change between calls (MAP loop). */
int gpt_fit(gpt_ctx *ctx, int kernel_id, const double *params, int nparams, double noise_var,
            const double *y, const double *err_y, double diag_add,
            double *ll_data_out, double *logdet_half_out);

/* The same for a model kernel that is a SUM of native kernels (SumKernel, ref: kernel/core.py:549-584, k1 + k2 + ...):
 * nterms <= 8 kernel ids, their parameter vectors concatenated in `params` (nparams[t] entries each).  One builder pass
 * per term, accumulated on the device; everything else as gpt_fit (which is the nterms == 1 case).  gpt_predict
 * afterwards uses the same sum. */
int gpt_fit_sum(gpt_ctx *ctx, int nterms, const int *kernel_ids, const double *params, const int *nparams,
                double noise_var, const double *y, const double *err_y, double diag_add, double *ll_data_out,
                double *logdet_half_out);

/* gpt_fit_sum with PRODUCT terms: term t is kernel_ids[t] alone (kernel_ids2[t] < 0) or the product kernel_ids[t] *
 * kernel_ids2[t]; its parameters are nparams[t] consecutive entries of `params`, the first nparams1[t] of them the first
 * factor's (nparams1[t] == nparams[t] for a plain term).  A model like k1 * k2 + k3 therefore runs the fused builder, not a
 * host-assembled K_tot through gpt_fit_matrix.  gpt_predict afterwards uses the same terms. */
int gpt_fit_terms(gpt_ctx *ctx, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                  const int *nparams, const int *nparams1, double noise_var, const double *y, const double *err_y,
                  double diag_add, double *ll_data_out, double *logdet_half_out);

/* nbatch INDEPENDENT evaluations of the resident data set in one launch sequence: element b uses params[b * nparams ..],
 * noise_var[b] and the target y[b * N ..] (the mean function may depend on the hyperparameters); err_y (N) is shared.
 * Replaces the loops over hyperparameter vectors of the reference's likelihood grid and random starts
 * (ref: gaussian_process.py:1607-1692, :723-735, gp_utils.py:98-115) at the sizes those run at: N <= 8192 resident
 * points (it pays up to N ~ 4096: 2.3x one gpt_fit per vector there, 9.5x at 1024; nbatch N^2 doubles of device memory), one native kernel
 * (sums, products and a linear transform: gpt_fit_batch_sum / gpt_fit_batch_terms below).
 * Every kernel of the factorisation carries the batch in a grid dimension; an element's results are bit-identical to
 * gpt_fit's for the same inputs.  info_out[b] = 0, or the LAPACK index of the leading minor that is not positive
 * definite (ll_data_out[b] is then meaningless); the call itself returns GPT_OK in both cases. */
int gpt_fit_batch(gpt_ctx *ctx, int nbatch, int kernel_id, const double *params, int nparams,
                  const double *noise_var, const double *y, const double *err_y, double diag_add,
                  double *ll_data_out, double *logdet_half_out, int32_t *info_out);

/* The same for a SumKernel of native kernels (ref: kernel/core.py:549-584; gpt_fit_sum for one matrix): element b's
 * parameters are the terms' parameters concatenated, params[b * ptot ..] with ptot = sum of nparams[t].  Bit-identical to
 * gpt_fit_sum per element. */
int gpt_fit_batch_sum(gpt_ctx *ctx, int nbatch, int nterms, const int *kernel_ids, const double *params,
                      const int *nparams, const double *noise_var, const double *y, const double *err_y,
                      double diag_add, double *ll_data_out, double *logdet_half_out, int32_t *info_out);

/* The batched evaluator for every model gpt_fit_terms takes: product terms (kernel_ids2 / nparams1 as in gpt_fit_terms) and, when
 * gpt_set_T has set one, the linear transform (y then holds nbatch x Ny targets, err_y Ny entries; K_tot = T (K + noise_var I) T^T +
 * ... per element by two batched GEMMs with the shared T).  Needs Nx, Ny <= 8192; bit-identical to gpt_fit_terms per element.
 * ref: gaussian_process.py:1607-1692, gp_utils.py:98-115 (the reference's grids work for any model). */
int gpt_fit_batch_terms(gpt_ctx *ctx, int nbatch, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                        const int *nparams, const int *nparams1, const double *noise_var, const double *y, const double *err_y,
                        double diag_add, double *ll_data_out, double *logdet_half_out, int32_t *info_out);

/* Free / total bytes of the context's GPU, and the release of the batched evaluator's scratch (nbatch matrices; otherwise kept
 * until gpt_ctx_destroy): GaussianProcess.ll_batch sizes its chunks by the first and returns the memory with the second. */
int gpt_mem_info(gpt_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
int gpt_release_batch_scratch(gpt_ctx *ctx);

/* Prediction from the RESIDENT BATCH: every element of the last successful gpt_fit_batch* at the same M test points -- the
 * reference's prediction marginalised over a hyperparameter trace (ref: gaussian_process.py:1840-1987 compute_from_MCMC,
 * :2144-2254 predict_MCMC: one update_hyperparameters + predict per trace row).  Per element b, as gpt_predict:
 *   V_b = K*_b^T L_b^-T,  mean_b = V_b z_b (z_b = L_b^-1 y_b, the fit's augmented row),  var_b = diag K**_b - rowsumsq(V_b),
 *   cov_b = K**_b - V_b V_b^T.
 * Xstar (M, D) / nstar (M, D) test points and derivative orders (the order checks of gpt_predict).  noise_n != NULL (D orders):
 * element b's own noise variance (the fit's noise_var[b]) is added where a row of nstar equals noise_n (ref: noise.py:103-104).
 * keep (nbatch): 0 skips element b -- its rows of the outputs are not written and it takes no part in cov_sum_out (pass
 * keep[b] = (info_out[b] == 0): a factor that is not positive definite must be skipped).  Outputs (host, row-major):
 *   mean_out (nbatch, M); var_out (nbatch, M) or NULL; cov_out (nbatch, M, M), full symmetric, or NULL;
 *   cov_sum_out (M, M) = sum over kept b of cov_b (full symmetric), or NULL: built on the device without the per-element
 *   matrices -- one pass for sum_b K**_b and ONE GEMM over the contraction (b, i) -- so it crosses PCIe once per call.
 * GPT_E_STATE: no batch resident (before any gpt_fit_batch*, after one that failed, and after gpt_set_data, gpt_set_T,
 * gpt_cov_sample or gpt_release_batch_scratch); GPT_E_NOTIMPL with a linear transform set.  The resident batch is unchanged. */
int gpt_predict_batch(gpt_ctx *ctx, const double *Xstar, const int32_t *nstar, int64_t M, const int32_t *noise_n,
                      const int32_t *keep, double *mean_out, double *var_out, double *cov_out, double *cov_sum_out);

/* The loop of an affine-invariant ENSEMBLE SAMPLER (Goodman & Weare's stretch move; what the reference drives emcee for, ref:
 * gaussian_process.py:1694-1838) over nfree free hyperparameters of the resident data set's model, inside the library: one step is
 * two dependent batches of nwalkers / 2 evaluations, each ONE launch sequence of the batched fit above, and no caller code runs
 * between them.  For a model without mean function and warp whose prior is a box:
 *   the model as gpt_fit_batch_terms takes it (kernel_ids, kernel_ids2, nparams, nparams1) and base_params, its complete parameter
 *   vector (sum of nparams doubles): the values of the parameters that are not free;
 *   free_idx[f]: the place of free parameter f in that vector, or its LENGTH for the noise sigma (squared for the fit; at most one);
 *   noise_var is the noise variance when the sigma is not free;
 *   lo / hi (nfree): the box, both ends inside; log_prior: the constant log-density inside it; y, err_y, diag_add as gpt_fit_batch_terms
 *   takes them for ONE element (the targets are every element's);
 *   u_stretch, partner, u_accept (nsteps, nwalkers): the variates, drawn beforehand.  Walkers [0, nwalkers / 2) are the first
 *   half.  Per step the first half moves against the second, then the second against the first; walker w of the moving half S
 *   against the other half C:  t = (a - 1) u_stretch[w] + 1, z = t t / a, q = C[partner[w]] - z (C[partner[w]] - S[w]) (partner
 *   indexes INTO C), accepted where (nfree - 1) log z + lnp(q) - lnp(S[w]) > log u_accept[w];
 *   lnp(q) = -inf outside the box (not evaluated), for parameters the model refuses (as gpt_fit_terms would, e.g. a length scale
 *   that is not positive), for a matrix that is not positive definite and for a NaN; else ll_data + log_prior;
 *   max_chunk: most elements of one launch sequence (the caller's memory budget); a chunk that answers GPT_E_NOMEM is halved.
 * pos (nwalkers, nfree) and lnp (nwalkers): the walkers and their log-probabilities, in and out.  Outputs: chain (nsteps, nwalkers,
 * nfree) and lnp_chain (nsteps, nwalkers), the state after every step; naccept (nwalkers), the accepted moves of this run.
 * The same variates give the chain of gptools_amd.sampler.EnsembleSampler's Python loop over GaussianProcess.ll_batch bit for bit.
 * Leaves the context as gpt_fit_batch_terms does (the last chunk is the resident batch; the resident factorisation is untouched);
 * any error of a launch sequence other than GPT_E_NOMEM ends the run with that status. */
int gpt_ensemble_run(gpt_ctx *ctx, int nterms, const int *kernel_ids, const int *kernel_ids2, const int *nparams, const int *nparams1,
                     const double *base_params, int nfree, const int32_t *free_idx, const double *lo, const double *hi,
                     double log_prior, const double *y, const double *err_y, double diag_add, double noise_var, int nwalkers,
                     int nsteps, double a, const double *u_stretch, const int32_t *partner, const double *u_accept, int max_chunk,
                     double *pos, double *lnp, double *chain, double *lnp_chain, int32_t *naccept);

/* Same as gpt_fit but for an explicit, caller-assembled symmetric K_tot (host, (N, N) row-major;
 * only the lower triangle is read): used for the `T` (linear transform) branch,
 * ref: gaussian_process.py:1443-1446, where K_tot = T (K + noise_K) T^T + ... is (N_y, N_y). */
int gpt_fit_matrix(gpt_ctx *ctx, const double *K_tot, int64_t N, const double *y,
                   double *ll_data_out, double *logdet_half_out);

/* State read-back (host outputs).  L: (N, N) lower, strict upper zero like scipy.linalg.cholesky
 * (ref: gaussian_process.py:1452).  alpha: (N,) = K_tot^-1 y (ref :1462). */
int gpt_get_L(gpt_ctx *ctx, double *L_out);
int gpt_get_alpha(gpt_ctx *ctx, double *alpha_out);

/* ---- GaussianProcess.predict (non-MCMC branch) -------------------------------------------- */
/* Analytic gradient of the LML data term (ref: gaussian_process.py:1471-1520), after gpt_fit / gpt_fit_sum (no transform):
 *   out[h]  = 1/2 * sum_ab (alpha_a alpha_b - (K_tot^-1)_ab) * dK[a][b] / d theta_h      for h < nh, where theta_h is
 *             parameter local_idx[h] (0 = sigma_f, j = l_j) of kernel term term_idx[h];
 *   out[nh] = 1/2 * (alpha^T alpha - tr K_tot^-1)   (times 2 sigma_n this is the derivative for a DiagonalNoiseKernel).
 * K_tot^-1 is formed on the device from the resident factor (triangular inverse + U U^T on the MFMA GEMM, ~N^3 flop
 * whatever nh is -- the reference spends 2 N^3 per parameter in cho_solve); dK is never materialised.
 * Squared-exponential terms only (GPT_E_NOTIMPL otherwise, like matern.py:543-544). */
int gpt_ll_grad(gpt_ctx *ctx, int nh, const int *term_idx, const int *local_idx, double *out);

/* The same gradient for EVERY kernel the fits take -- Matern52, Matern, RationalQuadratic, the Gibbs families, products,
 * GPT_KERNEL_ON_DIM factors -- by central differences of the pair function, taken PER PAIR before the weight:
 *   out[h]  = 1/2 * sum_ab (alpha_a alpha_b - (K_tot^-1)_ab) * (k_b - k_a)[a][b] / denom[h]      for h < nh,
 *   out[nh] = the noise trace term, the value gpt_ll_grad returns there (with a transform T: over the observations).
 * term_idx[h] names a term of the resident model (gpt_fit / gpt_fit_sum / gpt_fit_terms); k_a and k_b are that term with the
 * parameters the caller gives for the two stencil points of parameter h: params_a and params_b hold, concatenated over h, the
 * term's COMPLETE parameter vector in the layout gpt_fit_terms took (a product's two factors together), so entry h starts where
 * the vectors of the entries before it end.  denom[h] = theta_b - theta_a as the caller formed it in floating point (0, NaN or
 * an infinity: GPT_E_ARG).  The other terms of the sum cancel exactly and are not evaluated.
 * Cost: K_tot^-1 as gpt_ll_grad (~N^3 flop whatever nh is), then two O(N^2) evaluations of ONE term per entry -- against a whole
 * factorisation per parameter when the likelihood itself is differenced.  GPT_GRAD_MAXH entries of one term share a launch.
 * Deterministic: repeated calls return the same bits.  Accuracy: with a relative step of 6e-6 the truncation and rounding errors
 * meet near 1e-7 of the largest gradient entry.
 * Errors: GPT_E_STATE without a factorisation made by a fit of kernels (gpt_fit_matrix leaves none); GPT_E_NOTIMPL while warp
 * layers are set; every stencil point is checked as the parameters of a fit are (parameter domains, derivative orders) and the
 * first refusal is the call's status, before anything is launched. */
int gpt_ll_grad_diff(gpt_ctx *ctx, int nh, const int *term_idx, const double *params_a, const double *params_b,
                     const double *denom, double *out);

/* gpt_ll_grad_diff for every element of the RESIDENT BATCH (the last successful gpt_fit_batch*), one launch sequence and one host
 * synchronisation for all of them -- the gradient half of a multi-start optimiser's lockstep round.  nh and term_idx[nh] are shared
 * by the elements (term_idx names terms of the batch's model); per element b the stencil points and steps:
 *   params_a, params_b: [b][h], entry h its term's complete parameter vector as in gpt_ll_grad_diff (every element's row has the
 *   same length, the sum over h of the terms' parameter counts);  denom: [b][h].
 * keep (nbatch): 0 skips element b (pass keep[b] = (info_out[b] == 0)); its stencil is not read and its rows come back as NaN.
 * Outputs (host): out (nbatch, nh + 1), row b the entries gpt_ll_grad_diff returns for element b, the noise trace
 * 1/2 sum_i (alpha_i^2 - (K_tot^-1)_ii) last; alpha_out (nbatch, N) or NULL: alpha_b = K_tot,b^-1 y_b (the mean function's entries
 * are the host's).  Every stencil point of every kept element is checked as in gpt_ll_grad_diff before anything is launched.
 * An element's row does not depend on nbatch, on its place in the batch or on the other elements (same launch geometry and
 * summation order whatever the batch is); repeated calls return the same bits.  The batch stays resident: gpt_predict_batch
 * afterwards returns what it returned before.  Scratch (two nbatch x NP x NP matrices) in slots of its own, which
 * gpt_release_batch_scratch frees.
 * GPT_E_STATE: no batch resident (as gpt_predict_batch); GPT_E_NOTIMPL for a batch fitted with warps, while warp layers are set and
 * with a linear transform (gpt_set_T). */
int gpt_ll_grad_diff_batch(gpt_ctx *ctx, int nh, const int *term_idx, const double *params_a, const double *params_b,
                           const double *denom, const int32_t *keep, double *out, double *alpha_out);

/* ---- leave-one-out cross-validation (Rasmussen & Williams 5.4.2) ----------------- */
/* With W = K_tot^-1 over the N observations, alpha = W (y - T mu) and d_i = W_ii, from the resident factor:
 *   resid[i] = alpha_i / d_i = y_i - m_i, m_i the prediction at point i of the model that has not seen it;
 *   var[i]   = 1 / d_i, that prediction's variance (the noise of point i included);
 *   *loo_ll  = sum_i [ 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 pi ], the leave-one-out log predictive probability.
 * resid and var: N doubles each, or NULL.  The diagonal comes from the triangular inverse alone, d_i = sum_k (L^-T)_ik^2: ~N^3 / 3
 * flop, no K_tot^-1.  Needs nothing but a resident factor: every fit serves (gpt_fit*, gpt_fit_matrix, with warp layers, with a
 * transform T -- N is then the number of observations).  Deterministic: the terms are added in index order, repeated calls return
 * the same bits. */
int gpt_loo(gpt_ctx *ctx, double *loo_ll, double *resid, double *var);

/* The gradient of that value with respect to kernel parameters, in the shape of gpt_ll_grad_diff -- same arguments, same checks,
 * same launch groups -- with the weights of the pair pass replaced:
 *   out[h]  = 1/2 * sum_ab (u_a alpha_b + alpha_a u_b - V_ab) * (k_b - k_a)[a][b] / denom[h]      for h < nh,
 *   out[nh] = 1/2 * sum_i (2 u_i alpha_i - V_ii)      (times 2 sigma_n: the derivative for a DiagonalNoiseKernel),
 * where u = W resid, V = W diag(e) W and e_i = (1 + alpha_i^2 / d_i) / d_i.  Also returns what gpt_loo returns (loo_ll, resid, var:
 * each may be NULL) and u (N doubles or NULL): a mean function's parameter theta has the derivative u^T d mu / d theta.
 * Cost: K_tot^-1 as gpt_ll_grad_diff, one more NP^3 flop for V = A A^T (A = W diag(sqrt e)) whatever nh is, then the O(N^2) pair
 * passes.  Deterministic.
 * Errors: those of gpt_ll_grad_diff, and GPT_E_NOTIMPL with a linear transform T resident (dK_tot = T dK T^T: the weights would
 * have to be carried to the latent points). */
int gpt_loo_grad_diff(gpt_ctx *ctx, int nh, const int *term_idx, const double *params_a, const double *params_b,
                      const double *denom, double *out, double *loo_ll, double *resid, double *var, double *u);

/* Replaces  ref: gaussian_process.py:965-1006 for the T-free, untransformed case:
 *   Kstar = K(X, Xstar) ; mean = Kstar^T alpha ; v = L^-1 Kstar ; cov = K(Xstar,Xstar) - v^T v ;
 *   std = sqrt(diag(cov)).
 * want: 0 = mean only, 1 = mean + std, 2 = mean + cov (M, M) (+ std if std_out != NULL).
 * noise_params != NULL adds the DiagonalNoiseKernel term to K(Xstar, Xstar) (ref :985-986,
 * kernel/noise.py:103-104; the X-vs-Xstar term of ref :967-968 is identically zero because that
 * call is not `symmetric`, kernel/noise.py:109-110).
 * Uses the kernel / params of the last gpt_fit.
 * cov_out may be pageable or pinned host memory (gpt_host_alloc): into pinned memory the block rows of the covariance are
 * written by asynchronous DMA while the next block column of the SYRK is computed; pageable memory is reached through a
 * pinned staging ring.  want == 2 with cov_out == NULL leaves the covariance on the device (nothing of size M^2 crosses
 * PCIe; mean and, if std_out != NULL, std are still returned). */
int gpt_predict(gpt_ctx *ctx, const double *Xstar, const int32_t *nstar, int64_t M, int want,
                const double *noise_params, const int32_t *noise_n,
                double *mean_out, double *std_out, double *cov_out);

/* Posterior samples from the predictive covariance left on the device by gpt_predict(want = 2, cov_out = NULL)
 * (ref: gaussian_process.py:1295-1300, :1330 -- draw_sample with rand_vars, method = 'cholesky'):
 *   out (M x S, row-major) = cholesky(cov + diag_add I, lower) * rand (M x S, row-major);  the caller adds the mean.
 * M must be the M of that gpt_predict call (GPT_E_ARG otherwise).
 * The M x M covariance never leaves the device; the fit's resident factor is untouched; the covariance is consumed.
 * Status > 0: that leading minor is not positive definite (numpy.linalg.LinAlgError, as scipy.linalg.cholesky). */
int gpt_cov_sample(gpt_ctx *ctx, int64_t M, double diag_add, const double *rand, int64_t S, double *out);

/* Generic right-hand sides against the resident factor (host in/out, row-major):
 *   gpt_solve_L   : B (N, nrhs) <- L^-1 B          (ref: gaussian_process.py:983 solve_triangular)
 *   gpt_cho_solve : B (N, nrhs) <- K_tot^-1 B      (ref: gaussian_process.py:1462,1487,1503 cho_solve) */
/* Pinned (page-locked) host memory for large results: hipHostMalloc / hipHostFree behind a C ABI, so that a binding can hand
 * gpt_predict a destination the DMA engine writes directly. */
int gpt_host_alloc(int64_t bytes, void **out);
int gpt_host_free(void *p);

int gpt_solve_L(gpt_ctx *ctx, double *B, int64_t nrhs);
int gpt_cho_solve(gpt_ctx *ctx, double *B, int64_t nrhs);

/* Per-phase timings of the last gpt_fit in milliseconds (HIP events on the context's stream):
 * out[0]=upload, [1]=kbuild, [2]=potrf, [3]=ll tail, [4]=total; returns the count written. */
int gpt_last_timings(gpt_ctx *ctx, double *out_ms, int n);

/* With option "profile_gemm" = 1 every large (>= 1 GFLOP) trailing-update GEMM/SYRK launch is bracketed
 * by HIP events on the stream it runs on.  Reads and resets the accumulators:
 * out3[0] = algorithmic flops (2k per computed element of C, lower trapezoid for SYRK-style launches),
 * out3[1] = summed launch durations in ms, out3[2] = number of launches. */
int gpt_gemm_profile_read(gpt_ctx *ctx, double *out3);
/* The same with out4[3] = the launches' ALGORITHMIC bytes (16 B per computed element of C -- read and written once -- plus the
 * operand panel once, 8 k max(m, n)): what bench.py's roofline sets the measured HBM traffic of the same launches against. */
int gpt_gemm_profile_read4(gpt_ctx *ctx, double *out4);

/* Standalone dense kernels on host matrices (used by parity tests and the roofline bench). */
int gpt_potrf_host(gpt_ctx *ctx, double *A, int64_t N);                 /* in place, lower */
int gpt_gemm_nt_host(gpt_ctx *ctx, int64_t m, int64_t n, int64_t k, double alpha, const double *A,
                     const double *B, double beta, double *C);          /* C = beta C + alpha A B^T */

/* ---- device API --------------------------------------------------------------------------- */
/* All pointers below are DEVICE pointers unless marked host; work is enqueued on the context's
 * stream and NOT synchronised.  Leading dimensions are in elements.  Block sizes: every m, n, k
 * passed to the dense routines must be a multiple of 64 (callers pad). */

/* Fused covariance builder on device data.  Writes the (M, P) block K[i][j], i in [0,M), j in
 * [0,P) of k(Xi[i], Xj[j], ni[i], nj[j]) to dK (row stride ldk).  lower_only != 0: only tiles
 * that intersect {i + i0 >= j + j0} are written (i0, j0 = global offsets of the block).  If
 * d_err_y != NULL, entries with i + i0 == j + j0 get ((k + noise_var) + err_y[i+i0]^2) + diag_add. */
int gpt_dev_kbuild(gpt_ctx *ctx, int kernel_id, const double *params_host, int nparams,
                   const double *dXi, const int32_t *dni, int64_t M,
                   const double *dXj, const int32_t *dnj, int64_t P, int D,
                   int hyper_deriv, int symmetric, const int32_t *noise_n_host,
                   int lower_only, int64_t i0, int64_t j0,
                   const double *d_err_y, double noise_var, double diag_add,
                   double *dK, int64_t ldk);

/* C (m x n) = beta*C + alpha * A (m x k) * B (n x k)^T.  tri != 0: C's origin lies on the global
 * diagonal and only 64-aligned tiles with col_tile <= row_tile are computed (SYRK-style). */
int gpt_dev_gemm_nt(gpt_ctx *ctx, int64_t m, int64_t n, int64_t k, double alpha,
                    const double *dA, int64_t lda, const double *dB, int64_t ldb,
                    double beta, double *dC, int64_t ldc, int tri);
/* Block-cyclic trailing update in one launch: C (m x nseg*seg_cols, ldc) += alpha * A * B_q^T + beta-scaled C, where
 * column segment q (seg_cols columns) uses the B rows starting at row q * b_stride and only its rows >= q * row_step
 * are updated (lower trapezoid inside the segment; its diagonal block sits at row q * row_step).  With A = B = the
 * received panel this applies panel k to all block columns a rank owns to the right of it (they are adjacent in the
 * rank's storage, world * nb apart in the matrix): gptools_amd/dist.py, SURVEY.md section 8e.
 * seg_cols, row_step multiples of 64; k a multiple of 16; b_stride >= seg_cols. */
int gpt_dev_gemm_nt_stair(gpt_ctx *ctx, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha,
                          const double *dA, int64_t lda, const double *dB, int64_t ldb, int64_t b_stride,
                          int64_t row_step, double beta, double *dC, int64_t ldc);

/* Trailing update of one rank of the 2-D block-cyclic engine (gptools_amd/dist.py GridLML) in
 * one launch.  The rank holds the global block rows I = pr + li * den and block columns J = pc + lj * num of the matrix (block
 * size seg_cols both ways).  C = its local matrix from the update's first block row / column on, A (m x k) = the rank's rows of
 * the panel, B = its columns of the panel (column segment q: rows [q * seg_cols, (q + 1) * seg_cols)).  Segment q (global block
 * column J0 + q * num) is updated from its first block row with I >= J on: local block row ceil((off + q * num) / den) - base,
 * with off = J0 - pr and base = the local index of the update's first block row; where that first block is a diagonal block
 * of the matrix ((off + q * num) % den == 0) only its lower 64 x 64 tiles are computed.  The reference has nothing to mirror here
 * (gaussian_process.py:1452 is one LAPACK call). */
int gpt_dev_gemm_nt_gridstair(gpt_ctx *ctx, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha,
                              const double *dA, int64_t lda, const double *dB, int64_t ldb, int64_t off, int64_t num,
                              int64_t den, int64_t base, double beta, double *dC, int64_t ldc);
/* d_acc[0] += sum_{c < w} d_row[c]^2: the z.z part of ll (ref gaussian_process.py:1463) from the piece of the augmented row a
 * rank of that engine holds (one workgroup, fixed order). */
int gpt_dev_row_sumsq(gpt_ctx *ctx, const double *d_row, int64_t w, double *d_acc);

/* Factor one block column ("panel"): A is (m x nb), its top nb x nb block is the diagonal block.
 * On exit the top block holds L_kk (lower) and the rows below hold A21 * L_kk^-T.  d_invd:
 * workspace/output of GPT_WS_BLOCK (= 9216) doubles per 128 columns: the inverses of L's 16x16 diagonal
 * blocks and L's strictly-lower 16x16 blocks, packed in MFMA operand order for the panel TRSM.
 * d_info: int32 on device, set to info_base + j + 1 at the first non-positive pivot (never
 * cleared here). */
int gpt_dev_potrf_panel(gpt_ctx *ctx, int64_t m, int64_t nb, double *dA, int64_t lda,
                        double *d_invd, int32_t *d_info, int64_t info_base);

/* Whole lower Cholesky of the n x n matrix dA in place (blocked right-looking, look-ahead).
 * d_invd: (n/128)*GPT_WS_BLOCK doubles. */
int gpt_dev_potrf(gpt_ctx *ctx, int64_t n, double *dA, int64_t lda, double *d_invd, int32_t *d_info);

/* B (m x n) <- B * L^-T with L (n x n) lower, d_invd from the factorisation of L. */
int gpt_dev_trsm_rlt(gpt_ctx *ctx, int64_t m, int64_t n, const double *dL, int64_t ldl,
                     const double *d_invd, double *dB, int64_t ldb);

/* dW (n x n, row-major, ldw; zeros above the diagonal) <- L^-1, L (n x n) a factored diagonal block, d_invd from its
 * factorisation.  The TRSM of many rows then is one GEMM: gpt_dev_gemm_nt(m, n, n, 1, B, ldb, dW, ldw, 0, X, ldx, 0)
 * gives X = B L^-T (the reference reaches the same quantity through scipy.linalg.cho_factor / LAPACK dtrsm inside
 * dpotrf, gaussian_process.py:1452). */
int gpt_dev_trinv(gpt_ctx *ctx, int64_t n, const double *dL, int64_t ldl, const double *d_invd,
                  double *dW, int64_t ldw);

/* Small helpers of the one-process-per-GPU path (gptools_amd/dist.py), so that its queues carry no generic framework
 * kernels.  All asynchronous on the context's stream.
 *   gpt_dev_copy2d       : dst (rows x cols, ldd) <- src (rows x cols, lds) -- staging a block column of the local matrix
 *                          into a contiguous panel buffer.
 *   gpt_dev_pad_block    : rows [n_valid, n_pad) of a block column whose first column has global index c0 (nb columns,
 *                          row-major at dA = its element (row 0 of the matrix, column c0), row stride lda): the augmented row
 *                          n_valid gets y[c0 + c] (c0 + c < n_valid), the diagonal of the padding 1, the pivot under the
 *                          augmented row `big`, everything else 0 (layout of DESIGN.md section 3).
 *   gpt_dev_panel_scalars: d_acc[0] += sum_{i < w} log P[i][i]; if zrow >= 0 also d_acc[1] += sum_{c < w} P[zrow][c]^2 --
 *                          the two scalars of ll (ref gaussian_process.py:1463-1467) taken from a factored panel buffer
 *                          (P = its diagonal block, row stride ldp); accumulated in a fixed order (one workgroup). */
int gpt_dev_copy2d(gpt_ctx *ctx, int64_t rows, int64_t cols, const double *d_src, int64_t lds, double *d_dst, int64_t ldd);
/* The same copy on an explicit stream of the caller (a hipStream_t; NULL = the context's): the column exchange of the 2-D
 * engine gathers / scatters panel blocks on a queue that carries nothing else and has no context of its own. */
int gpt_dev_copy2d_on(gpt_ctx *ctx, void *stream, int64_t rows, int64_t cols, const double *d_src, int64_t lds, double *d_dst,
                      int64_t ldd);
int gpt_dev_pad_block(gpt_ctx *ctx, double *dA, int64_t lda, int64_t c0, int64_t nb, int64_t n_valid, int64_t n_pad,
                      const double *d_y, double big);
int gpt_dev_panel_scalars(gpt_ctx *ctx, const double *dP, int64_t ldp, int64_t w, int64_t zrow, double *d_acc);

/* ---- inducing-point approximations: FITC, VFE, DTC -------------------------------------------------
 * M inducing inputs Z (M, D) with derivative orders nZ (M, D; NULL: all zero) stand in for the N resident training points:
 * O(N M^2) time, O(M^2 + chunk M) memory.  With s_i = noise_var + err_y_i^2 and the jitter on the diagonal of K_uu:
 *   L_u = chol(k(Z, Z) + jitter I),  V = L_u^-1 k(Z, X),  q_i = sum_m V_mi^2,  k_i = k(x_i, x_i)
 *   Lambda_i = k_i - q_i + s_i (fitc),  Lambda_i = s_i (vfe, dtc)
 *   B = I + V Lambda^-1 V^T,  L_B = chol(B),  c = L_B^-1 V Lambda^-1 y
 *   ll = -1/2 [sum log Lambda_i + 2 sum log (L_B)_mm + y^T Lambda^-1 y - c.c + N log 2 pi]  - 1/2 sum (k_i - q_i) / s_i (vfe only)
 *   predict at x*:  v = L_u^-1 k(Z, x*),  w = L_B^-1 v,  mean = w.c,  cov = k(x*, x*') - v.v' + w.w'
 * The sparse state lives beside the dense factor of the same context; neither touches the other.  gpt_set_data and
 * gpt_sparse_set_inducing drop it.  With a linear transform (gpt_set_T) or warp layers (gpt_set_warp) set the calls answer
 * GPT_E_NOTIMPL; without data or inducing points (gpt_sparse_predict / gpt_sparse_get_c: without a sparse fit that succeeded)
 * GPT_E_STATE. */
#define GPT_SPARSE_FITC 0
#define GPT_SPARSE_VFE 1
#define GPT_SPARSE_DTC 2

/* Uploads the inducing inputs (after gpt_set_data; Z has the data's D columns) and drops any sparse fit. */
int gpt_sparse_set_inducing(gpt_ctx *ctx, const double *Z, const int32_t *nZ, int64_t M);

/* One evaluation.  The model as gpt_fit_terms takes it (same description, same order checks, applied to the training AND the
 * inducing orders); y: the targets with the mean function subtracted.  chunk_rows: training rows per pass, a multiple of 64; 0
 * picks what keeps the two chunk x (M padded) buffers within a fixed budget (512 MiB).  The chunks run in ascending order and every
 * sum has a fixed order: the same call gives the same bits.
 * parts_out (5 doubles, may be NULL): sum log Lambda_i, sum log (L_B)_mm, y^T Lambda^-1 y, c.c, sum (k_i - q_i) / s_i (0 unless vfe).
 * Status > 0: that leading minor of K_uu + jitter I or of B is not positive definite (gpt_last_error says which);
 * GPT_E_VALUE: a Lambda_i is not a positive finite number.  With the option "timing" set, gpt_last_timings afterwards returns
 * the milliseconds of [0] the K_fu builds, [1] the right-side solves, [2] the row passes, [3] the Grams, [4] both factorisations.
 * After a success L_u, L_B and c stay resident (nothing of size N does). */
int gpt_sparse_fit(gpt_ctx *ctx, int method, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                   const int *nparams, const int *nparams1, double noise_var, const double *y, const double *err_y, double jitter,
                   int64_t chunk_rows, double *ll_out, double *parts_out);

/* Predictions of the resident sparse fit; arguments and `want` as gpt_predict (cov_out is required for want == 2).  For want <= 1
 * the test points go through in the chunks of that fit: its chunk_rows argument (0: the same size rule), two chunk x (M padded)
 * buffers where the fit holds one -- what bounded the fit's memory bounds the prediction's.  want == 2 holds all Ms rows at once,
 * whatever chunk_rows was. */
int gpt_sparse_predict(gpt_ctx *ctx, const double *Xstar, const int32_t *nstar, int64_t Ms, int want, const double *noise_params,
                       const int32_t *noise_n, double *mean_out, double *std_out, double *cov_out);

/* c (M doubles) of the resident sparse fit: what the predictive mean is a dot product with. */
int gpt_sparse_get_c(gpt_ctx *ctx, double *c_out);

/* Device API: the tall-skinny Gram of the sparse fit on raw device pointers, on the context's stream.
 *   dG (mg x mg, row stride ldg; the 64 x 64 tiles on and below the diagonal) += dV^T dV,  dV (rows x mg, row stride ldv >= mg),
 * mg a multiple of 64, any rows >= 1.  The rows are split into nslices slices (0: chosen so that tiles x slices is about six times
 * the number of compute units), one workgroup per (tile, slice); the partial tiles are added in slice order (no atomics). */
int gpt_dev_sparse_gram(gpt_ctx *ctx, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices, double *dG, int64_t ldg);

/* Device API: the four other kernels of the sparse fit, one launch each, on raw device pointers and the context's stream.
 * gpt_dev_sparse_lambda: the per-row pass over a chunk dV (rows x ldv row-major, ldv > M; row i holds V_.i in its columns [0, M)).
 *   method: GPT_SPARSE_*.  q_i = sum_{m < M} V_mi^2, s_i = noise_var + d_err[i]^2, Lambda_i = d_kdiag[i] - q_i + s_i (fitc) or s_i;
 *   d_rowval[i] = log Lambda_i, d_rowval[ldr + i] = (d_kdiag[i] - q_i) / s_i (vfe, else 0); the columns [0, M) of row i are scaled by
 *   Lambda_i^-1/2 and column M is set to Lambda_i^-1/2 d_r[i]; the columns behind M are not touched.  A row whose Lambda_i is not a
 *   positive finite number sets *d_bad = 1 (the word is never cleared here), gets 0 in both row values and in its columns [0, M].
 *   rows <= ldr.
 * gpt_dev_sparse_rowsum: d_acc[0] += sum_i d_rowval[i], d_acc[1] += sum_i d_rowval[ldr + i], i < rows <= ldr; a fixed order.
 * gpt_dev_sparse_var: d_var[i] = d_kdiag[i] - sum_{m < M} dV[i][m]^2 + sum_{m < M} dW[i][m]^2 (both rows x ld row-major, M <= ld).
 * gpt_dev_sparse_assemble_b: dB (bp x bp, row stride bp > M, every element written) from dG (row stride ldg > M, lower triangle and
 *   row M read): rows < M hold I + G (the upper triangle zero), row M holds G[M][0..M) and `big` on the diagonal, the rows behind
 *   it a unit diagonal. */
int gpt_dev_sparse_lambda(gpt_ctx *ctx, double *dV, int64_t ldv, int64_t rows, int64_t M, int method, const double *d_kdiag,
                          const double *d_r, const double *d_err, double noise_var, double *d_rowval, int64_t ldr, int32_t *d_bad);
int gpt_dev_sparse_rowsum(gpt_ctx *ctx, const double *d_rowval, int64_t ldr, int64_t rows, double *d_acc);
int gpt_dev_sparse_var(gpt_ctx *ctx, const double *dV, const double *dW, int64_t ld, int64_t rows, int64_t M, const double *d_kdiag,
                       double *d_var);
int gpt_dev_sparse_assemble_b(gpt_ctx *ctx, const double *dG, int64_t ldg, int64_t M, double *dB, int64_t bp, double big);

/* nbatch evaluations of the sparse objective of the resident data and inducing inputs in ONE launch sequence (DESIGN.md section
 * 18.11): every kernel of gpt_sparse_fit's chain carries the batch in a grid dimension.  Every element has the first element's
 * kernel ids; params: nbatch x ptot (ptot = sum of nparams), noise_var: nbatch, y: nbatch x N (the mean function's parameters may
 * differ per element), err_y: N, shared.  method, jitter and chunk_rows as gpt_sparse_fit; the chunks are those gpt_sparse_fit
 * walks for the same chunk_rows, with one chunk x (M padded) buffer per element.
 * ll_out[b] and parts_out[5 b ...] (parts_out may be NULL) carry THE BITS gpt_sparse_fit returns for element b alone with the same
 * chunk_rows: they do not depend on nbatch or on the element's place in the batch.
 * An element that fails does not fail the call: info_out[b] is 0 or the leading minor that failed (1 ... M), which_out[b] names
 * the matrix -- 0 none, 1 K_uu + jitter I, 2 a Lambda_i is not a positive finite number (info 0), 3 B; ll_out[b] of such an element
 * is not meaningful; the other elements keep their bits.  An argument of one element that the parser refuses fails the whole call
 * with the parser's status.  GPT_E_STATE / GPT_E_NOTIMPL / GPT_E_ARG as gpt_sparse_fit, GPT_E_ARG for nbatch outside 1 ... 65535,
 * GPT_E_NOMEM where the batch's slots do not fit (the caller halves nbatch).
 * The batch lives in slots of its own (gpt_release_batch_scratch frees them): the resident single sparse fit and the dense factor
 * of the context survive the call. */
int gpt_sparse_fit_batch(gpt_ctx *ctx, int nbatch, int method, int nterms, const int *kernel_ids, const int *kernel_ids2,
                         const double *params, const int *nparams, const int *nparams1, const double *noise_var, const double *y,
                         const double *err_y, double jitter, int64_t chunk_rows, double *ll_out, double *parts_out, int32_t *info_out,
                         int32_t *which_out);

/* Device API: the batched forms of the four kernel groups, element b of nbatch on dV + b vstride (vstride >= rows ldv), d_kdiag + b
 * kstride, d_r + b rstride, d_noise_var[b] (a device array), d_rowval + b rvstride (rvstride >= 2 ldr), d_bad[b], d_acc + b astride,
 * dG + b gstride, dB + b bstride; d_err is shared.  Per element the arithmetic, the slice partition (that of gpt_dev_sparse_gram for
 * the same rows, mg and nslices) and every summation order are those of the single launchers above: the same bits. */
int gpt_dev_sparse_lambda_batch(gpt_ctx *ctx, int64_t nbatch, double *dV, int64_t ldv, int64_t vstride, int64_t rows, int64_t M, int method,
                                const double *d_kdiag, int64_t kstride, const double *d_r, int64_t rstride, const double *d_err,
                                const double *d_noise_var, double *d_rowval, int64_t ldr, int64_t rvstride, int32_t *d_bad);
int gpt_dev_sparse_rowsum_batch(gpt_ctx *ctx, int64_t nbatch, const double *d_rowval, int64_t ldr, int64_t rvstride, int64_t rows,
                                double *d_acc, int64_t astride);
int gpt_dev_sparse_gram_batch(gpt_ctx *ctx, int64_t nbatch, const double *dV, int64_t ldv, int64_t vstride, int64_t rows, int64_t mg,
                              int nslices, double *dG, int64_t ldg, int64_t gstride);
int gpt_dev_sparse_assemble_b_batch(gpt_ctx *ctx, int64_t nbatch, const double *dG, int64_t ldg, int64_t gstride, int64_t M, double *dB,
                                    int64_t bp, int64_t bstride, double big);

/* The gradient of the resident sparse fit's objective by per-pair central differences, the stencil
 * arguments those of gpt_ll_grad_diff: entry h < nh names term term_idx[h] of the fitted model with that term's complete parameter
 * vector at the two stencil points (params_a / params_b, entry after entry) and denom[h] = theta_b - theta_a; every stencil point goes
 * through the order checks of the fit as a one-term model.  y, err_y: as given to gpt_sparse_fit (the fit keeps no copy).
 *   t = L_B^-T c,  beta = L_u^-T t,  alpha_i = (y_i - v_i.t) / Lambda_i  (alpha = (Q_ff + Lambda)^-1 y),  w_i = L_B^-1 v_i
 *   W_ii = alpha_i^2 - 1 / Lambda_i + |w_i|^2 / Lambda_i^2,   e_i = W_ii (fitc), -1 / s_i (vfe), 0 (dtc)
 *   A_fu[i,:] = alpha_i beta^T - (1 / Lambda_i) v_i^T B^-1 L_u^-1 - e_i v_i^T L_u^-1
 *   A_uu = -1/2 (beta beta^T - L_u^-T (I - B^-1 + V diag(e) V^T) L_u^-1)
 *   d ll = sum A_uu dK_uu + sum A_fu dK_fu + 1/2 sum_i e_i dk_i + sum_i g_i ds_i,   g_i = W_ii / 2 (+ (k_i - q_i) / (2 s_i^2), vfe)
 * out[h], h < nh: the entry of the kernel parameter; out[nh] = sum_i g_i, the derivative with respect to noise_var.  alpha_out (N
 * doubles, may be NULL): alpha, what a mean function's parameters take their derivative against.  The jitter is a constant.
 * One more pass over the training rows in chunks -- the fit's chunk_rows, or the size rule for FOUR chunk x (M padded) buffers -- in
 * ascending order with fixed summation orders: the same call gives the same bits.  L_u, L_B, c and the dense factor of the context
 * are read, never written.  GPT_E_STATE without a sparse fit that succeeded, GPT_E_NOTIMPL with gpt_set_T or warp layers,
 * GPT_E_ARG for a zero or infinite denom, GPT_E_VALUE if a Lambda_i is not a positive finite number. */
int gpt_sparse_grad_diff(gpt_ctx *ctx, int nh, const int *term_idx, const double *params_a, const double *params_b, const double *denom,
                         const double *y, const double *err_y, double *out, double *alpha_out);

/* Device API: the kernels of that gradient alone, on raw device pointers and the context's stream.
 * gpt_dev_sparse_grad_rows: the per-row pass.  dV, dW (rows x ld row-major, M <= ld): row i holds v_i and w_i in its columns [0, M);
 *   d_t: M doubles.  Per row q_i = |v_i|^2, Lambda_i as gpt_dev_sparse_lambda, alpha_i, W_ii, e_i, g_i as above (d_kdiag is not read
 *   for dtc); written: d_alpha[i], d_e[i], d_gval[i] = g_i and d_gval[ldr + i] = 0 (the layout gpt_dev_sparse_rowsum adds up), and
 *   the scaled copies dS1[i] = v_i / Lambda_i, dS2[i] = e_i v_i with zeros in the columns [M, ld).  A row whose Lambda_i is not a
 *   positive finite number sets *d_bad = 1 and gets zeros throughout.  rows <= ldr.
 * gpt_dev_sparse_gram2: gpt_dev_sparse_gram with two operands, dG += dA^T dV (both rows x ldv): the signed-weight Gram V diag(e) V^T
 *   from dA = dS2.  The same tiles, slices and slice-ordered sum.
 * gpt_dev_sparse_grad_pairs: the rectangular pair pass for ONE term, kernel_id (* kernel_id2 where >= 0) of num_dim D with nparams
 *   parameters (nparams1 of them the first factor's): out[h] = sum_im dA[i][m] (k_b - k_a)(x_i, z_m) + 1/2 sum_i d_e[i] (k_b - k_a)(x_i,
 *   x_i) with k_a / k_b the term at params_a / params_b (host, nh x nparams each), h < nh (GPT_GRAD_MAXH per launch); not divided by
 *   a step.  dX (rows x D) and dZ (M x D) with orders dnx / dnz, max_order the largest order sum among them; dA rows x lda, M <= lda;
 *   d_e NULL: no diagonal part.  Partial sums are added in index order: the same call gives the same bits. */
int gpt_dev_sparse_grad_rows(gpt_ctx *ctx, const double *dV, const double *dW, int64_t ld, int64_t rows, int64_t M, int method,
                             const double *d_kdiag, const double *d_r, const double *d_err, double noise_var, const double *d_t,
                             double *d_alpha, double *d_e, double *d_gval, int64_t ldr, double *dS1, double *dS2, int32_t *d_bad);
int gpt_dev_sparse_gram2(gpt_ctx *ctx, const double *dA, const double *dV, int64_t ldv, int64_t rows, int64_t mg, int nslices, double *dG,
                         int64_t ldg);
int gpt_dev_sparse_grad_pairs(gpt_ctx *ctx, int kernel_id, int kernel_id2, int D, int max_order, int nh, const double *params_a,
                              const double *params_b, int nparams, int nparams1, const double *dX, const int32_t *dnx, int64_t rows,
                              const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda, const double *d_e,
                              double *out);

/* gpt_sparse_grad_diff and, from the same pass, the gradient with respect to the inducing inputs.  The
 * derivative of a covariance entry with respect to coordinate d of z_m is the pair function with z_m's derivative order raised by one
 * in dimension d, so with the adjoints above
 *   dz_out[m][d] = sum_i A_fu[i,m] k(x_i, z_m; n_i, n_m + e_d) + 2 sum_{m' != m} A_uu[m',m] k(z_m', z_m; n_m', n_m + e_d)
 * summed over the model's terms at the fitted parameters: M x D doubles, row-major, host; nothing is divided by a step (the pair
 * m' = m is left out: K_uu[m][m] does not depend on z_m).  out and alpha_out are gpt_sparse_grad_diff's, bit for bit; nh = 0 gives
 * out[0] = sum_i g_i and dz_out.  The pass meets the orders n_Z + e_d: the fitted model is held to the order rules of the fit at
 * the raised orders before anything is launched -- n_Z = 0 works for every kernel; derivative rows among Z are refused for a
 * Matern52 factor (GPT_E_VALUE) and, in its coordinate, for a Gibbs factor (GPT_E_NOTIMPL); the other statuses are
 * gpt_sparse_grad_diff's.  Fixed summation orders, no floating-point atomics: the same call gives the same bits.  A non-finite
 * entry of dz_out is returned as it is. */
int gpt_sparse_grad_z(gpt_ctx *ctx, int nh, const int *term_idx, const double *params_a, const double *params_b, const double *denom,
                      const double *y, const double *err_y, double *out, double *alpha_out, double *dz_out);

/* Device API: the pair pass of gpt_sparse_grad_z alone for ONE term, kernel_id (* kernel_id2 where >= 0) of num_dim D at `params`
 * (host; nparams of them, nparams1 the first factor's): out[m][d] = sum_i dA[i][m] k(x_i, z_m; n_i, n_m + e_d), M x D doubles on the
 * host, written, not accumulated.  dX (rows x D) and dZ (M x D) with orders dnx / dnz; max_order: the largest order sum of a point
 * of the pass, the raised n_Z + e_d included; dA rows x lda, M <= lda; skip_diag != 0: without the pairs i == m (X := Z).  Row
 * tiles of 64 are added in index order: the same call gives the same bits. */
int gpt_dev_sparse_grad_dz_pairs(gpt_ctx *ctx, int kernel_id, int kernel_id2, int D, int max_order, const double *params, int nparams,
                                 int nparams1, const double *dX, const int32_t *dnx, int64_t rows, const double *dZ, const int32_t *dnz,
                                 int64_t M, const double *dA, int64_t lda, int skip_diag, double *out);

/* Greedy conditional-variance choice of M inducing inputs among rows of the resident data: the partial
 * pivoted Cholesky of K_ff.  The model arguments are gpt_sparse_fit's, parsed against the training orders.  cand: ncand row indices,
 * strictly ascending, every one a row whose derivative orders are all zero; NULL: every such row of the data (ncand is ignored).
 *   d_i = k(x_i, x_i);  for j = 0 .. M-1:  p_j = the unselected candidate with the largest d_i (equal as doubles: the lowest row),
 *   dmax_j = d_{p_j};  stop (count = j) if j > 0 and dmax_j <= tol * dmax_0, or if dmax_j is not a positive finite number;
 *   l_i = (k(x_i, x_{p_j}) - sum_{t<j} L[i,t] L[p_j,t]) / sqrt(dmax_j),  L[i,j] = l_i,  d_i -= l_i^2  for EVERY candidate i;
 *   trace_{j+1} = sum over the unselected candidates of max(d_i, 0)   (trace_0 = sum of the initial d_i).
 * A selected row is excluded by its mark, never by its residual.  For a stationary kernel step 0 is a complete tie: the first pivot is
 * the lowest candidate.  idx_out (M), dmax_out (M), trace_out (M + 1), *count_out: host; the entries at and past count (trace: past
 * count) are -1 / NaN.  trace_count is tr(K_ff - K_fu K_uu^-1 K_uf) over the candidates, the quantity the VFE objective penalises.
 * The whole loop is enqueued on the context's stream without a host synchronisation between the steps -- per step one pick launch,
 * the builder's launches for the column k(x_p, .) (the pair (x_p, x_i), pivot first: the builder's bits) and one update launch -- and
 * read back once.  Device memory: the factor, (ncand rounded up to 64) x M doubles, column-major, in a slot of its own; neither the
 * dense factor nor the resident sparse state is touched.  Fixed summation orders: the same call gives the same bits.
 * GPT_E_STATE without gpt_set_data; GPT_E_NOTIMPL with gpt_set_T or warp layers; GPT_E_ARG for M < 1, M > ncand, M > 65000, tol < 0,
 * a candidate list that is not strictly ascending or out of range, or a candidate with a non-zero order; GPT_E_NOMEM (the byte
 * count in the message); GPT_E_VALUE if dmax_0 is not a positive finite number. */
int gpt_sparse_select_inducing(gpt_ctx *ctx, int nterms, const int *kernel_ids, const int *kernel_ids2, const double *params,
                               const int *nparams, const int *nparams1, const int32_t *cand, int64_t ncand, int64_t M, double tol,
                               int32_t *idx_out, double *dmax_out, double *trace_out, int64_t *count_out);

/* Device API: the two kernels of that loop alone, on raw device pointers and the context's stream (csrc/kgreedy.hip).
 * Shared state: d_scal, two doubles ([GPT_GREEDY_S_DMAX] the current pivot's dmax, [GPT_GREEDY_S_DMAX0] dmax_0); d_words, four int32
 * ([GPT_GREEDY_W_STOP] raised by the stop rule: both kernels then return at once, [GPT_GREEDY_W_COUNT] pivots chosen so far,
 * [GPT_GREEDY_W_PIVOT] the current pivot's row, [GPT_GREEDY_W_BAD] dmax_0 was not a positive finite number); partials, one per
 * GPT_GREEDY_ROWS_PER_PART rows, nparts = gpt_dev_greedy_parts(rows): d_part[b] the largest residual among workgroup b's unselected
 * rows (-inf: none), d_pidx[b] the lowest row at that value (INT32_MAX: none), d_part[nparts + b] the sum of max(residual, 0) there.
 * gpt_dev_greedy_update: step j for rows < rows <= ld of the column-major factor dL (columns [0, j) read): s_i = sum_{t<j}
 *   dL[i + t ld] d_prow[t]; d_col[i] = l_i = (d_col[i] - s_i) / sqrt(d_scal[0]) -- a division; d_resid[i] -= l_i^2; the partials
 *   over the rows with d_mark[i] == 0.  d_col is column j wherever the caller keeps it (dL + j ld in the library).
 * gpt_dev_greedy_pick: reduces nparts partials, writes d_trace[j]; with j < M applies the stop rule or writes d_idx[j] = d_cand[p]
 *   (d_cand NULL: p), d_dmax[j], d_mark[p] = 1, the scalars and words, d_xp[0 .. D) = dX[p], d_prow[t] = dL[p + t ld], t < j. */
#define GPT_GREEDY_ROWS_PER_PART 256
#define GPT_GREEDY_S_DMAX 0
#define GPT_GREEDY_S_DMAX0 1
#define GPT_GREEDY_W_STOP 0
#define GPT_GREEDY_W_COUNT 1
#define GPT_GREEDY_W_PIVOT 2
#define GPT_GREEDY_W_BAD 3
int64_t gpt_dev_greedy_parts(int64_t rows);
int gpt_dev_greedy_update(gpt_ctx *ctx, const double *dL, int64_t ld, int64_t rows, int64_t j, double *d_col, double *d_resid,
                          const int32_t *d_mark, const double *d_prow, const double *d_scal, const int32_t *d_words, double *d_part,
                          int32_t *d_pidx);
int gpt_dev_greedy_pick(gpt_ctx *ctx, int64_t j, int64_t M, double tol, const double *d_part, const int32_t *d_pidx, int64_t nparts,
                        const int32_t *d_cand, const double *dX, int D, const double *dL, int64_t ld, int32_t *d_mark, double *d_scal,
                        int32_t *d_words, int32_t *d_idx, double *d_dmax, double *d_trace, double *d_xp, double *d_prow);

/* ---- compiled schedules of the partitioned engines (round 6) ------------------------------------------------------------
 * The one-process-per-GPU block-cyclic Cholesky of gptools_amd/dist.py issues ~1000 operations per rank and evaluation; which
 * ones, on which buffers, in which order is static per (N, nb, world, rank).  The Python layer records its step loop once as an
 * op list -- GPT_PLAN_W = 20 int64 per op: [opcode, queue, a0 .. a17], doubles as their bit patterns, queues 0 = main, 1 = panel,
 * 2 = recv (the contexts given here, in this order), 3 + c = the stream of the plan's communication channel c -- and every
 * evaluation is then one gpt_plan_run: a C loop over the list, RCCL (dlopen'ed librccl) called directly for the panel exchanges.
 * Opcodes (csrc/api_plan.inc):
 *   0 record event a0 | 1 wait event a0 | 2 K block (r0, r1, c0, c1, out, ld) | 3 pad block (ptr, lda, c0, nb, N, NP, y, big) |
 *   4 copy2d (rows, cols, src, lds, dst, ldd) | 5 potrf_panel (m, nb, A, lda, invd, info, info_base) | 6 trinv (nb, L, ldl, invd, W, ldw) |
 *   7 gemm_nt (m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri) | 8 gemm_nt_stair (m, nseg, seg_cols, k, alpha, A, lda, B, ldb,
 *   b_stride, row_step, beta, C, ldc) | 9 panel_scalars (buf, ld, w, zrow, red) | 10 broadcast (buf, count, root) |
 *   11 scatter (buf, count per rank, root) | 12 all-gather in place (buf, count per rank) | 13 K rectangle (Xi, ni, r0, r1, c0, c1,
 *   out, ld: rows from the caller's own row table, no diagonal terms) | 14 row_sumsq (row, count, out) | 15 gemm_nt_gridstair (m,
 *   nseg, seg_cols, k, alpha, A, lda, B, ldb, off, num, den, base, beta, C, ldc).  Collectives (10-12) sit on a channel queue,
 *   kernels on a context queue, events on either.
 * dX (N x D float64), dn (N x D int32), d_err (N float64) are the device arrays the K-block ops read; the per-evaluation inputs
 * are arguments of gpt_plan_run.  A CHANNEL is one communicator + one high-priority stream (up to GPT_PLAN_CHANNELS; the 1-D
 * engine has one over all ranks, the 2-D engine five: process row x 2, process column x 2, the whole grid): gpt_plan_set_channel
 * is collective over the channel's ranks (ncclCommInitRank; the 128-byte id comes from gpt_plan_unique_id on the channel's rank 0
 * and travels by whatever means the caller has; every rank sets its channels in the same order); root / rank are positions in
 * that communicator.  gpt_plan_set_comm = channel 0.  The ops of a channel without a communicator are skipped (single rank).
 * The caller keeps the buffers alive and synchronises the contexts' streams itself.  (Environment GPT_PLAN_PROFILE=1: gpt_plan_run prints
 * its host time per opcode to stderr.) */
#define GPT_PLAN_W 20
#define GPT_PLAN_CHANNELS 8
typedef struct gpt_plan gpt_plan;
int gpt_plan_unique_id(void *out128);
int gpt_plan_create(int nctx, gpt_ctx **ctxs, const int64_t *ops, int64_t nops, int nevents, const void *dX, const void *dn, int D,
                    const void *d_err, gpt_plan **out);
int gpt_plan_set_comm(gpt_plan *plan, int nranks, int rank, const void *unique_id128);
int gpt_plan_set_channel(gpt_plan *plan, int channel, int nranks, int rank, const void *unique_id128);
int gpt_plan_run(gpt_plan *plan, int kernel_id, const double *params, int nparams, double noise_var, double diag_add);
double gpt_plan_last_enqueue_ms(gpt_plan *plan);          /* host time gpt_plan_run spent enqueueing, last call */
int gpt_plan_destroy(gpt_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* GPT_HIP_H_ */
