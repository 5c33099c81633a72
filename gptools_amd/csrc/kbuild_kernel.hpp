// kbuild_kernel.hpp -- the fused covariance-builder kernel (see kbuild.hip), shared by the single-matrix launcher
// (kbuild.hip) and the batched one (kbuild_batch.hip: gpt_fit_batch, one matrix per blockIdx.z); below the kernels, the host
// side all the launchers share: kernel-id and num_dim dispatch, the tile grid, the one launch of kbuild_kernel.
#pragma once
#include "kpair.hpp"

#define KB_THREADS 256
#define KB_CPT 1                        // columns per lane.  2 (16-byte stores) lifts the pure write pattern from 4.6 to
                                        // 5.4 TB/s but the pair arithmetic then runs with half the waves: SE 4.65 -> 4.44
                                        // TB/s, Matern-5/2 with derivative rows 0.18 -> 0.21 ms at N=8192 (measured)
#define KB_COLS (KB_THREADS * KB_CPT)
#define KB_ROWS 32
#define KB_RATIO (KB_COLS / KB_ROWS)

// the product instantiations (ProductKids below): k1 * k2 in the form the id names
constexpr bool is_product_kid(int kid)
{
    return kid == GPT_KERNEL_PRODUCT || kid == GPT_KID_PRODUCT_GM || kid == GPT_KID_PRODUCT_GB || kid == GPT_KID_PRODUCT_PER;
}

// The term KID at one pair: a native kernel, or the product k1 * k2 in the form KID names (k2 is read for a product only).  The pair
// passes of the gradients (kgrad.hip, kgrad_rect.hip) evaluate their terms through this.
template <int KID, int D>
__device__ __forceinline__ double term_pair(const KParams &k1, const KParams *__restrict__ k2, const double *xi, const double *xj,
                                            const int *ni, const int *nj)
{
    if constexpr (KID == GPT_KERNEL_PRODUCT) return prod_pair<D>(k1, *k2, xi, xj, ni, nj);
    else if constexpr (KID == GPT_KID_PRODUCT_GM) return prod_pair<D, true>(k1, *k2, xi, xj, ni, nj);
    else if constexpr (KID == GPT_KID_PRODUCT_GB) return prod_pair<D, true, true>(k1, *k2, xi, xj, ni, nj);
    else if constexpr (KID == GPT_KID_PRODUCT_PER) return prod_pair<D, true, true, true>(k1, *k2, xi, xj, ni, nj);
    else return any_pair<KID, D>(k1, xi, xj, ni, nj);
}

// BATCH: element blockIdx.z of a batch of independent matrices over the same points -- its hyperparameters kps[z], its
// noise variance nvs[z], its matrix K + z * bstride (gpt_fit_batch); `kp_one` / `noise_one` are unused then.
// WARP (gpt_set_warp): Xi / Xj hold WARPED points and Si / Sj the points' chain-rule slopes (warp.hpp: exactly 1.0 for a value
// point); every pair of a tile that carries a derivative order is multiplied by Si[i] Sj[j] before it is added to earlier terms
// and before the diagonal epilogue.  PLAIN tiles have S = 1 throughout and skip the factor.  A template flag, not a run-time
// test: the instantiations without a warp are the code they were.
template <int KID, int D, bool BATCH, bool WARP = false>
__global__ __launch_bounds__(KB_THREADS) void kbuild_kernel(
    KParams kp_one, const double *__restrict__ Xi, const int32_t *__restrict__ ni, int64_t M,
    const double *__restrict__ Xj, const int32_t *__restrict__ nj, int64_t P,
    int lower_only, int64_t i0, int64_t j0, const double *__restrict__ err_y, double noise_one,
    double diag_add, double *__restrict__ K, int64_t ldk, int accumulate, const KParams *__restrict__ kps,
    const double *__restrict__ nvs, int64_t bstride, KParams kp_two_one, const KParams *__restrict__ kps2,
    const double *__restrict__ Si = nullptr, const double *__restrict__ Sj = nullptr, int64_t xstride = 0, int64_t sstride = 0)
{
    if constexpr (BATCH && WARP) {       // a warped batch: element z has its own warped points and slope factors (gpt_set_warp_batch)
        Xi += (int64_t)blockIdx.z * xstride;
        Xj += (int64_t)blockIdx.z * xstride;
        Si += (int64_t)blockIdx.z * sstride;
        Sj += (int64_t)blockIdx.z * sstride;
    }
    const KParams &kp = BATCH ? kps[blockIdx.z] : kp_one;
    const KParams &kp_two = (BATCH && kps2 != nullptr) ? kps2[blockIdx.z] : kp_two_one;      // second factor of a product term
    const double noise_var = BATCH ? nvs[blockIdx.z] : noise_one;
    if (BATCH) K += (int64_t)blockIdx.z * bstride;
    int64_t rt, ct;
    if (lower_only == 2) {
        // Triangular launch (i0 == j0, M == P): only the tiles that touch the lower triangle exist.  Row tile rt
        // (KB_ROWS rows) needs column tiles 0 .. rt / R (R = KB_COLS / KB_ROWS); groups of R row tiles share a count,
        // so with g = rt / R the tiles before group g number R g (g + 1) / 2 and the linear index inverts in closed
        // form.
        constexpr int64_t R = KB_RATIO;
        const int64_t b = blockIdx.x;
        int64_t g = (int64_t)((sqrt(1.0 + 8.0 * (double)b / (double)R) - 1.0) * 0.5);
        while (g > 0 && R * g * (g + 1) / 2 > b) g--;
        while (R * (g + 1) * (g + 2) / 2 <= b) g++;
        const int64_t rem = b - R * g * (g + 1) / 2;
        rt = R * g + rem / (g + 1);
        ct = rem % (g + 1);
        if (rt * KB_ROWS >= M) return;
    } else {
        rt = blockIdx.y;
        ct = blockIdx.x;
    }
    const int64_t rbase = rt * KB_ROWS;
    const int64_t cbase = ct * KB_COLS;
    if (lower_only && (cbase + j0 > rbase + KB_ROWS - 1 + i0)) return;     // tile strictly above the diagonal
    const int64_t jfirst = cbase + (int64_t)threadIdx.x * KB_CPT;
    double xj[KB_CPT][D];
    int njr[KB_CPT][D];
#pragma unroll
    for (int c = 0; c < KB_CPT; c++) {
        const int64_t jc = (jfirst + c < P) ? jfirst + c : (P - 1);
#pragma unroll
        for (int d = 0; d < D; d++) {
            xj[c][d] = Xj[jc * D + d];
            njr[c][d] = nj[jc * D + d];
        }
    }
    double sj[KB_CPT];
    if constexpr (WARP) {
#pragma unroll
        for (int c = 0; c < KB_CPT; c++) sj[c] = Sj[(jfirst + c < P) ? jfirst + c : (P - 1)];
    }
    // both columns in range and the pair 16-byte aligned -> one dwordx4 store per row
    const bool vec = (jfirst + KB_CPT <= P) && ((ldk & 1) == 0) && ((((uintptr_t)K >> 3) + (uint64_t)jfirst) & 1) == 0;
    const int64_t rend = (rbase + KB_ROWS < M) ? rbase + KB_ROWS : M;
    // PLAIN tiles (round 4).  Most of a real Gram matrix pairs value rows with value columns: if none of the
    // tile's rows and none of this wave's columns carries a derivative order, the row loop needs no class logic at all -- no
    // derivative-order loads, no index selection (the ~25 scalar and ~6 vector instructions per row the general loop spends on
    // choosing among four formulas).  The test is once per tile and wave: the orders of the rows in one or two vector loads
    // and a ballot.  C3 (last quarter derivative rows): 56 % of the lower triangle's pairs.
    if constexpr (gibbs_kid(KID) && KB_CPT == 1) {
        static_assert(D == 1, "the Gibbs kernels are one-dimensional");
        // The warps are hoisted out of the row loop (kpair.hpp, GibbsPt): this lane's column point once, and the tile's
        // 32 row points once per wave -- lane q (and q + 32) forms row rbase + q, the row loop reads it back with
        // v_readlane into scalar registers.  Per pair: one v_rsq_f64 + Newton step, one exponential, a few FMAs.
        const GibbsPt cp = gibbs_point<KID>(kp, xj[0][0]);
        const int lane = (int)(threadIdx.x & 63);
        const int64_t ir = (rbase + (lane & 31) < M) ? rbase + (lane & 31) : M - 1;
        const GibbsPt rp = gibbs_point<KID>(kp, Xi[ir]);
        const double s2 = kp.sigma * kp.sigma;
        const bool col_d = __builtin_amdgcn_ballot_w64(njr[0][0] != 0) != 0;
        bool row_d = false;
        {
            int rn = 0;
            for (int64_t q = rbase + (threadIdx.x & 63); q < rend; q += 64) rn |= ni[q];
            row_d = __builtin_amdgcn_ballot_w64(rn != 0) != 0;
        }
        if (!col_d && !row_d) {
            // PLAIN tile: value class only
            for (int64_t i = rbase; i < rend; i++) {
                const int q = (int)(i - rbase);
                const double xi = Xi[i];
                const double a = readlane_f64(rp.l, q), ra = readlane_f64(rp.r2, q);
                const double rb = gibbs_col_root(a, cp.rp, cp.rn);
                double v = gibbs_core(s2, xi, a, 0.0, 0.0, ra, xj[0][0], cp.l, 0.0, 0.0, rb, 0, 0, false);
                if (accumulate && jfirst < P) v += K[i * ldk + jfirst];
                if (err_y != nullptr && (i + i0 == jfirst + j0)) {
                    const double e = err_y[i + i0];
                    v = ((v + noise_var) + e * e) + diag_add;
                }
                if (jfirst < P) K[i * ldk + jfirst] = v;
            }
            return;
        }
        for (int64_t i = rbase; i < rend; i++) {
            const int q = (int)(i - rbase);
            const double xi = Xi[i];
            const int nir = ni[i];
            const double a = readlane_f64(rp.l, q), ra = readlane_f64(rp.r2, q);
            const double A = readlane_f64(rp.A, q), ha = gibbs_h_other<KID>(readlane_f64(rp.h, q), cp.l);
            const double rb = gibbs_col_root(a, cp.rp, cp.rn);
            double v = gibbs_core(s2, xi, a, A, ha, ra, xj[0][0], cp.l, cp.A, gibbs_h_other<KID>(cp.h, a), rb, nir, njr[0][0],
                                  col_d || nir != 0);
            if constexpr (WARP) v *= Si[i] * sj[0];
            if (accumulate && jfirst < P) v += K[i * ldk + jfirst];
            if (err_y != nullptr && (i + i0 == jfirst + j0)) {
                const double e = err_y[i + i0];
                v = ((v + noise_var) + e * e) + diag_add;
            }
            if (jfirst < P) K[i * ldk + jfirst] = v;
        }
        return;
    }
    if constexpr ((KID == GPT_KERNEL_SE || KID == GPT_KERNEL_M52) && KB_CPT == 1) {
        int cn = 0;
#pragma unroll
        for (int d = 0; d < D; d++) cn |= njr[0][d];
        bool plain = kp.hyper_deriv < 0 && __builtin_amdgcn_ballot_w64(cn != 0) == 0;
        if (plain) {
            int rn = 0;
            const int64_t cnt = (rend - rbase) * D;
            for (int64_t q = threadIdx.x & 63; q < cnt; q += 64) rn |= ni[rbase * D + q];
            plain = __builtin_amdgcn_ballot_w64(rn != 0) == 0;
        }
        if (plain) {
            for (int64_t i = rbase; i < rend; i++) {
                double xi[D];
#pragma unroll
                for (int d = 0; d < D; d++) xi[d] = Xi[i * D + d];          // wave-uniform addresses -> scalar loads
                double v = plain_pair<KID, D>(kp, xi, xj[0]);
                if (accumulate && jfirst < P) v += K[i * ldk + jfirst];
                if (err_y != nullptr && (i + i0 == jfirst + j0)) {
                    const double e = err_y[i + i0];
                    v = ((v + noise_var) + e * e) + diag_add;
                }
#ifdef KB_DEBUG_NOCOMPUTE
                v = (double)i;
#endif
#ifdef KB_DEBUG_NOSTORE
                if (v != 12345.678) continue;
#endif
                if (jfirst < P) K[i * ldk + jfirst] = v;
            }
            return;
        }
    }
    for (int64_t i = rbase; i < rend; i++) {
        double xi[D];
        int nir[D];
#pragma unroll
        for (int d = 0; d < D; d++) {          // wave-uniform addresses -> scalar loads
            xi[d] = Xi[i * D + d];
            nir[d] = ni[i * D + d];
        }
        double v[KB_CPT];
#pragma unroll
        for (int c = 0; c < KB_CPT; c++) {
            if constexpr (KID == GPT_KERNEL_PRODUCT) v[c] = prod_pair<D>(kp, kp_two, xi, xj[c], nir, njr[c]);
            else if constexpr (KID == GPT_KID_PRODUCT_GM) v[c] = prod_pair<D, true>(kp, kp_two, xi, xj[c], nir, njr[c]);
            else if constexpr (KID == GPT_KID_PRODUCT_GB) v[c] = prod_pair<D, true, true>(kp, kp_two, xi, xj[c], nir, njr[c]);
            else if constexpr (KID == GPT_KID_PRODUCT_PER) v[c] = prod_pair<D, true, true, true>(kp, kp_two, xi, xj[c], nir, njr[c]);
            else v[c] = any_pair<KID, D>(kp, xi, xj[c], nir, njr[c]);
            if constexpr (WARP) v[c] *= Si[i] * sj[c];
            // SumKernel (ref: gptools/kernel/core.py:549-584): later terms add to what the earlier passes stored
            if (accumulate && jfirst + c < P) v[c] += K[i * ldk + jfirst + c];
            if (err_y != nullptr && (i + i0 == jfirst + c + j0)) {
                const double e = err_y[i + i0];
                v[c] = ((v[c] + noise_var) + e * e) + diag_add;
            }
        }
#ifdef KB_DEBUG_NOCOMPUTE           // (measurement builds, scratch/kb_variants.sh: the store pattern alone / the arithmetic alone.
        v[0] = (double)i;           //  Round 3, N = 8192 lower triangle: stores alone 5.6 TB/s; arithmetic alone = the product's time, for
#endif                             //  SE as for Matern-5/2: the builder is bound by its ~57 VALU + ~45 SALU instructions per row and wave)
#ifdef KB_DEBUG_NOSTORE
        if (v[0] != 12345.678) continue;
#endif
        if (KB_CPT == 2 && vec) {
            f64x2 w = {v[0], v[KB_CPT - 1]};
            *reinterpret_cast<f64x2 *>(K + i * ldk + jfirst) = w;
        } else {
#pragma unroll
            for (int c = 0; c < KB_CPT; c++)
                if (jfirst + c < P) K[i * ldk + jfirst + c] = v[c];
        }
    }
}

template <int KID, int D>
__global__ __launch_bounds__(256) void kpairs_kernel(KParams kp, const double *__restrict__ Xi,
                                                     const double *__restrict__ Xj,
                                                     const int32_t *__restrict__ ni,
                                                     const int32_t *__restrict__ nj, int64_t M,
                                                     double *__restrict__ out, int accumulate, KParams kp_two)
{
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double xi[D], xj[D];
    int nir[D], njr[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        xi[d] = Xi[m * D + d];
        xj[d] = Xj[m * D + d];
        nir[d] = ni[m * D + d];
        njr[d] = nj[m * D + d];
    }
    double v;
    if constexpr (KID == GPT_KERNEL_PRODUCT) v = prod_pair<D>(kp, kp_two, xi, xj, nir, njr);
    else if constexpr (KID == GPT_KID_PRODUCT_GM) v = prod_pair<D, true>(kp, kp_two, xi, xj, nir, njr);
    else if constexpr (KID == GPT_KID_PRODUCT_GB) v = prod_pair<D, true, true>(kp, kp_two, xi, xj, nir, njr);
    else if constexpr (KID == GPT_KID_PRODUCT_PER) v = prod_pair<D, true, true, true>(kp, kp_two, xi, xj, nir, njr);
    else v = any_pair<KID, D>(kp, xi, xj, nir, njr);
    out[m] = accumulate ? out[m] + v : v;
}

// ================================================================================================
// Host side: from the run-time (kernel_id, num_dim) to ONE instantiation of the templates above.  Every launcher of kbuild.hip,
// kbuild_prod.hip and kbuild_batch.hip goes through dispatch_kid and dispatch_dim; a new kernel id is one entry of FitKids.
// ================================================================================================
#include <type_traits>
#include <utility>

// the ids a launcher accepts, as a type
template <int... KIDS>
struct KidList {
    template <int... MORE>
    using plus = KidList<KIDS..., MORE...>;
};
// the kernels a model term can be (native_fit_kernel, api_kparams.inc): what the batched builders take
using FitKids = KidList<GPT_KERNEL_SE, GPT_KERNEL_M52, GPT_KERNEL_RQ, GPT_KERNEL_MATERN, GPT_KERNEL_GIBBS_TANH, GPT_KERNEL_GIBBS_DTANH,
                        GPT_KERNEL_GIBBS_CUBIC, GPT_KERNEL_GIBBS_QUINTIC, GPT_KERNEL_GIBBS_EXPGAUSS, GPT_KERNEL_GIBBS_BSPLINE, GPT_KERNEL_GIBBS_GP,
                        GPT_KERNEL_PERIODIC, GPT_KERNEL_SPECTRAL>;
// ... and the noise kernels: the single-matrix builder and the pair list
using AllKids = FitKids::plus<GPT_KERNEL_DIAGNOISE, GPT_KERNEL_ZERO>;
// the builders' product instantiations (product_kid chooses)
using ProductKids = KidList<GPT_KERNEL_PRODUCT, GPT_KID_PRODUCT_GM, GPT_KID_PRODUCT_GB, GPT_KID_PRODUCT_PER>;

// The product of the factors id1 * id2 at num_dim D: GPT_KID_PRODUCT_GM carries the bucket / exp-Gauss Gibbs branches and exists
// at num_dim 1 only.  The single-matrix kernels take it only when a factor needs those branches (GPT_KERNEL_PRODUCT at num_dim 1
// stays the code it was, for the products of the older kernels); the batched ones, whose factor ids only the device sees, take it
// for every 1-D product.  GPT_KID_PRODUCT_GB adds the B-spline and nested-GP branches and is taken, single-matrix or batched, only when a factor
// is one of those two (gibbs_gb_kid; batched: the caller says so, GPT_GFORM_GB).  Why: common.hpp, at GPT_KID_PRODUCT_GM.
// At num_dim 2 .. GPT_GIBBS_ON_DIM_MAX_D a Gibbs factor acts on ONE coordinate (GPT_KERNEL_ON_DIM; make_kparams admits no other
// Gibbs factor there): GPT_KID_PRODUCT_GM, the tanh warps included, or GPT_KID_PRODUCT_GB with a B-spline or nested GP -- instantiations of their
// own, so GPT_KERNEL_PRODUCT at those num_dim stays the code it was for every product without a Gibbs factor.
// gform: the GPT_GFORM_* bits of the factors (gibbs_form_of; batched: of the whole model, ModelKernel::gibbs_form());
// gibbs_more: a factor is a bucket / exp-Gauss kernel (single-matrix launchers at num_dim 1 only).
// GPT_KID_PRODUCT_PER (GPT_GFORM_PER: a factor, batched: some kernel of the model, is Periodic or Spectral) is taken for nothing else; it exists at
// every num_dim and carries every branch, so the products of a model that also holds Gibbs terms are in it too.
inline int gibbs_form_of(int D, int id1, int id2)
{
    return ((gibbs_gb_kid(id1) || gibbs_gb_kid(id2)) ? GPT_GFORM_GB : 0) |
           ((D > 1 && (gibbs_kid(id1) || gibbs_kid(id2))) ? GPT_GFORM_ON_DIM : 0) |
           ((id1 == GPT_KERNEL_PERIODIC || id2 == GPT_KERNEL_PERIODIC || id1 == GPT_KERNEL_SPECTRAL || id2 == GPT_KERNEL_SPECTRAL) ? GPT_GFORM_PER : 0);
}
inline int product_kid(int D, int gform, bool gibbs_more, bool batched)
{
    if (gform & GPT_GFORM_PER) return GPT_KID_PRODUCT_PER;
    const bool gb = (gform & GPT_GFORM_GB) != 0;
    if (D > 1) return !(gform & GPT_GFORM_ON_DIM) ? GPT_KERNEL_PRODUCT : gb ? GPT_KID_PRODUCT_GB : GPT_KID_PRODUCT_GM;
    if (gb) return GPT_KID_PRODUCT_GB;
    return batched || gibbs_more ? GPT_KID_PRODUCT_GM : GPT_KERNEL_PRODUCT;
}

constexpr int kid_max_dim(int kid)
{
    return gibbs_kid(kid) ? 1 : kid == GPT_KID_PRODUCT_GM || kid == GPT_KID_PRODUCT_GB ? GPT_GIBBS_ON_DIM_MAX_D : GPT_MAX_DIM;
}
// (the WARP instantiations exist for these only: the noise kernels are never warped)
// what dispatch_dim says when num_dim is beyond kid_max_dim(kid) (NULL: its general message)
static_assert(GPT_GIBBS_ON_DIM_MAX_D == 3, "the message below names the number");
constexpr const char *kid_dim_rule(int kid)
{
    return gibbs_kid(kid) ? "the Gibbs kernels need num_dim 1"
                          : kid == GPT_KID_PRODUCT_GM || kid == GPT_KID_PRODUCT_GB ? "a Gibbs factor needs num_dim <= 3" : nullptr;
}
constexpr bool kid_can_warp(int kid) { return kid != GPT_KERNEL_DIAGNOISE && kid != GPT_KERNEL_ZERO; }

// f(std::integral_constant<int, KID>()) for the entry of the list that equals `kid`, else refuse() -- the launcher's own message
// and status
template <int... KIDS, class F, class R>
int dispatch_kid(KidList<KIDS...>, int kid, F &&f, R &&refuse)
{
    int rc = GPT_OK;
    const bool hit = ((kid == KIDS && (rc = f(std::integral_constant<int, KIDS>()), true)) || ...);
    return hit ? rc : refuse();
}

// One model term given by its factors' ids on a single matrix -- id1, or the product id1 * id2 where id2 >= 0 -- at num_dim D: the
// product instantiation its factors ask for (product_kid), else the fit kernel id1; `who` names the launcher in the refusal.  What
// the pair passes of the gradients launch through (kgrad.hip, kgrad_rect.hip).
template <class F>
int dispatch_term_kid(const char *who, int id1, int id2, int D, F &&for_kid)
{
    if (id2 >= 0)
        return dispatch_kid(ProductKids(), product_kid(D, gibbs_form_of(D, id1, id2), gibbs_more_kid(id1) || gibbs_more_kid(id2), false), for_kid,
                            [] { return GPT_E_ARG; });
    return dispatch_kid(FitKids(), id1, for_kid, [&] {
        gpt_set_error("%s: kernel_id %d is not a fit kernel", who, id1);
        return GPT_E_ARG;
    });
}

template <class F, int... I>
bool dispatch_dim_fold(int D, F &f, int &rc, std::integer_sequence<int, I...>)
{
    return ((D == I + 1 && (rc = f(std::integral_constant<int, I + 1>()), true)) || ...);
}

// f(std::integral_constant<int, D>()) for D in 1 .. MAXD (kid_max_dim); `who` names the launcher in the refusal, `rule` (the
// caller's, kid_dim_rule) says why MAXD is what it is
template <int MAXD, class F>
int dispatch_dim(const char *who, int D, F &&f, const char *rule = nullptr)
{
    int rc = GPT_OK;
    if (dispatch_dim_fold(D, f, rc, std::make_integer_sequence<int, MAXD>())) return rc;
    if (rule) gpt_set_error("%s: %s, got %d", who, rule, D);
    else gpt_set_error("%s: unsupported num_dim %d (max %d)", who, D, MAXD);
    return GPT_E_ARG;
}

// Tiles of the lower triangle of an N x N matrix: row tile rt (KB_ROWS rows) needs column tiles 0 .. rt / KB_RATIO
inline int64_t lower_tile_count(int64_t N)
{
    const int64_t nrt = (N + KB_ROWS - 1) / KB_ROWS;
    int64_t ntile = 0;
    for (int64_t rt = 0; rt < nrt; rt++) ntile += rt / KB_RATIO + 1;
    return ntile;
}

// The builder's grid and the lower_only it is launched with.  A square block on the diagonal with lower_only set (the batched fit
// without a transform asks for exactly that; `full` = lower_only 0) launches only the tiles that exist, in the kernel's mode 2;
// everything else is the whole rectangle.  nbatch: one matrix per blockIdx.z.
struct TileGrid {
    dim3 grid;
    int lower_only;
};
inline TileGrid tile_grid(int64_t M, int64_t P, int lower_only, int64_t i0, int64_t j0, int64_t nbatch = 1)
{
    if (lower_only && i0 == j0 && M == P) return {dim3((unsigned)lower_tile_count(M), 1, (unsigned)nbatch), 2};
    return {dim3((unsigned)((P + KB_COLS - 1) / KB_COLS), (unsigned)((M + KB_ROWS - 1) / KB_ROWS), (unsigned)nbatch), lower_only};
}

// What a batched launch adds to KBuildArgs (common.hpp): element z's hyperparameters kps[z] (kps2[z]: the second factor of a product
// term), its noise variance nvs[z], its matrix at K + z * bstride; warped: its points at X + z * xstride, its slopes at S + z * sstride
struct KBatchArgs {
    const KParams *kps = nullptr;
    const double *nvs = nullptr;
    int64_t nbatch = 1, bstride = 0;
    const KParams *kps2 = nullptr;
    int64_t xstride = 0, sstride = 0;
};

// THE launch of kbuild_kernel: the parameters a mode does not use are padded here, and the WARP instantiation is chosen here (slopes
// given; for the kernels that can warp only).  kp / kp2: the single matrix's hyperparameters (dummies for a batch).
template <int KID, int D, bool BATCH>
int kbuild_launch(hipStream_t st, const KParams &kp, const KParams &kp2, const KBuildArgs &a, const KBatchArgs &b = KBatchArgs())
{
    const TileGrid tg = tile_grid(a.M, a.P, a.lower_only, a.i0, a.j0, b.nbatch);
    const dim3 block(KB_THREADS);
    if constexpr (kid_can_warp(KID)) {
        if (a.Si != nullptr) {
            hipLaunchKernelGGL((kbuild_kernel<KID, D, BATCH, true>), tg.grid, block, 0, st, kp, a.Xi, a.ni, a.M, a.Xj, a.nj, a.P,
                               tg.lower_only, a.i0, a.j0, a.err_y, a.noise_var, a.diag_add, a.K, a.ldk, a.accumulate, b.kps, b.nvs,
                               b.bstride, kp2, b.kps2, a.Si, a.Sj, b.xstride, b.sstride);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        }
    }
    hipLaunchKernelGGL((kbuild_kernel<KID, D, BATCH, false>), tg.grid, block, 0, st, kp, a.Xi, a.ni, a.M, a.Xj, a.nj, a.P, tg.lower_only,
                       a.i0, a.j0, a.err_y, a.noise_var, a.diag_add, a.K, a.ldk, a.accumulate, b.kps, b.nvs, b.bstride, kp2, b.kps2,
                       (const double *)nullptr, (const double *)nullptr, (int64_t)0, (int64_t)0);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// The single-matrix builder / pair list for the ids of one list: AllKids in kbuild.hip, ProductKids (kid from product_kid) in
// kbuild_prod.hip -- each translation unit compiles the instantiations of its list.
template <class LIST>
int kbuild_dispatch(LIST list, int kid, hipStream_t st, const KParams &kp, const KParams &kp2, const KBuildArgs &a)
{
    return dispatch_kid(list, kid, [&](auto k) {
        constexpr int KID = decltype(k)::value;
        if (a.Si != nullptr && (!kid_can_warp(KID) || a.Sj == nullptr)) {
            gpt_set_error("kbuild: warp slopes given for kernel_id %d", kp.kernel_id);
            return GPT_E_ARG;
        }
        return dispatch_dim<kid_max_dim(KID)>("kbuild", kp.D, [&](auto d) { return kbuild_launch<KID, decltype(d)::value, false>(st, kp, kp2, a); }, kid_dim_rule(KID));
    }, [&] {
        gpt_set_error("kbuild: unknown kernel_id %d", kid);
        return GPT_E_ARG;
    });
}

struct KPairsArgs {
    const double *Xi, *Xj;
    const int32_t *ni, *nj;
    int64_t M;
    double *out;
    int accumulate;
};
template <class LIST>
int kpairs_dispatch(LIST list, int kid, hipStream_t st, const KParams &kp, const KParams &kp2, const KPairsArgs &a)
{
    return dispatch_kid(list, kid, [&](auto k) {
        constexpr int KID = decltype(k)::value;
        return dispatch_dim<kid_max_dim(KID)>("kpairs", kp.D, [&](auto d) {
            hipLaunchKernelGGL((kpairs_kernel<KID, decltype(d)::value>), dim3((unsigned)((a.M + 255) / 256)), dim3(256), 0, st, kp, a.Xi, a.Xj,
                               a.ni, a.nj, a.M, a.out, a.accumulate, kp2);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        }, kid_dim_rule(KID));
    }, [&] {
        gpt_set_error("kpairs: unknown kernel_id %d", kid);
        return GPT_E_ARG;
    });
}

// the product halves of launch_kbuild / launch_kpairs (kbuild_prod.hip)
int kbuild_prod(hipStream_t st, const KParams &kp1, const KParams &kp2, const KBuildArgs &a);
int kpairs_prod(hipStream_t st, const KParams &kp1, const KParams &kp2, const KPairsArgs &a);
