// kbuild_batch.hip -- the covariance builder for a BATCH of independent hyperparameter vectors over the same resident
// points (gpt_fit_batch, include/gpt_hip.h): one launch builds the lower triangles (+ fused diagonal loading) of all the
// K_tot, element z of the batch from its own KParams in device memory.  Same kernel as the single-matrix path
// (kbuild_kernel.hpp), so an element of a batch holds the very numbers gpt_fit would build alone.
// ref: gptools/gaussian_process.py:1607-1692 (compute_ll_matrix) and :723-735 (random starts) evaluate the LML at many
// hyperparameter vectors one after another; this is their builder.
// The launchers fill KBuildArgs / KBatchArgs and go through the dispatch of kbuild_kernel.hpp (FitKids; a product term:
// ProductKids by product_kid); the two kernels of the predictive half that loop over terms and elements are defined here.
#include "kbuild_kernel.hpp"

// One term of every element: kernel_id, or (d_kps2 != NULL) a product term, whose factors' ids the kernel reads from the elements'
// KParams at run time.  `who` names the launcher in a refusal.
// gform: ModelKernel::gibbs_form() -- GPT_GFORM_GB: the model holds a B-spline or nested-GP Gibbs kernel, a product term then takes GPT_KID_PRODUCT_GB;
// GPT_GFORM_ON_DIM: it holds a Gibbs factor on one coordinate of num_dim > 1, a product term then takes the GM / GB form
// of that num_dim (product_kid).
static int kbuild_batch_dispatch(const char *who, hipStream_t st, int kernel_id, int D, const KBuildArgs &a, const KBatchArgs &b, int gform)
{
    const KParams dummy = KParams();
    auto for_kid = [&](auto k) {
        constexpr int KID = decltype(k)::value;
        return dispatch_dim<kid_max_dim(KID)>(who, D, [&](auto d) { return kbuild_launch<KID, decltype(d)::value, true>(st, dummy, dummy, a, b); }, kid_dim_rule(KID));
    };
    if (b.kps2 != nullptr) return dispatch_kid(ProductKids(), product_kid(D, gform, false, true), for_kid, [] { return GPT_E_ARG; });
    return dispatch_kid(FitKids(), kernel_id, for_kid, [&] {
        gpt_set_error("%s: kernel_id %d is not a fit kernel", who, kernel_id);
        return GPT_E_ARG;
    });
}

// full != 0: the whole symmetric N x N matrix of every element (the transform path multiplies it by T from both sides), else
// the tiles of its lower triangle.  d_kps2 (product terms): element z's second factor.
// (dS != NULL: a warped batch -- element z's points at dX + z * xstride, its slope factors at dS + z * sstride, the WARP instantiation)
int launch_kbuild_batch(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_noise_var, int64_t nbatch,
                        const double *dX, const int32_t *dn, int64_t N, const double *d_err_y, double diag_add, double *dK,
                        int64_t ldk, int64_t bstride, int accumulate, int full, const KParams *d_kps2, int64_t xstride,
                        const double *dS, int64_t sstride, int gform)
{
    if (N <= 0 || nbatch <= 0) return GPT_OK;
    const KBuildArgs a = {dX, dn, N, dX, dn, N, full ? 0 : 1, 0, 0, d_err_y, 0.0, diag_add, dK, ldk, accumulate, dS, dS};
    const KBatchArgs b = {d_kps, d_noise_var, nbatch, bstride, d_kps2, xstride, sstride};
    return kbuild_batch_dispatch("kbuild_batch", st, kernel_id, D, a, b, gform);
}

// ---- the predictive half of a resident batch (gpt_predict_batch, api_batch.inc) ----------------------------------------
// Cross-covariance of every element: rows = the M test points Xi, columns = the P resident points Xj, the whole rectangle
// (K*_b^T, or K**_b with Xi = Xj), element z at dK + z * bstride.  Sums and products as launch_kbuild_batch: later terms
// accumulate, a product term reads its factors' ids from the elements' KParams.
// (d_nv: the elements' noise variances -- the batched kernel reads its element's entry, though without err_y nothing uses it)
int launch_kbuild_batch_cross(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_nv, int64_t nbatch,
                              const double *dXi, const int32_t *dni, int64_t M, const double *dXj, const int32_t *dnj, int64_t P, double *dK,
                              int64_t ldk, int64_t bstride, int accumulate, const KParams *d_kps2, int gform)
{
    if (M <= 0 || P <= 0 || nbatch <= 0) return GPT_OK;
    if (!d_kps || !d_nv) {
        gpt_set_error("kbuild_batch_cross: the elements' KParams and noise variances must be device arrays");
        return GPT_E_ARG;
    }
    const KBuildArgs a = {dXi, dni, M, dXj, dnj, P, 0, 0, 0, nullptr, 0.0, 0.0, dK, ldk, accumulate};
    const KBatchArgs b = {d_kps, d_nv, nbatch, bstride, d_kps2};
    return kbuild_batch_dispatch("kbuild_batch_cross", st, kernel_id, D, a, b, gform);
}

// One term of element b's kernel at a pair, kernels chosen at run time (the two kernels below loop over terms AND elements,
// whose ids only the KParams carry): the same pair functions as the builder, so the same numbers.
// GB: with the B-spline and nested-GP branches (GPT_KID_PRODUCT_GB's form; models that hold such a kernel only)
// GM: with the Gibbs branches of GPT_KID_PRODUCT_GM -- every 1-D model, and at num_dim 2 .. GPT_GIBBS_ON_DIM_MAX_D the models with a
// Gibbs factor on one coordinate (instantiations of their own: the kernels of every other model at those num_dim are the code they were)
// PER: with the periodic kernel's branch (GPT_KID_PRODUCT_PER's form: GB and GM set too; models that hold a Periodic or a Spectral kernel only)
template <int D, bool GB = false, bool GM = (D == 1), bool PER = false>
__device__ __forceinline__ double batch_term_pair(const KParams *__restrict__ kps, const KParams *__restrict__ kps2, int64_t idx,
                                                  const double *xi, const double *xj, const int *ni, const int *nj)
{
    // (D == 1: with the bucket / exp-Gauss Gibbs branches, GPT_KID_PRODUCT_GM's form; otherwise the functions the builders share)
    if (kps2 != nullptr && kps2[idx].kernel_id >= 0) return prod_pair<D, GM, GB, PER>(kps[idx], kps2[idx], xi, xj, ni, nj);
    return factor_pair<D, GM, GB, PER>(kps[idx], xi, xj, ni, nj);
}

// diag K**_b: out[b * ldo + a] = k_b((x_a, n_a), (x_a, n_a)), terms summed in order (as gpt_predict's pair launches do)
// (GB, here and in kss_sum_kernel: the form for a 1-D model that holds a B-spline or nested-GP kernel; a flag of the kernel itself, not a shared
// body behind two kernels -- through a wrapper the pointers lose __restrict__ and the code of every num_dim changes)
template <int D, bool GB = false, bool GM = (D == 1), bool PER = false>
__global__ __launch_bounds__(256) void kdiag_batch_kernel(int nterms, const KParams *__restrict__ kps, const KParams *__restrict__ kps2,
                                                          int64_t nbatch, const double *__restrict__ X, const int32_t *__restrict__ n,
                                                          int64_t M, double *__restrict__ out, int64_t ldo)
{
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (a >= M) return;
    double x[D];
    int na[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        x[d] = X[a * D + d];
        na[d] = n[a * D + d];
    }
    double v = 0.0;
    for (int t = 0; t < nterms; t++) {
        const double p = batch_term_pair<D, GB, GM, PER>(kps, kps2, (int64_t)t * nbatch + b, x, x, na, na);
        v = t > 0 ? v + p : p;
    }
    out[b * ldo + a] = v;
}

// Lower triangle of  C = sum over kept elements b of K**_b  (+ noise_sum on the diagonal of the rows hit[a] != 0): ONE pass over
// the M x M triangle with the elements' KParams looped inside, 16 x 16 entries per workgroup; rows / columns in [M, MP) get 0.
template <int D, bool GB = false, bool GM = (D == 1), bool PER = false>
__global__ __launch_bounds__(256) void kss_sum_kernel(int nterms, const KParams *__restrict__ kps, const KParams *__restrict__ kps2,
                                                      int64_t nbatch, const int32_t *__restrict__ keep, const double *__restrict__ X,
                                                      const int32_t *__restrict__ n, int64_t M, int64_t MP, const int32_t *__restrict__ hit,
                                                      double noise_sum, double *__restrict__ C, int64_t ldc)
{
    if (blockIdx.x > blockIdx.y) return;                                  // tile strictly above the diagonal
    const int64_t a = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4), cc = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
    if (a >= MP || cc > a) return;
    double v = 0.0;
    if (a < M) {
        double xa[D], xc[D];
        int na[D], nc[D];
#pragma unroll
        for (int d = 0; d < D; d++) {
            xa[d] = X[a * D + d];
            na[d] = n[a * D + d];
            xc[d] = X[cc * D + d];
            nc[d] = n[cc * D + d];
        }
        for (int64_t b = 0; b < nbatch; b++) {
            if (!keep[b]) continue;
            double kb = 0.0;
            for (int t = 0; t < nterms; t++) {
                const double p = batch_term_pair<D, GB, GM, PER>(kps, kps2, (int64_t)t * nbatch + b, xa, xc, na, nc);
                kb = t > 0 ? kb + p : p;
            }
            v += kb;
        }
        if (a == cc && hit != nullptr && hit[a]) v += noise_sum;
    }
    C[a * ldc + cc] = v;
}

// gform: ModelKernel::gibbs_form() (see kbuild_batch_dispatch): the kernel with the B-spline branch at num_dim 1, the kernels
// with the on-coordinate Gibbs branches at num_dim 2 .. GPT_GIBBS_ON_DIM_MAX_D
// f(D, GB) for the on-coordinate forms
template <class F>
static int dispatch_on_dim(const char *who, int D, int gform, F &&f)
{
    return dispatch_dim<GPT_GIBBS_ON_DIM_MAX_D>(who, D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if constexpr (DD == 1) return GPT_E_ARG;      // (never: the callers come here with num_dim > 1)
        else return (gform & GPT_GFORM_GB) ? f(d, std::true_type()) : f(d, std::false_type());
    }, kid_dim_rule(GPT_KID_PRODUCT_GM));
}

int launch_kdiag_batch(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const double *dX,
                       const int32_t *dn, int64_t M, double *dout, int64_t ldo, int gform)
{
    if (M <= 0 || nbatch <= 0) return GPT_OK;
    if (gform & GPT_GFORM_PER)      // a model with a Periodic or a Spectral kernel: the one form with every branch, at every num_dim
        return dispatch_dim<GPT_MAX_DIM>("kdiag_batch", D, [&](auto d) {
            hipLaunchKernelGGL((kdiag_batch_kernel<decltype(d)::value, true, true, true>), dim3((unsigned)((M + 255) / 256), (unsigned)nbatch),
                               dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, dX, dn, M, dout, ldo);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        });
    if ((gform & GPT_GFORM_ON_DIM) && D > 1)
        return dispatch_on_dim("kdiag_batch", D, gform, [&](auto d, auto gb) {
            hipLaunchKernelGGL((kdiag_batch_kernel<decltype(d)::value, decltype(gb)::value, true>), dim3((unsigned)((M + 255) / 256), (unsigned)nbatch),
                               dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, dX, dn, M, dout, ldo);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        });
    if ((gform & GPT_GFORM_GB) && D == 1) {
        hipLaunchKernelGGL((kdiag_batch_kernel<1, true>), dim3((unsigned)((M + 255) / 256), (unsigned)nbatch), dim3(256), 0, st, nterms, d_kps,
                           d_kps2, nbatch, dX, dn, M, dout, ldo);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    }
    return dispatch_dim<GPT_MAX_DIM>("kdiag_batch", D, [&](auto d) {
        hipLaunchKernelGGL((kdiag_batch_kernel<decltype(d)::value, false>), dim3((unsigned)((M + 255) / 256), (unsigned)nbatch), dim3(256), 0, st,
                           nterms, d_kps, d_kps2, nbatch, dX, dn, M, dout, ldo);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    });
}

int launch_kss_sum(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const int32_t *d_keep,
                   const double *dX, const int32_t *dn, int64_t M, int64_t MP, const int32_t *d_hit, double noise_sum, double *dC,
                   int64_t ldc, int gform)
{
    if (MP <= 0) return GPT_OK;
    const unsigned nt = (unsigned)((MP + 15) / 16);
    if (gform & GPT_GFORM_PER)
        return dispatch_dim<GPT_MAX_DIM>("kss_sum", D, [&](auto d) {
            hipLaunchKernelGGL((kss_sum_kernel<decltype(d)::value, true, true, true>), dim3(nt, nt), dim3(256), 0, st, nterms, d_kps, d_kps2,
                               nbatch, d_keep, dX, dn, M, MP, d_hit, noise_sum, dC, ldc);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        });
    if ((gform & GPT_GFORM_ON_DIM) && D > 1)
        return dispatch_on_dim("kss_sum", D, gform, [&](auto d, auto gb) {
            hipLaunchKernelGGL((kss_sum_kernel<decltype(d)::value, decltype(gb)::value, true>), dim3(nt, nt), dim3(256), 0, st, nterms, d_kps,
                               d_kps2, nbatch, d_keep, dX, dn, M, MP, d_hit, noise_sum, dC, ldc);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        });
    if ((gform & GPT_GFORM_GB) && D == 1) {
        hipLaunchKernelGGL((kss_sum_kernel<1, true>), dim3(nt, nt), dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, d_keep, dX, dn, M, MP,
                           d_hit, noise_sum, dC, ldc);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    }
    return dispatch_dim<GPT_MAX_DIM>("kss_sum", D, [&](auto d) {
        hipLaunchKernelGGL((kss_sum_kernel<decltype(d)::value, false>), dim3(nt, nt), dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, d_keep, dX, dn,
                           M, MP, d_hit, noise_sum, dC, ldc);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    });
}
