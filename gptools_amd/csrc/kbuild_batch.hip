// kbuild_batch.hip -- the covariance builder for a BATCH of independent hyperparameter vectors over the same resident
// points (gpt_fit_batch, include/gpt_hip.h): one launch builds the lower triangles (+ fused diagonal loading) of all the
// K_tot, element z of the batch from its own KParams in device memory.  Same kernel as the single-matrix path
// (kbuild_kernel.hpp), so an element of a batch holds the very numbers gpt_fit would build alone.
// ref: gptools/gaussian_process.py:1607-1692 (compute_ll_matrix) and :723-735 (random starts) evaluate the LML at many
// hyperparameter vectors one after another; this is their builder.
#include <string.h>
#include "kbuild_kernel.hpp"

// full != 0: the whole symmetric N x N matrix of every element (the transform path multiplies it by T from both sides), else
// the tiles of its lower triangle.  d_kps2 (product terms): element z's second factor.
template <int KID>
static int kbuild_batch_d(hipStream_t st, int D, const KParams *d_kps, const double *d_nv, int64_t nbatch, const double *dX,
                          const int32_t *dn, int64_t N, const double *d_err_y, double diag_add, double *dK, int64_t ldk,
                          int64_t bstride, int accumulate, int full, const KParams *d_kps2, int64_t xstride, const double *dS,
                          int64_t sstride)
{
    const int64_t nrt = (N + KB_ROWS - 1) / KB_ROWS;
    int64_t ntile = 0;
    for (int64_t rt = 0; rt < nrt; rt++) ntile += rt / KB_RATIO + 1;
    dim3 grid((unsigned)ntile, 1, (unsigned)nbatch), block(KB_THREADS);
    if (full) grid = dim3((unsigned)((N + KB_COLS - 1) / KB_COLS), (unsigned)nrt, (unsigned)nbatch);
    const int lower = full ? 0 : 2;
    KParams dummy = KParams();
    // (dS != NULL: a warped batch -- element z's points at dX + z * xstride, its slope factors at dS + z * sstride, the WARP instantiation)
#define KBB_CASE(DD)                                                                                              \
    case DD:                                                                                                      \
        if (dS != nullptr) {                                                                                      \
            hipLaunchKernelGGL((kbuild_kernel<KID, DD, true, true>), grid, block, 0, st, dummy, dX, dn, N, dX, dn, N, lower, \
                               (int64_t)0, (int64_t)0, d_err_y, 0.0, diag_add, dK, ldk, accumulate, d_kps, d_nv, bstride, dummy, d_kps2, \
                               dS, dS, xstride, sstride);                                                         \
            break;                                                                                                \
        }                                                                                                         \
        hipLaunchKernelGGL((kbuild_kernel<KID, DD, true>), grid, block, 0, st, dummy, dX, dn, N, dX, dn, N, lower, \
                           (int64_t)0, (int64_t)0, d_err_y, 0.0, diag_add, dK, ldk, accumulate, d_kps, d_nv, bstride, dummy, d_kps2, \
                           (const double *)nullptr, (const double *)nullptr); \
        break;
    if constexpr (gibbs_kid(KID) || KID == GPT_KID_PRODUCT_GM) {      // (1-D kernels: one instantiation)
        switch (D) {
            KBB_CASE(1)
        default:
            gpt_set_error("kbuild_batch: the Gibbs kernels need num_dim 1, got %d", D);
            return GPT_E_ARG;
        }
    } else switch (D) {
        KBB_CASE(1) KBB_CASE(2) KBB_CASE(3) KBB_CASE(4) KBB_CASE(5) KBB_CASE(6) KBB_CASE(7) KBB_CASE(8)
        KBB_CASE(9) KBB_CASE(10) KBB_CASE(11) KBB_CASE(12) KBB_CASE(13) KBB_CASE(14) KBB_CASE(15) KBB_CASE(16)
    default:
        gpt_set_error("kbuild_batch: unsupported num_dim %d (max %d)", D, GPT_MAX_DIM);
        return GPT_E_ARG;
    }
#undef KBB_CASE
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_kbuild_batch(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_noise_var, int64_t nbatch,
                        const double *dX, const int32_t *dn, int64_t N, const double *d_err_y, double diag_add, double *dK,
                        int64_t ldk, int64_t bstride, int accumulate, int full, const KParams *d_kps2, int64_t xstride,
                        const double *dS, int64_t sstride)
{
    if (N <= 0 || nbatch <= 0) return GPT_OK;
    if (d_kps2 != nullptr)           // a product term: the factors' kernel ids are read from the elements' KParams at run time
        return D == 1 ? kbuild_batch_d<GPT_KID_PRODUCT_GM>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride,
                                                           accumulate, full, d_kps2, xstride, dS, sstride)
                      : kbuild_batch_d<GPT_KERNEL_PRODUCT>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride,
                                                           accumulate, full, d_kps2, xstride, dS, sstride);
    switch (kernel_id) {
    case GPT_KERNEL_SE: return kbuild_batch_d<GPT_KERNEL_SE>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_M52: return kbuild_batch_d<GPT_KERNEL_M52>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_RQ: return kbuild_batch_d<GPT_KERNEL_RQ>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_MATERN: return kbuild_batch_d<GPT_KERNEL_MATERN>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_GIBBS_TANH: return kbuild_batch_d<GPT_KERNEL_GIBBS_TANH>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_GIBBS_DTANH: return kbuild_batch_d<GPT_KERNEL_GIBBS_DTANH>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_GIBBS_CUBIC: return kbuild_batch_d<GPT_KERNEL_GIBBS_CUBIC>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_GIBBS_QUINTIC: return kbuild_batch_d<GPT_KERNEL_GIBBS_QUINTIC>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    case GPT_KERNEL_GIBBS_EXPGAUSS: return kbuild_batch_d<GPT_KERNEL_GIBBS_EXPGAUSS>(st, D, d_kps, d_noise_var, nbatch, dX, dn, N, d_err_y, diag_add, dK, ldk, bstride, accumulate, full, nullptr, xstride, dS, sstride);
    default:
        gpt_set_error("kbuild_batch: kernel_id %d is not a fit kernel", kernel_id);
        return GPT_E_ARG;
    }
}

// ---- the predictive half of a resident batch (gpt_predict_batch, api_batch.inc) ----------------------------------------
// Cross-covariance of every element: rows = the M test points Xi, columns = the P resident points Xj, the whole rectangle
// (K*_b^T, or K**_b with Xi = Xj), element z at dK + z * bstride.  Sums and products as launch_kbuild_batch: later terms
// accumulate, a product term reads its factors' ids from the elements' KParams.
// (d_nv: the elements' noise variances -- the batched kernel reads its element's entry, though without err_y nothing uses it)
template <int KID>
static int kbuild_batch_cross_d(hipStream_t st, int D, const KParams *d_kps, const double *d_nv, int64_t nbatch, const double *dXi,
                                const int32_t *dni, int64_t M, const double *dXj, const int32_t *dnj, int64_t P, double *dK, int64_t ldk,
                                int64_t bstride, int accumulate, const KParams *d_kps2)
{
    dim3 grid((unsigned)((P + KB_COLS - 1) / KB_COLS), (unsigned)((M + KB_ROWS - 1) / KB_ROWS), (unsigned)nbatch), block(KB_THREADS);
    KParams dummy = KParams();
#define KBC_CASE(DD)                                                                                                         \
    case DD:                                                                                                                 \
        hipLaunchKernelGGL((kbuild_kernel<KID, DD, true>), grid, block, 0, st, dummy, dXi, dni, M, dXj, dnj, P, 0, (int64_t)0, \
                           (int64_t)0, nullptr, 0.0, 0.0, dK, ldk, accumulate, d_kps, d_nv, bstride, dummy, d_kps2,          \
                           (const double *)nullptr, (const double *)nullptr);                                        \
        break;
    if constexpr (gibbs_kid(KID) || KID == GPT_KID_PRODUCT_GM) {
        switch (D) {
            KBC_CASE(1)
        default:
            gpt_set_error("kbuild_batch_cross: the Gibbs kernels need num_dim 1, got %d", D);
            return GPT_E_ARG;
        }
    } else switch (D) {
        KBC_CASE(1) KBC_CASE(2) KBC_CASE(3) KBC_CASE(4) KBC_CASE(5) KBC_CASE(6) KBC_CASE(7) KBC_CASE(8)
        KBC_CASE(9) KBC_CASE(10) KBC_CASE(11) KBC_CASE(12) KBC_CASE(13) KBC_CASE(14) KBC_CASE(15) KBC_CASE(16)
    default:
        gpt_set_error("kbuild_batch_cross: unsupported num_dim %d (max %d)", D, GPT_MAX_DIM);
        return GPT_E_ARG;
    }
#undef KBC_CASE
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_kbuild_batch_cross(hipStream_t st, int kernel_id, int D, const KParams *d_kps, const double *d_nv, int64_t nbatch,
                              const double *dXi, const int32_t *dni, int64_t M, const double *dXj, const int32_t *dnj, int64_t P, double *dK,
                              int64_t ldk, int64_t bstride, int accumulate, const KParams *d_kps2)
{
    if (M <= 0 || P <= 0 || nbatch <= 0) return GPT_OK;
    if (!d_kps || !d_nv) {
        gpt_set_error("kbuild_batch_cross: the elements' KParams and noise variances must be device arrays");
        return GPT_E_ARG;
    }
    if (d_kps2 != nullptr)
        return D == 1 ? kbuild_batch_cross_d<GPT_KID_PRODUCT_GM>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, d_kps2)
                      : kbuild_batch_cross_d<GPT_KERNEL_PRODUCT>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, d_kps2);
    switch (kernel_id) {
    case GPT_KERNEL_SE: return kbuild_batch_cross_d<GPT_KERNEL_SE>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_M52: return kbuild_batch_cross_d<GPT_KERNEL_M52>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_RQ: return kbuild_batch_cross_d<GPT_KERNEL_RQ>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_MATERN: return kbuild_batch_cross_d<GPT_KERNEL_MATERN>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_GIBBS_TANH: return kbuild_batch_cross_d<GPT_KERNEL_GIBBS_TANH>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_GIBBS_DTANH: return kbuild_batch_cross_d<GPT_KERNEL_GIBBS_DTANH>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_GIBBS_CUBIC: return kbuild_batch_cross_d<GPT_KERNEL_GIBBS_CUBIC>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_GIBBS_QUINTIC: return kbuild_batch_cross_d<GPT_KERNEL_GIBBS_QUINTIC>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    case GPT_KERNEL_GIBBS_EXPGAUSS: return kbuild_batch_cross_d<GPT_KERNEL_GIBBS_EXPGAUSS>(st, D, d_kps, d_nv, nbatch, dXi, dni, M, dXj, dnj, P, dK, ldk, bstride, accumulate, nullptr);
    default:
        gpt_set_error("kbuild_batch_cross: kernel_id %d is not a fit kernel", kernel_id);
        return GPT_E_ARG;
    }
}

// One term of element b's kernel at a pair, kernels chosen at run time (the two kernels below loop over terms AND elements,
// whose ids only the KParams carry): the same pair functions as the builder, so the same numbers.
template <int D>
__device__ __forceinline__ double batch_term_pair(const KParams *__restrict__ kps, const KParams *__restrict__ kps2, int64_t idx,
                                                  const double *xi, const double *xj, const int *ni, const int *nj)
{
    // (D == 1: with the bucket / exp-Gauss Gibbs branches, GPT_KID_PRODUCT_GM's form; otherwise the functions the builders share)
    if (kps2 != nullptr && kps2[idx].kernel_id >= 0) return prod_pair<D, D == 1>(kps[idx], kps2[idx], xi, xj, ni, nj);
    return factor_pair<D, D == 1>(kps[idx], xi, xj, ni, nj);
}

// diag K**_b: out[b * ldo + a] = k_b((x_a, n_a), (x_a, n_a)), terms summed in order (as gpt_predict's pair launches do)
template <int D>
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
        const double p = batch_term_pair<D>(kps, kps2, (int64_t)t * nbatch + b, x, x, na, na);
        v = t > 0 ? v + p : p;
    }
    out[b * ldo + a] = v;
}

// Lower triangle of  C = sum over kept elements b of K**_b  (+ noise_sum on the diagonal of the rows hit[a] != 0): ONE pass over
// the M x M triangle with the elements' KParams looped inside, 16 x 16 entries per workgroup; rows / columns in [M, MP) get 0.
template <int D>
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
                const double p = batch_term_pair<D>(kps, kps2, (int64_t)t * nbatch + b, xa, xc, na, nc);
                kb = t > 0 ? kb + p : p;
            }
            v += kb;
        }
        if (a == cc && hit != nullptr && hit[a]) v += noise_sum;
    }
    C[a * ldc + cc] = v;
}

int launch_kdiag_batch(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const double *dX,
                       const int32_t *dn, int64_t M, double *dout, int64_t ldo)
{
    if (M <= 0 || nbatch <= 0) return GPT_OK;
    dim3 grid((unsigned)((M + 255) / 256), (unsigned)nbatch);
#define KD_CASE(DD)                                                                                                               \
    case DD:                                                                                                                      \
        hipLaunchKernelGGL(kdiag_batch_kernel<DD>, grid, dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, dX, dn, M, dout, ldo); \
        break;
    switch (D) {
        KD_CASE(1) KD_CASE(2) KD_CASE(3) KD_CASE(4) KD_CASE(5) KD_CASE(6) KD_CASE(7) KD_CASE(8)
        KD_CASE(9) KD_CASE(10) KD_CASE(11) KD_CASE(12) KD_CASE(13) KD_CASE(14) KD_CASE(15) KD_CASE(16)
    default:
        gpt_set_error("kdiag_batch: unsupported num_dim %d (max %d)", D, GPT_MAX_DIM);
        return GPT_E_ARG;
    }
#undef KD_CASE
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_kss_sum(hipStream_t st, int D, int nterms, const KParams *d_kps, const KParams *d_kps2, int64_t nbatch, const int32_t *d_keep,
                   const double *dX, const int32_t *dn, int64_t M, int64_t MP, const int32_t *d_hit, double noise_sum, double *dC,
                   int64_t ldc)
{
    if (MP <= 0) return GPT_OK;
    const unsigned nt = (unsigned)((MP + 15) / 16);
    dim3 grid(nt, nt);
#define KS_CASE(DD)                                                                                                                  \
    case DD:                                                                                                                         \
        hipLaunchKernelGGL(kss_sum_kernel<DD>, grid, dim3(256), 0, st, nterms, d_kps, d_kps2, nbatch, d_keep, dX, dn, M, MP, d_hit, \
                           noise_sum, dC, ldc);                                                                                      \
        break;
    switch (D) {
        KS_CASE(1) KS_CASE(2) KS_CASE(3) KS_CASE(4) KS_CASE(5) KS_CASE(6) KS_CASE(7) KS_CASE(8)
        KS_CASE(9) KS_CASE(10) KS_CASE(11) KS_CASE(12) KS_CASE(13) KS_CASE(14) KS_CASE(15) KS_CASE(16)
    default:
        gpt_set_error("kss_sum: unsupported num_dim %d (max %d)", D, GPT_MAX_DIM);
        return GPT_E_ARG;
    }
#undef KS_CASE
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
