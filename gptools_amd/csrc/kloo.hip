// kloo.hip -- the device side of the leave-one-out entry points (gpt_loo, gpt_loo_grad_diff: api_loo.inc).
// With W = K_tot^-1 = U U^T, U = L^-T, and alpha = W (y - T mu):
//     d_i = W_ii = sum_{i <= k < N} U_ik^2        r_i = alpha_i / d_i = y_i - m_i        s_i^2 = 1 / d_i
//     L_LOO = sum_i [ 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 pi ]
// (Rasmussen & Williams 5.4.2) -- the diagonal from the triangular inverse alone, N^3 / 3 flop, no U U^T.  The gradient brings
// the objective into the shape of the LML's, 1/2 sum_ab G_ab dK_ab, with the weights
//     G = u alpha^T + alpha u^T - V,     u = W r,     V = W diag(e) W = A A^T,     A = W diag(sqrt e),     e_i = (1 + alpha_i^2 / d_i) / d_i > 0:
// loo_terms_kernel leaves d, r, sqrt(e) and the rows' terms of L_LOO, loo_sum_kernel adds the terms in index order, and
// loo_scale_cols_kernel forms A from the mirrored W.  A A^T is the GEMM's, u a launch_gemv_n, the pair pass kgrad.hip's.
// U is the inverse transpose of the AUGMENTED factor, order NP: column N belongs to the augmented row (-(alpha) / d there, d^2 some
// 1e300) and the columns behind it to the padding, so the sums stop at N.  Rows >= N get d = 1, r = sqrt(e) = 0 and a zero term:
// the columns >= N of A are exact zeros, and every entry of A is finite where W is.
#include "common.hpp"

// One wave per row of U (the geometry and shuffle tree of kgrad_batch_alpha_kernel, kgrad.hip): row i's sum of squares over the
// columns [i, N) in lane order, then the row's four results by lane 0.  Rows [N, NP) are the padding's.
__global__ __launch_bounds__(256) void loo_terms_kernel(const double *__restrict__ U, int64_t ldu, const double *__restrict__ alpha,
                                                         int64_t N, int64_t NP, double *__restrict__ d, double *__restrict__ r,
                                                         double *__restrict__ se, double *__restrict__ term)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= NP) return;                                                  // (wave-uniform)
    if (i >= N) {
        if (lane == 0) {
            d[i] = 1.0;
            r[i] = 0.0;
            se[i] = 0.0;
            term[i] = 0.0;
        }
        return;
    }
    const double *row = U + i * ldu;
    double s = 0.0;
    for (int64_t k = i - (i & 63) + lane; k < N; k += 64)                 // (U is upper triangular: columns < i hold zeros)
        if (k >= i) s = fma(row[k], row[k], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        const double a = alpha[i], q = a * a / s;
        d[i] = s;
        r[i] = a / s;
        se[i] = sqrt((1.0 + q) / s);
        term[i] = 0.5 * log(s) - 0.5 * q - 0.9189385332046727;           // 1/2 log 2 pi
    }
}

// out[0] = sum_{i < n} term[i]: thread t adds its run of consecutive entries in index order, thread 0 the 256 runs in index order --
// the same additions on every call, whatever else the device is doing.
__global__ __launch_bounds__(256) void loo_sum_kernel(const double *__restrict__ term, int64_t n, double *__restrict__ out)
{
    __shared__ double part[256];
    const int64_t run = (n + 255) / 256, lo = (int64_t)threadIdx.x * run, hi = (lo + run < n) ? lo + run : n;
    double s = 0.0;
    for (int64_t i = lo; i < hi; i++) s += term[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int t = 0; t < 256; t++) tot += part[t];
        out[0] = tot;
    }
}

// A (n x n, row stride lda) = W diag(se): column j of the full (mirrored) W times se[j].  A lane owns a column, a workgroup 256
// columns of 8 rows: every global access is a run of consecutive doubles.
__global__ __launch_bounds__(256) void loo_scale_cols_kernel(const double *__restrict__ W, int64_t ldw, const double *__restrict__ se,
                                                              int64_t n, double *__restrict__ A, int64_t lda)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x, i0 = (int64_t)blockIdx.y * 8;
    if (j >= n) return;
    const double f = se[j];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int64_t i = i0 + q;
        if (i < n) A[i * lda + j] = W[i * ldw + j] * f;
    }
}

// d, r, se, term: NP doubles each, every entry written; out1: the sum of the first N terms
int launch_loo_terms(hipStream_t st, const double *dU, int64_t ldu, const double *dalpha, int64_t N, int64_t NP, double *d, double *r,
                     double *se, double *term, double *out1)
{
    if (N <= 0 || NP < N || ldu < NP || !dU || !dalpha || !d || !r || !se || !term || !out1) return GPT_E_ARG;
    hipLaunchKernelGGL(loo_terms_kernel, dim3((unsigned)((NP + 3) / 4)), dim3(256), 0, st, dU, ldu, dalpha, N, NP, d, r, se, term);
    GPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(loo_sum_kernel, dim3(1), dim3(256), 0, st, term, N, out1);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_loo_scale_cols(hipStream_t st, const double *dW, int64_t ldw, const double *se, int64_t n, double *dA, int64_t lda)
{
    if (n <= 0 || ldw < n || lda < n || !dW || !se || !dA) return GPT_E_ARG;
    hipLaunchKernelGGL(loo_scale_cols_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((n + 7) / 8)), dim3(256), 0, st, dW, ldw, se, n,
                       dA, lda);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
