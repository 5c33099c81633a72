// kgrad_dz.hip -- the pair pass of gpt_sparse_grad_z (api_sparse_grad.inc): the gradient of the inducing-point objective
// with respect to the inducing INPUTS.  The derivative of a covariance entry with respect to coordinate d of z_m is the same pair
// function with the inducing point's derivative order raised by one in dimension d,
//     d k(x_i, z_m; n_i, n_m) / d z_{m,d} = k(x_i, z_m; n_i, n_m + e_d),
// so for one chunk of rows x_i against the M inducing inputs and ONE model term at its fitted parameters
//     dz[m][d] += sum_i A[i][m] k(x_i, z_m; n_i, n_m + e_d),
// A the chunk's adjoint A_fu (rows x lda, row-major) -- or, with X := Z, nx := n_Z and skip_diag, 2 A_uu whole: the Z-Z pass, which drops
// the pair m' = m (K_uu[m][m] does not depend on z_m for any configuration the call accepts).  A term is evaluated
// through term_pair and the instantiations come from dispatch_term_kid (kbuild_kernel.hpp), as in kgrad_rect.hip.  A translation unit of
// its own: the other code objects stay what they were.
// Geometry: kgrad_rect.hip's.  A tile is KZ_ROWS = 64 rows x 64 columns; the 64 lanes of EVERY wave are the tile's consecutive columns
// m -- z_m and n_m stay in registers, a row of A is one coalesced 512-byte read -- and the four waves take the rows in turn, so M <= 64
// still fills a workgroup.  The result is per column: a lane keeps D accumulators and evaluates the pair D times, the order of dimension
// d raised for evaluation d (a loop that is not unrolled: one copy of the pair function per instantiation).  No cross-lane reduction.
// Determinism: the four waves' sums are added through LDS in wave order, the workgroup writes partial[row tile][m][d], and
// kgrad_dz_finish_kernel -- one thread per (m, d) -- adds the row tiles in index order to the running dz[m][d] of the call, launch after
// launch on one stream.  No floating-point atomics.
#include "kbuild_kernel.hpp"

#define KZ_ROWS 64

// k1 (k2: the second factor of a product term, else unused): the term at its fitted parameters.  partial: gridDim.y x M x D, every entry
// written.  Lanes with m >= M, rows past the tile's end and waves without a row add nothing.
template <int KID, int D>
__global__ __launch_bounds__(256) void kgrad_dz_kernel(KParams k1, KParams k2, const double *__restrict__ X, const int32_t *__restrict__ nx,
                                                       int64_t rows, const double *__restrict__ Z, const int32_t *__restrict__ nz, int64_t M,
                                                       const double *__restrict__ A, int64_t lda, int skip_diag, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool live = j < M;
    const int64_t jc = live ? j : 0;                                // (a lane without a column reads point 0 and adds nothing)
    const int64_t rbase = (int64_t)blockIdx.y * KZ_ROWS;
    const int64_t rend = (rbase + KZ_ROWS < rows) ? rbase + KZ_ROWS : rows;
    double zj[D], acc[D];
    int nzj[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        zj[d] = Z[jc * D + d];
        nzj[d] = nz[jc * D + d];
        acc[d] = 0.0;
    }
    if (live)
        for (int64_t i = rbase + wave; i < rend; i += 4) {
            if (skip_diag && i == j) continue;
            double xi[D];
            int nir[D];
#pragma unroll
            for (int d = 0; d < D; d++) {                           // wave-uniform addresses
                xi[d] = X[i * D + d];
                nir[d] = nx[i * D + d];
            }
            const double w = A[i * lda + j];
#pragma unroll 1
            for (int d = 0; d < D; d++) {
                int nup[D];
#pragma unroll
                for (int q = 0; q < D; q++) nup[q] = nzj[q] + (q == d ? 1 : 0);
                const double v = term_pair<KID, D>(k1, &k2, xi, zj, nir, nup);
#pragma unroll
                for (int q = 0; q < D; q++) acc[q] = (q == d) ? fma(w, v, acc[q]) : acc[q];
            }
        }
    __shared__ double red[4][64][D];
#pragma unroll
    for (int d = 0; d < D; d++) red[wave][lane][d] = acc[d];
    __syncthreads();
    for (int t = threadIdx.x; t < 64 * D; t += 256) {
        const int l = t / D, d = t % D;
        const int64_t m = (int64_t)blockIdx.x * 64 + l;
        if (m < M) partial[((int64_t)blockIdx.y * M + m) * D + d] = ((red[0][l][d] + red[1][l][d]) + red[2][l][d]) + red[3][l][d];
    }
}

// dz[t] += partial[0][t] + partial[1][t] + ..., t < md = M D: the ntile row tiles in index order, one at a time into the running sum
__global__ __launch_bounds__(256) void kgrad_dz_finish_kernel(const double *__restrict__ partial, int64_t ntile, int64_t md, double *__restrict__ dz)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= md) return;
    double s = dz[t];
    for (int64_t b = 0; b < ntile; b++) s += partial[b * md + t];
    dz[t] = s;
}

int64_t kgrad_dz_tiles(int64_t rows) { return (rows + KZ_ROWS - 1) / KZ_ROWS; }

// One launch: ONE term, kernel id1 (* id2 where id2 >= 0, k2 its parameters) at num_dim D.  dpartial: kgrad_dz_tiles(rows) x M x D doubles;
// ddz (M x D, row-major, device) += the sums.
int launch_kgrad_dz(hipStream_t st, int id1, int id2, int D, const KParams &k1, const KParams *k2, const double *dX, const int32_t *dnx,
                    int64_t rows, const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda, int skip_diag,
                    double *dpartial, double *ddz)
{
    if (rows <= 0 || M <= 0 || M > lda || (id2 >= 0 && !k2) || !dX || !dnx || !dZ || !dnz || !dA || !dpartial || !ddz ||
        (rows + KZ_ROWS - 1) / KZ_ROWS > 65535) {
        gpt_set_error("kgrad_dz: bad arguments (rows=%lld, M=%lld, row stride %lld)", (long long)rows, (long long)M, (long long)lda);
        return GPT_E_ARG;
    }
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)kgrad_dz_tiles(rows));
    const KParams &kb = k2 ? *k2 : k1;                              // (no product: the second argument is never read)
    auto for_kid = [&](auto k) {
        constexpr int KID = decltype(k)::value;
        return dispatch_dim<kid_max_dim(KID)>("sparse_grad_z", D, [&](auto d) {
            hipLaunchKernelGGL((kgrad_dz_kernel<KID, decltype(d)::value>), grid, dim3(256), 0, st, k1, kb, dX, dnx, rows, dZ, dnz, M, dA, lda,
                               skip_diag, dpartial);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        }, kid_dim_rule(KID));
    };
    const int rc = dispatch_term_kid("sparse_grad_z", id1, id2, D, for_kid);
    if (rc != GPT_OK) return rc;
    const int64_t md = M * D;
    hipLaunchKernelGGL(kgrad_dz_finish_kernel, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, st, dpartial, kgrad_dz_tiles(rows), md, ddz);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
