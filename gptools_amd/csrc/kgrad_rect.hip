// kgrad_rect.hip -- the RECTANGULAR pair pass of gpt_sparse_grad_diff (api_sparse_grad.inc): for one chunk of training
// rows x_i against the M inducing inputs z_m, per free parameter h of one model term,
//     sum_im A[i][m] (k_b - k_a)(x_i, z_m)  +  1/2 sum_i e_i (k_b - k_a)(x_i, x_i),
// A the chunk's adjoint A_fu (rows x lda, row-major) and k_a / k_b the term at the two stencil points of parameter h.  As in kgrad.hip
// the difference is taken PER PAIR, before the weight, the stencil points' KParams live in device memory and are read by reference with
// wave-uniform indices, the parameters of a launch are walked by a loop that is not unrolled, a term is evaluated through term_pair
// and the instantiations come from dispatch_term_kid (both kbuild_kernel.hpp, both shared with kgrad.hip: FitKids, ProductKids by
// product_kid).  A translation unit of its own: the builders' and kgrad.hip's code objects stay what they were.
// Geometry.  kgrad_diff_kernel's tiles (32 rows x 256 columns of the lower triangle, a lane per column) do not fit: M is often <= 64, and
// three of a workgroup's four waves would own no column at all.  Here a tile is KR_ROWS = 64 rows x 64 columns: the 64 lanes of EVERY
// wave are the tile's 64 consecutive columns m -- a lane keeps its z_m in registers, and a row of A is read as one 512-byte line,
// coalesced along m -- and the four waves take the tile's rows in turn (row rbase + wave, + 4, ...), so a row's point x_i arrives
// through wave-uniform loads and M <= 64 still fills all four waves.  The grid is (column tiles) x (row tiles): one column tile and
// rows / 64 workgroups at M <= 64, 455 workgroups for a 29120-row chunk.  The diagonal part belongs to the first column tile: lane l of
// wave 0 adds row rbase + l's entry, one extra pair per lane against sixteen.  (The 1-D Gibbs kernels go through the general pair
// function here, without kgrad.hip's length-scale hoist: a row's point is shared by a wave, not by a tile.)
// Determinism: a workgroup writes its KR_MAXH partial sums (waves added in index order); kgrad_rect_finish_kernel adds the workgroups'
// partial sums to the running sums of the call -- thread t the workgroups t, t + 256, ..., then a fixed tree -- chunk after chunk on
// one stream.  No floating-point atomics.
#include "kbuild_kernel.hpp"

#define KR_MAXH GPT_GRAD_MAXH
#define KR_ROWS 64

// kps[2 h], kps[2 h + 1]: the term at the stencil points a, b of parameter h < nh <= KR_MAXH (kps2: the second factors of a product
// term, else unused).  e == NULL: no diagonal part.  partial: (gridDim.y * gridDim.x) x KR_MAXH, every entry written.
template <int KID, int D>
__global__ __launch_bounds__(256) void kgrad_rect_diff_kernel(const KParams *__restrict__ kps, const KParams *__restrict__ kps2, int nh,
                                                              const double *__restrict__ X, const int32_t *__restrict__ nx, int64_t rows,
                                                              const double *__restrict__ Z, const int32_t *__restrict__ nz, int64_t M,
                                                              const double *__restrict__ A, int64_t lda, const double *__restrict__ e,
                                                              double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t j = (int64_t)blockIdx.x * 64 + lane;
    const bool live = j < M;
    const int64_t jc = live ? j : 0;                                // (a lane without a column reads point 0 and adds nothing)
    const int64_t rbase = (int64_t)blockIdx.y * KR_ROWS;
    const int64_t rend = (rbase + KR_ROWS < rows) ? rbase + KR_ROWS : rows;
    double zj[D];
    int nzj[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        zj[d] = Z[jc * D + d];
        nzj[d] = nz[jc * D + d];
    }
    // the diagonal part: this lane's row of the tile (first column tile, wave 0 only)
    const int64_t idg = rbase + lane;
    const bool diag = e != nullptr && blockIdx.x == 0 && wave == 0 && idg < rend;
    const int64_t ic = diag ? idg : 0;
    double xd[D];
    int nd[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        xd[d] = X[ic * D + d];
        nd[d] = nx[ic * D + d];
    }
    const double ed = diag ? 0.5 * e[ic] : 0.0;
    __shared__ double red[4][KR_MAXH];
#pragma unroll 1
    for (int h = 0; h < KR_MAXH; h++) {
        double acc = 0.0;
        if (h < nh) {
            const KParams &ka = kps[2 * h], &kb = kps[2 * h + 1];
            const KParams *ka2 = nullptr, *kb2 = nullptr;
            if constexpr (is_product_kid(KID)) {
                ka2 = kps2 + 2 * h;
                kb2 = kps2 + 2 * h + 1;
            }
            if (live)
                for (int64_t i = rbase + wave; i < rend; i += 4) {
                    double xi[D];
                    int nir[D];
#pragma unroll
                    for (int d = 0; d < D; d++) {                   // wave-uniform addresses
                        xi[d] = X[i * D + d];
                        nir[d] = nx[i * D + d];
                    }
                    const double w = A[i * lda + j];
                    const double dk = term_pair<KID, D>(kb, kb2, xi, zj, nir, nzj) - term_pair<KID, D>(ka, ka2, xi, zj, nir, nzj);
                    acc = fma(w, dk, acc);
                }
            if (diag) {
                const double dk = term_pair<KID, D>(kb, kb2, xd, xd, nd, nd) - term_pair<KID, D>(ka, ka2, xd, xd, nd, nd);
                acc = fma(ed, dk, acc);
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) red[wave][h] = acc;
    }
    __syncthreads();
    if (threadIdx.x < KR_MAXH) {
        const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[blk * KR_MAXH + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}

// acc[h] += sum over the nblk workgroups of partial[blk][h], h = blockIdx.x < nh: thread t adds blocks t, t + 256, ... in index order,
// then the tree below -- a fixed order for a given nblk
__global__ __launch_bounds__(256) void kgrad_rect_finish_kernel(const double *__restrict__ partial, int64_t nblk, double *__restrict__ acc)
{
    __shared__ double s[4];
    const int h = blockIdx.x;
    double a = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += 256) a += partial[b * KR_MAXH + h];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) acc[h] += ((s[0] + s[1]) + s[2]) + s[3];
}

int64_t kgrad_rect_blocks(int64_t rows, int64_t M) { return ((rows + KR_ROWS - 1) / KR_ROWS) * ((M + 63) / 64); }

// One launch: nh <= GPT_GRAD_MAXH parameters of ONE term, kernel id1 (* id2 where id2 >= 0) at num_dim D; d_kps / d_kps2: 2 nh KParams
// each in device memory (d_kps2 only for a product).  dpartial: kgrad_rect_blocks(rows, M) x GPT_GRAD_MAXH doubles; dacc[h] += the sum.
int launch_kgrad_rect_diff(hipStream_t st, int id1, int id2, int D, const KParams *d_kps, const KParams *d_kps2, int nh, const double *dX,
                           const int32_t *dnx, int64_t rows, const double *dZ, const int32_t *dnz, int64_t M, const double *dA, int64_t lda,
                           const double *de, double *dpartial, double *dacc)
{
    if (nh < 1 || nh > KR_MAXH || rows <= 0 || M <= 0 || M > lda || !d_kps || (id2 >= 0 && !d_kps2) || !dX || !dnx || !dZ || !dnz || !dA ||
        !dpartial || !dacc || (rows + KR_ROWS - 1) / KR_ROWS > 65535) {
        gpt_set_error("kgrad_rect_diff: bad arguments (nh=%d, rows=%lld, M=%lld, row stride %lld)", nh, (long long)rows, (long long)M,
                      (long long)lda);
        return GPT_E_ARG;
    }
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)((rows + KR_ROWS - 1) / KR_ROWS));
    auto for_kid = [&](auto k) {
        constexpr int KID = decltype(k)::value;
        return dispatch_dim<kid_max_dim(KID)>("sparse_grad_diff", D, [&](auto d) {
            hipLaunchKernelGGL((kgrad_rect_diff_kernel<KID, decltype(d)::value>), grid, dim3(256), 0, st, d_kps, d_kps2, nh, dX, dnx, rows, dZ,
                               dnz, M, dA, lda, de, dpartial);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        }, kid_dim_rule(KID));
    };
    const int rc = dispatch_term_kid("sparse_grad_diff", id1, id2, D, for_kid);
    if (rc != GPT_OK) return rc;
    hipLaunchKernelGGL(kgrad_rect_finish_kernel, dim3((unsigned)nh), dim3(256), 0, st, dpartial, kgrad_rect_blocks(rows, M), dacc);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
