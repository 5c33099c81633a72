// kgrad.hip -- the pair pass of gpt_ll_grad_diff (api_grad.inc): the LML gradient of ANY model term by per-pair central
// differences of its pair function,
//     d ll / d theta_h ~= 1/2 sum_ab (alpha_a alpha_b - W_ab) (k_b - k_a)[a][b] / (theta_b - theta_a),   W = K_tot^-1 resident,
// where k_a / k_b are the term at the two stencil points of parameter h.  The difference is taken PER PAIR, before the weight
// (differencing the two weighted sums instead loses a digit: the sums are large and nearly equal), and the division by the
// step is the host's, once per parameter.  Geometry and reduction are grad_reduce_kernel's (kbuild.hip): the tiles of the lower
// triangle, a workgroup owns 32 x 256 pairs, each lane keeps its column's point, the rows arrive through wave-uniform loads,
// the strictly lower part counts twice; per-workgroup partial sums that the host adds in index order (deterministic); slot
// GR_MAXH of a partial row carries sum_i (alpha_i^2 - W_ii), the same bits grad_reduce_kernel leaves there.
// The stencil points' KParams (two per parameter, four for a product term: 656 bytes each) do not fit the kernel arguments: they
// live in device memory and are read BY REFERENCE with wave-uniform indices, as the batched builder reads kps[z] -- never copied
// per lane.  The parameters of a launch are walked by an outer loop that is not unrolled, so an instantiation holds the pair
// function twice (a and b), whatever the number of parameters.  That trades bandwidth for registers: every parameter reads the
// tile's weights again (W, alpha, the rows' points: N^2 / 2 doubles of W per parameter, 1 GB at N = 16384), where
// grad_reduce_kernel forms a pair's weight once for its eight parameters but holds eight accumulators and its pair function
// eight times.  For the cheap pair functions the pass is then bound by that traffic (Matern-5/2, N = 16384: 0.47 ms per
// parameter); next to K_tot^-1 (57 ms there) it does not show.  The 1-D Gibbs kernels hoist their length scales out of the pair
// loop as the builder does.
// Instantiated through the dispatch the builders share (kbuild_kernel.hpp, dispatch_term_kid): FitKids for a plain term, ProductKids
// by product_kid for a product term -- the form its factors' gform asks for; a term at one pair is term_pair, there too (both shared
// with the rectangular pass, kgrad_rect.hip).  A translation unit of its own: the builders' code objects stay
// what they were.
// A BATCH (gpt_ll_grad_diff_batch, the gradient half of a resident batch): the element is the grid's second dimension.  Element e
// reads its own stencil points kps[2 nh e ..], its own alpha + e ldw and W + e ldw^2 and writes its own partial rows behind those
// of the elements before it -- the strides follow from nh, ldw and the grid, so the kernel takes no further argument, and e is
// wave-uniform: the element costs scalar registers only.  The single route is element 0 of a batch of one: the same instructions
// on the same addresses, the same bits.  Tile geometry and summation order do not know the batch, so an element's partial sums
// are the same whatever the batch around it is.  The LEAVE-ONE-OUT gradient (gpt_loo_grad_diff, api_loo.inc) is the same
// pass with other weights, u_a alpha_b + alpha_a u_b - V_ab: a second vector u and V in the place of W, chosen at run time per launch
// (kgrad_weight below).  kgrad_batch_finish_kernel adds the partial sums of every element and launch
// group in index order, as the host does for the single route, and alpha of a batch comes from kgrad_batch_alpha_kernel.
#include "kbuild_kernel.hpp"

#define GR_MAXH GPT_GRAD_MAXH

// The weight of pair (i, j), lane j: alpha_i alpha_j - W_ij for the LML (u == alpha, loo false: the expression this file has always
// had there), u_i alpha_j + alpha_i u_j - V_ij for the leave-one-out objective (gpt_loo_grad_diff: W is V = W diag(e) W then).  `loo`
// is the same in every lane of a launch -- one scalar branch per pair, not a template parameter: that would double every KID x D
// instantiation.  On the diagonal this is the trace slot's entry, 2 u_i alpha_i - V_ii.
__device__ __forceinline__ double kgrad_weight(bool loo, const double *__restrict__ alpha, const double *__restrict__ u,
                                               const double *__restrict__ W, int64_t ldw, int64_t i, int64_t j, double aj, double uj)
{
    if (loo) return (u[i] * aj + alpha[i] * uj) - W[i * ldw + j];
    return alpha[i] * aj - W[i * ldw + j];
}

// kps[2 h], kps[2 h + 1]: the term at the stencil points a, b of parameter h < nh <= GR_MAXH (kps2: the second factors of a product
// term, else unused); partial: grad_reduce_blocks(N) x (GR_MAXH + 1), every entry written.  blockIdx.y: the element of a batch (see
// the head of this file), 0 on the single route
template <int KID, int D>
__global__ __launch_bounds__(KB_THREADS) void kgrad_diff_kernel(
    const KParams *__restrict__ kps_, const KParams *__restrict__ kps2_, int nh, const double *__restrict__ X,
    const int32_t *__restrict__ nn, int64_t N, const double *__restrict__ alpha_, const double *__restrict__ W_, int64_t ldw,
    double *__restrict__ partial_, const double *__restrict__ u_)
{
    constexpr int64_t R = KB_RATIO;
    const int64_t e = blockIdx.y;
    const KParams *__restrict__ kps = kps_ + e * 2 * nh;
    const KParams *__restrict__ kps2 = kps2_ + e * 2 * nh;         // (only a product term reads it)
    const double *__restrict__ alpha = alpha_ + e * ldw;
    const double *__restrict__ W = W_ + e * ldw * ldw;
    const bool loo = u_ != nullptr;                                 // (a kernel argument: wave-uniform)
    const double *__restrict__ u = loo ? u_ + e * ldw : alpha;
    double *__restrict__ partial = partial_ + e * (int64_t)gridDim.x * (GR_MAXH + 1);
    const int64_t b = blockIdx.x;
    int64_t g = (int64_t)((sqrt(1.0 + 8.0 * (double)b / (double)R) - 1.0) * 0.5);
    while (g > 0 && R * g * (g + 1) / 2 > b) g--;
    while (R * (g + 1) * (g + 2) / 2 <= b) g++;
    const int64_t rem = b - R * g * (g + 1) / 2;
    const int64_t rt = R * g + rem / (g + 1), ct = rem % (g + 1);
    const int64_t rbase = rt * KB_ROWS, j = ct * KB_COLS + threadIdx.x;
    const bool live = rbase < N && j < N;
    const int64_t jc = live ? j : 0;                                // (a lane without a column reads point 0 and adds nothing)
    const int64_t rend = (rbase + KB_ROWS < N) ? rbase + KB_ROWS : N;
    double xj[D];
    int njr[D];
#pragma unroll
    for (int d = 0; d < D; d++) {
        xj[d] = X[jc * D + d];
        njr[d] = nn[jc * D + d];
    }
    const double aj = alpha[jc], uj = u[jc];
    __shared__ double red[KB_THREADS / 64][GR_MAXH + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int h = 0; h <= GR_MAXH; h++) {
        double acc = 0.0;
        if constexpr (gibbs_kid(KID)) {
            // The 1-D Gibbs kernels with the builder's hoist (kbuild_kernel.hpp): the length scale is formed once per point and
            // stencil -- this lane's column, and the tile's 32 rows once per wave, lane q (and q + 32) row rbase + q, read back
            // with v_readlane before the lanes part ways -- so a pair costs two gibbs_core, not eight length-scale evaluations
            // (measured, DoubleTanh at N = 16384: 10.0 -> 0.82 ms per parameter).  EVERY lane takes part in the hoist, the ones
            // without a column too: a row's point may sit in such a lane.
            static_assert(D == 1, "the Gibbs kernels are one-dimensional");
            if (h < nh) {
                const KParams &ka = kps[2 * h], &kb = kps[2 * h + 1];
                const GibbsPt ca = gibbs_point<KID>(ka, xj[0]), cb = gibbs_point<KID>(kb, xj[0]);
                const int64_t ir = (rbase + (lane & 31) < N) ? rbase + (lane & 31) : N - 1;
                const double xr = X[ir];
                const GibbsPt ra = gibbs_point<KID>(ka, xr), rb = gibbs_point<KID>(kb, xr);
                const double s2a = ka.sigma * ka.sigma, s2b = kb.sigma * kb.sigma;
                for (int64_t i = rbase; i < rend; i++) {
                    const int q = (int)(i - rbase);
                    const double xi = X[i];
                    const int nir = nn[i];
                    const double la = readlane_f64(ra.l, q), Aa = readlane_f64(ra.A, q), ha = readlane_f64(ra.h, q), qa = readlane_f64(ra.r2, q);
                    const double lb = readlane_f64(rb.l, q), Ab = readlane_f64(rb.A, q), hb = readlane_f64(rb.h, q), qb = readlane_f64(rb.r2, q);
                    if (!live || j > i) continue;                   // lower triangle (wave-uniform row, per-lane column)
                    const bool need_d = (nir | njr[0]) != 0;
                    const double va = gibbs_core(s2a, xi, la, Aa, gibbs_h_other<KID>(ha, ca.l), qa, xj[0], ca.l, ca.A, gibbs_h_other<KID>(ca.h, la),
                                                 gibbs_col_root(la, ca.rp, ca.rn), nir, njr[0], need_d);
                    const double vb = gibbs_core(s2b, xi, lb, Ab, gibbs_h_other<KID>(hb, cb.l), qb, xj[0], cb.l, cb.A, gibbs_h_other<KID>(cb.h, lb),
                                                 gibbs_col_root(lb, cb.rp, cb.rn), nir, njr[0], need_d);
                    const double w = kgrad_weight(loo, alpha, u, W, ldw, i, j, aj, uj);
                    acc = fma((i == j) ? w : 2.0 * w, vb - va, acc);
                }
            }
        } else if (live && h < nh) {
            const KParams &ka = kps[2 * h], &kb = kps[2 * h + 1];
            const KParams *ka2 = nullptr, *kb2 = nullptr;
            if constexpr (is_product_kid(KID)) {
                ka2 = kps2 + 2 * h;
                kb2 = kps2 + 2 * h + 1;
            }
            for (int64_t i = rbase; i < rend; i++) {
                if (j > i) continue;                                // lower triangle (wave-uniform row, per-lane column)
                double xi[D];
                int nir[D];
#pragma unroll
                for (int d = 0; d < D; d++) {
                    xi[d] = X[i * D + d];
                    nir[d] = nn[i * D + d];
                }
                const double w = kgrad_weight(loo, alpha, u, W, ldw, i, j, aj, uj);
                const double w2 = (i == j) ? w : 2.0 * w;
                const double dk = term_pair<KID, D>(kb, kb2, xi, xj, nir, njr) - term_pair<KID, D>(ka, ka2, xi, xj, nir, njr);
                acc = fma(w2, dk, acc);
            }
        }
        // the noise trace: this lane's diagonal entry, if the tile holds it
        if (live && h == GR_MAXH && j >= rbase && j < rend) acc += kgrad_weight(loo, alpha, u, W, ldw, j, j, aj, uj);
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0) red[wave][h] = acc;
    }
    __syncthreads();
    if (threadIdx.x <= GR_MAXH) {
        double v = 0.0;
        for (int wv = 0; wv < KB_THREADS / 64; wv++) v += red[wv][threadIdx.x];
        partial[(int64_t)blockIdx.x * (GR_MAXH + 1) + threadIdx.x] = v;
    }
}

// One launch: nh <= GPT_GRAD_MAXH parameters of ONE term, kernel id1 (* id2 where id2 >= 0) at num_dim D; d_kps / d_kps2: 2 nh
// KParams each in device memory (d_kps2 only for a product).  The N points dX / dn against the weights alpha alpha^T - W.
// nbatch > 1: that many elements, element e with d_kps + 2 nh e, dalpha + e ldw, dW + e ldw^2 and dpartial + e
// grad_reduce_blocks(N) (GR_MAXH + 1); the points are shared.  du (N; NULL for the LML): the second vector of the leave-one-out
// weights u alpha^T + alpha u^T - V, with V in the place of W (kgrad_weight).
int launch_kgrad_diff(hipStream_t st, int id1, int id2, int D, const KParams *d_kps, const KParams *d_kps2, int nh, const double *dX,
                      const int32_t *dn, int64_t N, const double *dalpha, const double *dW, int64_t ldw, double *dpartial, int64_t nbatch,
                      const double *du)
{
    if (nh < 0 || nh > GR_MAXH || N <= 0 || !d_kps || (id2 >= 0 && !d_kps2) || nbatch < 1 || nbatch > 65535 || (nbatch > 1 && ldw < N))
        return GPT_E_ARG;
    auto for_kid = [&](auto k) {
        constexpr int KID = decltype(k)::value;
        return dispatch_dim<kid_max_dim(KID)>("ll_grad_diff", D, [&](auto d) {
            hipLaunchKernelGGL((kgrad_diff_kernel<KID, decltype(d)::value>), dim3((unsigned)grad_reduce_blocks(N), (unsigned)nbatch), dim3(KB_THREADS), 0, st,
                               d_kps, d_kps2, nh, dX, dn, N, dalpha, dW, ldw, dpartial, du);
            GPT_LAUNCH_CHECK();
            return GPT_OK;
        }, kid_dim_rule(KID));
    };
    return dispatch_term_kid("ll_grad_diff", id1, id2, D, for_kid);
}

// alpha_b = U_b z_b over the N points of every element of a resident batch: U_b = L_b^-T (upper triangular, row stride ldu, element
// stride su), z_b = L_b^-1 y_b the augmented row N of element b's factor (A + b sa + N lda).  One wave per row, the row's sum in
// the lane order and by the shuffle tree below whatever the batch is; alpha + b sal, entries [N, sal) set to zero.
__global__ __launch_bounds__(256) void kgrad_batch_alpha_kernel(const double *__restrict__ U, int64_t ldu, int64_t su,
                                                                 const double *__restrict__ A, int64_t lda, int64_t sa, int64_t N,
                                                                 double *__restrict__ alpha, int64_t sal)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (i >= sal) return;
    double s = 0.0;
    if (i < N) {
        const double *row = U + b * su + i * ldu, *z = A + b * sa + N * lda;
        for (int64_t k = i - (i & 63) + lane; k < N; k += 64)            // (U is upper triangular: columns < i hold zeros)
            if (k >= i) s = fma(row[k], z[k], s);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    }
    if (lane == 0) alpha[b * sal + i] = s;
}

int launch_kgrad_batch_alpha(hipStream_t st, const double *dU, int64_t ldu, int64_t su, const double *dA, int64_t lda, int64_t sa,
                             int64_t N, int64_t nbatch, double *dalpha, int64_t sal)
{
    if (N <= 0 || sal < N || ldu < N || nbatch < 1 || nbatch > 65535) return GPT_E_ARG;
    hipLaunchKernelGGL(kgrad_batch_alpha_kernel, dim3((unsigned)((sal + 3) / 4), (unsigned)nbatch), dim3(256), 0, st, dU, ldu, su, dA, lda,
                       sa, N, dalpha, sal);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// out[b][j] = 1/2 sum over the nblk workgroups, in index order, of entry src[j] of element b's partial rows: partial holds, launch
// group after launch group, nbatch x nblk rows of GR_MAXH + 1 sums; src[j] = group (GR_MAXH + 1) + slot names the group and slot of
// output j < nout.  One thread per (b, j): the order of the additions is the host's on the single route and knows nothing of the
// batch.
__global__ __launch_bounds__(64) void kgrad_batch_finish_kernel(const double *__restrict__ partial, const int32_t *__restrict__ src,
                                                                int nout, int64_t nblk, int64_t nbatch, double *__restrict__ out)
{
    const int64_t b = blockIdx.y;
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nout) return;
    const int64_t group = src[j] / (GR_MAXH + 1), slot = src[j] % (GR_MAXH + 1);
    const double *p = partial + ((group * nbatch + b) * nblk) * (GR_MAXH + 1) + slot;
    double sum = 0.0;
    for (int64_t w = 0; w < nblk; w++) sum += p[w * (GR_MAXH + 1)];
    out[b * nout + j] = 0.5 * sum;
}

int launch_kgrad_batch_finish(hipStream_t st, const double *dpartial, const int32_t *dsrc, int nout, int64_t nblk, int64_t nbatch,
                              double *dout)
{
    if (nout < 1 || nblk < 1 || nbatch < 1 || nbatch > 65535) return GPT_E_ARG;
    hipLaunchKernelGGL(kgrad_batch_finish_kernel, dim3((unsigned)((nout + 63) / 64), (unsigned)nbatch), dim3(64), 0, st, dpartial, dsrc, nout,
                       nblk, nbatch, dout);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
