// ksparse.hip -- device kernels of the inducing-point (FITC / VFE / DTC) path, gfx950.
//
// One chunk of training rows arrives as V^T (rows x LDV, row-major): row i holds (L_u^-1 k(Z, x_i))^T in columns [0, M), zeros
// behind.  sparse_lambda_kernel turns it into V~^T -- every row scaled by Lambda_i^-1/2, with r~_i = Lambda_i^-1/2 r_i in column M
// -- and the hot path, sparse_gram_kernel, adds V~ V~^T over the chunk's rows to G (lower 64 x 64 tiles): the contraction index is
// the ROW of the chunk, so both MFMA operands of a k-step are 16-double segments of the same four rows and nothing is transposed.
// With the r~ column, row M of G is b = V Lambda^-1 r and G[M][M] = r^T Lambda^-1 r: the augmented factorisation of B = I + G
// delivers c = L_B^-1 b in its row M.
//
// Determinism: every sum has a fixed order.  The Gram kernel splits the chunk's rows into S slices, workgroup (tile, slice) writes
// its partial tile to a workspace and sparse_gram_reduce_kernel adds the S partials to G in slice order: no floating-point atomics.
//
// The gradient of the objective (gpt_sparse_grad_diff) adds, at the end of this file, its per-row pass
// (sparse_grad_rows_kernel, which forms q_i and Lambda_i through the functions the fit's row pass forms them with), the rank-one part
// of A_fu and two small kernels of order M; its Gram V diag(e) V^T, for weights of either sign, is the two-operand instantiation of
// sparse_gram_kernel.
#include "common.hpp"

// ---- per-row pass ------------------------------------------------------------------------------------------------------------------
// What the fit's row pass and the gradient's (sparse_grad_rows_kernel, below) must form alike, bit for bit -- a row the fit accepted has
// the same Lambda_i in the gradient that differentiates it.  This thread's share of q_i = |v_i|^2 over the columns [0, M) of a row:
// two accumulators at a stride of 512, joined at the end.  The wave and workgroup reductions behind it are each kernel's own.
__device__ __forceinline__ double sparse_row_sumsq(const double *__restrict__ row, int64_t M)
{
    double a0 = 0.0, a1 = 0.0;
    int64_t c = threadIdx.x;
    for (; c + 256 < M; c += 512) {
        const double v0 = row[c], v1 = row[c + 256];
        a0 = fma(v0, v0, a0);
        a1 = fma(v1, v1, a1);
    }
    for (; c < M; c += 256) {
        const double v0 = row[c];
        a0 = fma(v0, v0, a0);
    }
    return a0 + a1;
}

// Lambda_i from kmq = k_i - q_i (entered for fitc only: vfe and dtc may pass anything -- the fit's row pass passes a k_i nobody wrote
// for dtc, the gradient's passes 0) and s_i; ok: a positive finite number.  (fitc as a bool, not the method: with the method as an
// argument the compiler lays out the gradient's row pass otherwise.)
struct SparseLambda {
    double lam;
    bool ok;
};
__device__ __forceinline__ SparseLambda sparse_lambda_of(bool fitc, double kmq, double s)
{
    const double lam = fitc ? kmq + s : s;
    return SparseLambda{lam, lam > 0.0 && lam < INFINITY};
}

// method: 0 fitc (Lambda_i = k_i - q_i + s_i), 1 vfe, 2 dtc (Lambda_i = s_i); s_i = noise_var + err_i^2.
// rowval[i] = log Lambda_i, rowval[ldr + i] = (k_i - q_i) / s_i (vfe, else 0).  A row whose Lambda_i is not a positive finite number
// raises *bad and contributes nothing (its scale is 0): the host reads the word once, at the end of the fit.
// The ONE body of the row pass, inlined into its two kernels below: every pointer is the element's own already.
__device__ __forceinline__ void sparse_lambda_rows(double *__restrict__ V, int64_t ldv, int64_t rows, int64_t M, int method,
                                                   const double *__restrict__ kdiag, const double *__restrict__ r,
                                                   const double *__restrict__ err, double noise_var, double *__restrict__ rowval,
                                                   int64_t ldr, int32_t *__restrict__ bad)
{
    __shared__ double part[4];
    __shared__ double scale;
    const int64_t i = blockIdx.x;
    if (i >= rows) return;
    double *row = V + i * ldv;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = sparse_row_sumsq(row, M);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double q = (part[0] + part[1]) + (part[2] + part[3]);
        const double e = err[i], s = noise_var + e * e, kmq = kdiag[i] - q;
        const SparseLambda L = sparse_lambda_of(method == 0, kmq, s);
        const double lam = L.lam;
        const bool ok = L.ok;
        if (!ok) *bad = 1;
        rowval[i] = ok ? log(lam) : 0.0;
        rowval[ldr + i] = (ok && method == 1) ? kmq / s : 0.0;
        scale = ok ? 1.0 / sqrt(lam) : 0.0;
    }
    __syncthreads();
    const double sc = scale;
    for (int64_t c = threadIdx.x; c < M; c += 256) row[c] *= sc;
    if (threadIdx.x == 0) row[M] = r[i] * sc;
}

// The single fit's: one chunk, noise_var by value, one word.
__global__ __launch_bounds__(256) void sparse_lambda_kernel(double *__restrict__ V, int64_t ldv, int64_t rows, int64_t M, int method,
                                                            const double *__restrict__ kdiag, const double *__restrict__ r,
                                                            const double *__restrict__ err, double noise_var,
                                                            double *__restrict__ rowval, int64_t ldr, int32_t *__restrict__ bad)
{
    sparse_lambda_rows(V, ldv, rows, M, method, kdiag, r, err, noise_var, rowval, ldr, bad);
}

// A batch's: element b = blockIdx.y on V + b vstride, kdiag + b kstride, r + b rstride, rowval + b rvstride with
// noise_var[b] and bad[b]; err is shared.  A bad row raises bad[b] only and zeroes its own row.
__global__ __launch_bounds__(256) void sparse_lambda_batch_kernel(double *__restrict__ V, int64_t ldv, int64_t vstride, int64_t rows, int64_t M,
                                                                  int method, const double *__restrict__ kdiag, int64_t kstride,
                                                                  const double *__restrict__ r, int64_t rstride,
                                                                  const double *__restrict__ err, const double *__restrict__ noise_var,
                                                                  double *__restrict__ rowval, int64_t ldr, int64_t rvstride,
                                                                  int32_t *__restrict__ bad)
{
    const int64_t b = blockIdx.y;
    sparse_lambda_rows(V + b * vstride, ldv, rows, M, method, kdiag + b * kstride, r + b * rstride, err, noise_var[b], rowval + b * rvstride,
                       ldr, bad + b);
}

// Both launchers: the checks, the grid (rows, elements).  noise_var_b NULL: the single kernel with noise_var_1 (nbatch is 1 then).
static int sparse_lambda_launch(hipStream_t st, const char *who, int64_t nbatch, double *V, int64_t ldv, int64_t vstride, int64_t rows, int64_t M,
                                int method, const double *kdiag, int64_t kstride, const double *r, int64_t rstride, const double *err,
                                const double *noise_var_b, double noise_var_1, double *rowval, int64_t ldr, int64_t rvstride, int32_t *bad)
{
    if (rows <= 0 || nbatch <= 0) return GPT_OK;
    if (M < 0 || M >= ldv || rows > ldr || nbatch > 65535 || vstride < rows * ldv || rvstride < 2 * ldr) {
        gpt_set_error("%s: M = %lld does not leave a column for r in rows of %lld, or %lld rows (value stride %lld), %lld elements %lld / %lld apart",
                      who, (long long)M, (long long)ldv, (long long)rows, (long long)ldr, (long long)nbatch, (long long)vstride,
                      (long long)rvstride);
        return GPT_E_ARG;
    }
    const dim3 grid((unsigned)rows, (unsigned)nbatch);
    if (noise_var_b)
        hipLaunchKernelGGL(sparse_lambda_batch_kernel, grid, dim3(256), 0, st, V, ldv, vstride, rows, M, method, kdiag, kstride, r, rstride, err,
                           noise_var_b, rowval, ldr, rvstride, bad);
    else
        hipLaunchKernelGGL(sparse_lambda_kernel, grid, dim3(256), 0, st, V, ldv, rows, M, method, kdiag, r, err, noise_var_1, rowval, ldr, bad);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_sparse_lambda(hipStream_t st, double *V, int64_t ldv, int64_t rows, int64_t M, int method, const double *kdiag,
                         const double *r, const double *err, double noise_var, double *rowval, int64_t ldr, int32_t *bad)
{
    return sparse_lambda_launch(st, "sparse_lambda", 1, V, ldv, rows * ldv, rows, M, method, kdiag, 0, r, 0, err, nullptr, noise_var, rowval, ldr,
                                2 * ldr, bad);
}

int launch_sparse_lambda_batch(hipStream_t st, int64_t nbatch, double *V, int64_t ldv, int64_t vstride, int64_t rows, int64_t M, int method,
                               const double *kdiag, int64_t kstride, const double *r, int64_t rstride, const double *err,
                               const double *noise_var, double *rowval, int64_t ldr, int64_t rvstride, int32_t *bad)
{
    if (!noise_var) return GPT_E_ARG;
    return sparse_lambda_launch(st, "sparse_lambda_batch", nbatch, V, ldv, vstride, rows, M, method, kdiag, kstride, r, rstride, err, noise_var,
                                0.0, rowval, ldr, rvstride, bad);
}

// acc[0] += sum_i rowval[i], acc[1] += sum_i rowval[ldr + i] over the chunk's rows: one workgroup per element (blockIdx.x, on rowval +
// b rvstride and acc + b astride), a fixed order
__global__ __launch_bounds__(256) void sparse_rowsum_kernel(const double *__restrict__ rowval, int64_t ldr, int64_t rvstride, int64_t rows,
                                                            double *__restrict__ acc, int64_t astride)
{
    __shared__ double s0[4], s1[4];
    rowval += (int64_t)blockIdx.x * rvstride;
    acc += (int64_t)blockIdx.x * astride;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {
        a += rowval[i];
        b += rowval[ldr + i];
    }
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        s0[threadIdx.x >> 6] = a;
        s1[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        acc[0] += ((s0[0] + s0[1]) + s0[2]) + s0[3];
        acc[1] += ((s1[0] + s1[1]) + s1[2]) + s1[3];
    }
}

static int sparse_rowsum_launch(hipStream_t st, const char *who, int64_t nbatch, const double *rowval, int64_t ldr, int64_t rvstride, int64_t rows,
                                double *acc, int64_t astride)
{
    if (rows <= 0 || nbatch <= 0) return GPT_OK;
    if (rows > ldr || rvstride < 2 * ldr || astride < 2) {
        gpt_set_error("%s: %lld rows with a value stride of %lld, elements %lld / %lld apart", who, (long long)rows, (long long)ldr,
                      (long long)rvstride, (long long)astride);
        return GPT_E_ARG;
    }
    hipLaunchKernelGGL(sparse_rowsum_kernel, dim3((unsigned)nbatch), dim3(256), 0, st, rowval, ldr, rvstride, rows, acc, astride);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_sparse_rowsum(hipStream_t st, const double *rowval, int64_t ldr, int64_t rows, double *acc)
{
    return sparse_rowsum_launch(st, "sparse_rowsum", 1, rowval, ldr, 2 * ldr, rows, acc, 2);
}

int launch_sparse_rowsum_batch(hipStream_t st, int64_t nbatch, const double *rowval, int64_t ldr, int64_t rvstride, int64_t rows, double *acc,
                               int64_t astride)
{
    return sparse_rowsum_launch(st, "sparse_rowsum_batch", nbatch, rowval, ldr, rvstride, rows, acc, astride);
}

// ---- the weighted Gram -------------------------------------------------------------------------------------------------------------
// Workgroup (tile t, slice s): tile t is the 64 x 64 block (ti, tj), tj <= ti, of the lower triangle in row-major tile order; slice s
// the rows [s * slice_rows, min(rows, (s + 1) * slice_rows)) of the chunk.  Four waves in a 2 x 2 arrangement, 32 x 32 results each:
// two A and two B fragments per k-step of four rows feed four v_mfma_f64_16x16x4_f64.  Operand lane map (fr = lane & 15, fk = lane >>
// 4): A holds A[fr][fk], B holds B[fk][fr], result register q holds C[fk + 4 q][fr]; here A[i][k] = V[k][i0 + i], B[k][j] =
// V[k][j0 + j], so lanes 0-15 of either operand read 16 consecutive doubles of row k.  Rows past the slice's end load as 0.0 (no
// access), so a slice or chunk may end anywhere, below four rows too.  Columns: i0 + 63 < mg <= ldv by the launcher's check.
// part: (nslices x ntiles) tiles of 4096 doubles, tile-local row-major; every workgroup writes its whole tile.
// TWO: the signed-weight Gram of the gradient, tile (ti, tj) += sum_k A[k][i0 + i] V[k][j0 + j] with A a second
// matrix of V's shape -- A holds the rows e_k v_k, and e_k changes sign, so the rows cannot be scaled by a square root and fed in
// as one operand.  Without TWO, A is not read and both operands come from V: the fit's instantiation, the code it was before the
// gradient existed.  A template flag, not a run-time test, for that reason.
// BATCH: workgroup (tile, slice, element b = blockIdx.z) on V + b vstride and part + b pstride, the element's own (slices x tiles) partial
// tiles (gpt_sparse_fit_batch).  Without BATCH neither blockIdx.z nor a stride is read: a flag for the reason TWO is
// one.  Instantiated: <false, false> the fit's, <true, false> the gradient's, <false, true> the batch's.
#define SG_UNROLL 4

// (ti, tj), tj <= ti, from the row-major index t of the lower triangle's tiles: ti (ti + 1) / 2 <= t
__device__ __forceinline__ void sparse_tile_of(int t, int *ti_out, int *tj_out)
{
    int ti = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    while (ti * (ti + 1) / 2 > t) ti--;
    *ti_out = ti;
    *tj_out = t - ti * (ti + 1) / 2;
}

template <bool TWO, bool BATCH>
__global__ __launch_bounds__(256) void sparse_gram_kernel(const double *__restrict__ A, const double *__restrict__ V, int64_t ldv,
                                                          int64_t rows, int64_t slice_rows, int ntiles, double *__restrict__ part,
                                                          int64_t vstride, int64_t pstride)
{
    static_assert(!(TWO && BATCH), "the signed-weight Gram has no batched form: A carries no element stride");
    const int t = blockIdx.x, s = blockIdx.y;
    if (BATCH) {
        V += (int64_t)blockIdx.z * vstride;
        part += (int64_t)blockIdx.z * pstride;
    }
    int ti, tj;
    sparse_tile_of(t, &ti, &tj);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t i0 = (int64_t)ti * 64 + (wave >> 1) * 32, j0 = (int64_t)tj * 64 + (wave & 1) * 32;
    const int64_t k0 = (int64_t)s * slice_rows;
    const int64_t k1 = (k0 + slice_rows < rows) ? k0 + slice_rows : rows;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t k = k0; k < k1; k += 4 * SG_UNROLL) {
        double av[SG_UNROLL][2], bv[SG_UNROLL][2];
#pragma unroll
        for (int u = 0; u < SG_UNROLL; u++) {
            const int64_t kr = k + 4 * u + fk;
            const bool live = kr < k1;
            const double *rb = V + kr * ldv, *ra = TWO ? A + kr * ldv : rb;
            av[u][0] = live ? ra[i0 + fr] : 0.0;
            av[u][1] = live ? ra[i0 + 16 + fr] : 0.0;
            bv[u][0] = live ? rb[j0 + fr] : 0.0;
            bv[u][1] = live ? rb[j0 + 16 + fr] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < SG_UNROLL; u++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u][a], bv[u][b], acc[a][b], 0, 0, 0);
    }
    double *out = part + ((int64_t)s * ntiles + t) * 4096;
    const int li = (wave >> 1) * 32, lj = (wave & 1) * 32;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int q = 0; q < 4; q++) out[(li + a * 16 + fk + 4 * q) * 64 + lj + b * 16 + fr] = acc[a][b][q];
}

// G tile (ti, tj) += part[0][t] + part[1][t] + ... in slice order; one thread per entry, grid (tiles, 16, elements): element b =
// blockIdx.z on part + b pstride and G + b gstride
__global__ __launch_bounds__(256) void sparse_gram_reduce_kernel(const double *__restrict__ part, int64_t pstride, int ntiles, int nslices,
                                                                 double *__restrict__ G, int64_t ldg, int64_t gstride)
{
    const int t = blockIdx.x;
    part += (int64_t)blockIdx.z * pstride;
    G += (int64_t)blockIdx.z * gstride;
    int ti, tj;
    sparse_tile_of(t, &ti, &tj);
    const int e = blockIdx.y * 256 + threadIdx.x;          // element of the tile, row-major
    const int64_t gi = (int64_t)ti * 64 + (e >> 6), gj = (int64_t)tj * 64 + (e & 63);
    double v = G[gi * ldg + gj];
    for (int s = 0; s < nslices; s++) v += part[((int64_t)s * ntiles + t) * 4096 + e];
    G[gi * ldg + gj] = v;
}

// G_b (mg x mg, mg a multiple of 64, row stride ldg, elements gstride apart; lower tiles) += V_b^T V_b (A == NULL) or A^T V (one
// element) over the `rows` rows of V_b = V + b vstride and A (row stride ldv >= mg).  nslices workgroups share a tile (chosen by the
// caller: api_sparse.inc sparse_slices) in the partition sparse_gram_slicing gives for (rows, nslices) -- not a function of nbatch;
// part holds nbatch x pstride doubles, pstride >= sparse_gram_part_doubles(mg, nslices).  Both launchers: the checks, the partition,
// the grids; `batch` says whose instantiation runs (the batch keeps its own at nbatch = 1 too).
static int sparse_gram_launch(hipStream_t st, const char *who, bool batch, int64_t nbatch, const double *A, const double *V, int64_t ldv,
                              int64_t vstride, int64_t rows, int64_t mg, int nslices, double *part, int64_t pstride, double *G, int64_t ldg,
                              int64_t gstride)
{
    if (rows <= 0 || nbatch <= 0) return GPT_OK;
    if (mg <= 0 || mg % 64 || mg > ldv || mg > ldg || nslices < 1 || nslices > 65535 || mg / 64 > 2000 || nbatch > 65535 ||
        (!batch && nbatch != 1) || (A && batch) || vstride < rows * ldv || gstride < mg * ldg || pstride < sparse_gram_part_doubles(mg, nslices)) {
        gpt_set_error("%s: order %lld (a multiple of 64, at most the row strides %lld / %lld), %d slices, %lld elements %lld / %lld / %lld apart",
                      who, (long long)mg, (long long)ldv, (long long)ldg, nslices, (long long)nbatch, (long long)vstride, (long long)pstride,
                      (long long)gstride);
        return GPT_E_ARG;
    }
    const int ntiles = (int)sparse_gram_tiles(mg);
    const SparseSlicing sl = sparse_gram_slicing(rows, nslices);
    const dim3 grid((unsigned)ntiles, (unsigned)sl.ns, (unsigned)nbatch);
    auto kernel = A ? sparse_gram_kernel<true, false> : batch ? sparse_gram_kernel<false, true> : sparse_gram_kernel<false, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, A, V, ldv, rows, sl.slice_rows, ntiles, part, vstride, pstride);
    GPT_LAUNCH_CHECK();
    hipLaunchKernelGGL(sparse_gram_reduce_kernel, dim3((unsigned)ntiles, 16, (unsigned)nbatch), dim3(256), 0, st, part, pstride, ntiles, sl.ns, G,
                       ldg, gstride);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_sparse_gram(hipStream_t st, const double *A, const double *V, int64_t ldv, int64_t rows, int64_t mg, int nslices, double *part,
                       double *G, int64_t ldg)
{
    return sparse_gram_launch(st, A ? "sparse_gram2" : "sparse_gram", false, 1, A, V, ldv, rows * ldv, rows, mg, nslices, part,
                              sparse_gram_part_doubles(mg, nslices), G, ldg, mg * ldg);
}

int launch_sparse_gram_batch(hipStream_t st, int64_t nbatch, const double *V, int64_t ldv, int64_t vstride, int64_t rows, int64_t mg, int nslices,
                             double *part, int64_t pstride, double *G, int64_t ldg, int64_t gstride)
{
    return sparse_gram_launch(st, "sparse_gram_batch", true, nbatch, nullptr, V, ldv, vstride, rows, mg, nslices, part, pstride, G, ldg, gstride);
}

// ---- B = I + G with the augmented row ------------------------------------------------------------------------------------------------
// B (bp x bp, row stride bp; bp a multiple of 128, > M): rows / columns < M: I + G (lower; the upper triangle is zeroed); row M: b^T =
// G[M][0..M) with `big` on the diagonal (the pivot stays positive whatever c.c is: solve.hip fill_pad_kernel); rows > M: unit diagonal.
// Grid (columns / 256, rows, elements): element b = blockIdx.z on G + b gstride and B + b bstride.
__global__ void sparse_assemble_b_kernel(const double *__restrict__ G, int64_t ldg, int64_t gstride, int64_t M, double *__restrict__ B, int64_t bp,
                                         int64_t bstride, double big)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= bp) return;
    G += (int64_t)blockIdx.z * gstride;
    B += (int64_t)blockIdx.z * bstride;
    double v = 0.0;
    if (i < M) {
        if (j <= i) v = G[i * ldg + j] + (i == j ? 1.0 : 0.0);
    } else if (i == M) {
        v = (j < M) ? G[i * ldg + j] : (j == M ? big : 0.0);
    } else if (i == j) {
        v = 1.0;
    }
    B[i * bp + j] = v;
}

static int sparse_assemble_b_launch(hipStream_t st, const char *who, int64_t nbatch, const double *G, int64_t ldg, int64_t gstride, int64_t M,
                                    double *B, int64_t bp, int64_t bstride, double big)
{
    if (nbatch <= 0) return GPT_OK;
    if (M < 1 || bp <= M || ldg <= M || bp > 65535 || nbatch > 65535 || gstride < (M + 1) * ldg || bstride < bp * bp) {
        gpt_set_error("%s: M = %lld, padded order %lld, %lld elements %lld / %lld apart", who, (long long)M, (long long)bp, (long long)nbatch,
                      (long long)gstride, (long long)bstride);
        return GPT_E_ARG;
    }
    hipLaunchKernelGGL(sparse_assemble_b_kernel, dim3((unsigned)((bp + 255) / 256), (unsigned)bp, (unsigned)nbatch), dim3(256), 0, st, G, ldg,
                       gstride, M, B, bp, bstride, big);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_sparse_assemble_b(hipStream_t st, const double *G, int64_t ldg, int64_t M, double *B, int64_t bp, double big)
{
    return sparse_assemble_b_launch(st, "sparse_assemble_b", 1, G, ldg, (M + 1) * ldg, M, B, bp, bp * bp, big);
}

int launch_sparse_assemble_b_batch(hipStream_t st, int64_t nbatch, const double *G, int64_t ldg, int64_t gstride, int64_t M, double *B, int64_t bp,
                                   int64_t bstride, double big)
{
    return sparse_assemble_b_launch(st, "sparse_assemble_b_batch", nbatch, G, ldg, gstride, M, B, bp, bstride, big);
}

// ---- predictive variance ---------------------------------------------------------------------------------------------------------------
// var[i] = kdiag[i] - sum_{j < M} V[i][j]^2 + sum_{j < M} W[i][j]^2: one workgroup per test row, a fixed order
__global__ __launch_bounds__(256) void sparse_var_kernel(const double *__restrict__ V, const double *__restrict__ W, int64_t ld,
                                                         int64_t rows, int64_t M, const double *__restrict__ kdiag,
                                                         double *__restrict__ var)
{
    __shared__ double pv[4], pw[4];
    const int64_t i = blockIdx.x;
    if (i >= rows) return;
    const double *v = V + i * ld, *w = W + i * ld;
    double a = 0.0, b = 0.0;
    for (int64_t c = threadIdx.x; c < M; c += 256) {
        a = fma(v[c], v[c], a);
        b = fma(w[c], w[c], b);
    }
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    if ((threadIdx.x & 63) == 0) {
        pv[threadIdx.x >> 6] = a;
        pw[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        var[i] = (kdiag[i] - ((pv[0] + pv[1]) + (pv[2] + pv[3]))) + ((pw[0] + pw[1]) + (pw[2] + pw[3]));
}

int launch_sparse_var(hipStream_t st, const double *V, const double *W, int64_t ld, int64_t rows, int64_t M, const double *kdiag,
                      double *var)
{
    if (rows <= 0) return GPT_OK;
    hipLaunchKernelGGL(sparse_var_kernel, dim3((unsigned)rows), dim3(256), 0, st, V, W, ld, rows, M, kdiag, var);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// ---- the gradient of the objective (gpt_sparse_grad_diff, api_sparse_grad.inc) -----------------------------------------
// Per-row pass of the gradient's second sweep over the chunks.  Row i of V holds v_i^T = (L_u^-1 k(Z, x_i))^T, row i of W holds
// w_i^T = (L_B^-1 v_i)^T (columns < M of either); t = L_B^-T c.  With s_i = noise_var + err_i^2 and Lambda_i as in the fit:
//     q_i = |v_i|^2      alpha_i = (r_i - v_i.t) / Lambda_i      W_ii = alpha_i^2 - 1 / Lambda_i + |w_i|^2 / Lambda_i^2
//     e_i = W_ii (fitc), -1 / s_i (vfe), 0 (dtc)                 g_i = W_ii / 2 (+ (k_i - q_i) / (2 s_i^2) for vfe)
// Written: alpha[i], e[i], gval[i] = g_i (gval[ldr + i] = 0: the layout sparse_rowsum_kernel adds up in a fixed order), and the two
// scaled copies of the row, S1[i] = v_i / Lambda_i and S2[i] = e_i v_i, columns [M, ld) zero -- the operands of the chunk's GEMMs and
// of the signed Gram.  q_i and Lambda_i come from the functions sparse_lambda_kernel forms them with (sparse_row_sumsq,
// sparse_lambda_of; kmq is 0 for dtc, whose k_i nobody writes): a row the fit accepted has the same Lambda_i here.  A row whose Lambda_i
// is not a positive finite number raises *bad and contributes nothing (alpha, e, g and both copies are zero).
__global__ __launch_bounds__(256) void sparse_grad_rows_kernel(const double *__restrict__ V, const double *__restrict__ W, int64_t ld,
                                                               int64_t rows, int64_t M, int method, const double *__restrict__ kdiag,
                                                               const double *__restrict__ r, const double *__restrict__ err,
                                                               double noise_var, const double *__restrict__ t,
                                                               double *__restrict__ alpha, double *__restrict__ e_out,
                                                               double *__restrict__ gval, int64_t ldr, double *__restrict__ S1,
                                                               double *__restrict__ S2, int32_t *__restrict__ bad)
{
    __shared__ double pq[4], pt[4], pw[4];
    __shared__ double sc1, sc2;
    const int64_t i = blockIdx.x;
    if (i >= rows) return;
    const double *v = V + i * ld, *w = W + i * ld;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = sparse_row_sumsq(v, M), bt = 0.0, bw = 0.0;
    for (int64_t c = threadIdx.x; c < M; c += 256) {
        bt = fma(v[c], t[c], bt);
        bw = fma(w[c], w[c], bw);
    }
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off);
        bt += __shfl_down(bt, off);
        bw += __shfl_down(bw, off);
    }
    if (lane == 0) {
        pq[wave] = acc;
        pt[wave] = bt;
        pw[wave] = bw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double q = (pq[0] + pq[1]) + (pq[2] + pq[3]), vt = (pt[0] + pt[1]) + (pt[2] + pt[3]), ww = (pw[0] + pw[1]) + (pw[2] + pw[3]);
        const double er = err[i], s = noise_var + er * er, kmq = (method == 2) ? 0.0 : kdiag[i] - q;
        const SparseLambda L = sparse_lambda_of(method == 0, kmq, s);
        const double lam = L.lam;
        const bool ok = L.ok;
        if (!ok) *bad = 1;
        const double il = ok ? 1.0 / lam : 0.0;
        const double al = ok ? (r[i] - vt) * il : 0.0;
        const double wii = (al * al - il) + ww * il * il;
        const double e = !ok ? 0.0 : (method == 0) ? wii : (method == 1) ? -1.0 / s : 0.0;
        double g = 0.5 * wii;
        if (method == 1) g += 0.5 * kmq / (s * s);
        alpha[i] = al;
        e_out[i] = e;
        gval[i] = ok ? g : 0.0;
        gval[ldr + i] = 0.0;
        sc1 = il;
        sc2 = e;
    }
    __syncthreads();
    const double s1 = sc1, s2 = sc2;
    double *o1 = S1 + i * ld, *o2 = S2 + i * ld;
    for (int64_t c = threadIdx.x; c < ld; c += 256) {
        const double vc = (c < M) ? v[c] : 0.0;
        o1[c] = vc * s1;
        o2[c] = vc * s2;
    }
}

int launch_sparse_grad_rows(hipStream_t st, const double *V, const double *W, int64_t ld, int64_t rows, int64_t M, int method,
                            const double *kdiag, const double *r, const double *err, double noise_var, const double *t, double *alpha,
                            double *e_out, double *gval, int64_t ldr, double *S1, double *S2, int32_t *bad)
{
    if (rows <= 0) return GPT_OK;
    if (M < 1 || M > ld || rows > ldr) {
        gpt_set_error("sparse_grad_rows: M = %lld in rows of %lld, %lld rows with a value stride of %lld", (long long)M, (long long)ld,
                      (long long)rows, (long long)ldr);
        return GPT_E_ARG;
    }
    hipLaunchKernelGGL(sparse_grad_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st, V, W, ld, rows, M, method, kdiag, r, err, noise_var,
                       t, alpha, e_out, gval, ldr, S1, S2, bad);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// A[i][m] += alpha[i] * beta[m], i < rows, m < M: the rank-one part of a chunk's A_fu
__global__ __launch_bounds__(256) void sparse_rank1_kernel(double *__restrict__ A, int64_t lda, int64_t rows, int64_t M,
                                                           const double *__restrict__ alpha, const double *__restrict__ beta)
{
    const int64_t m = (int64_t)blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
    if (m < M && i < rows) A[i * lda + m] = fma(alpha[i], beta[m], A[i * lda + m]);
}

int launch_sparse_rank1(hipStream_t st, double *A, int64_t lda, int64_t rows, int64_t M, const double *alpha, const double *beta)
{
    if (rows <= 0 || M <= 0) return GPT_OK;
    if (M > lda || (M + 255) / 256 > 65535) return GPT_E_ARG;
    hipLaunchKernelGGL(sparse_rank1_kernel, dim3((unsigned)rows, (unsigned)((M + 255) / 256)), dim3(256), 0, st, A, lda, rows, M, alpha, beta);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// dst (np x np, row stride ldd) = the lower triangle of src's leading n x n block, zeros elsewhere: L_B without its augmented rows
__global__ void sparse_tril_kernel(const double *__restrict__ src, int64_t lds, int64_t n, double *__restrict__ dst, int64_t ldd, int64_t np)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= np) return;
    dst[i * ldd + j] = (i < n && j <= i) ? src[i * lds + j] : 0.0;
}

int launch_sparse_tril(hipStream_t st, const double *src, int64_t lds, int64_t n, double *dst, int64_t ldd, int64_t np)
{
    if (n < 1 || np < n || np > 65535 || ldd < np) return GPT_E_ARG;
    hipLaunchKernelGGL(sparse_tril_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, st, src, lds, n, dst, ldd, np);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// Mid (np x np, symmetric, both triangles) = I - Binv + E over the leading M x M block, zeros elsewhere.  mode 0 (fitc): E = the lower
// tiles of the signed Gram V diag(e) V^T (entry (i, j) read at (max, min)); mode 1 (vfe): E = -(B - I), B given whole; mode 2 (dtc): 0.
__global__ void sparse_grad_mid_kernel(const double *__restrict__ Binv, int64_t ldb, const double *__restrict__ E, int64_t lde, int64_t M,
                                       int mode, double *__restrict__ Mid, int64_t np)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= np) return;
    double v = 0.0;
    if (i < M && j < M) {
        const double id = (i == j) ? 1.0 : 0.0;
        const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
        v = id - Binv[hi * ldb + lo];
        if (mode == 0) v += E[hi * lde + lo];
        else if (mode == 1) v -= E[hi * lde + lo] - id;
    }
    Mid[i * np + j] = v;
}

int launch_sparse_grad_mid(hipStream_t st, const double *Binv, int64_t ldb, const double *E, int64_t lde, int64_t M, int mode, double *Mid,
                           int64_t np)
{
    if (M < 1 || np < M || np > 65535 || (mode != 2 && !E)) return GPT_E_ARG;
    hipLaunchKernelGGL(sparse_grad_mid_kernel, dim3((unsigned)((np + 255) / 256), (unsigned)np), dim3(256), 0, st, Binv, ldb, E, lde, M, mode,
                       Mid, np);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// dst (M x M, row stride ldd, both triangles) = S - beta beta^T = 2 A_uu, S given in its lower triangle (entry (i, j) read at (max, min)):
// the weights of the Z-Z pass of gpt_sparse_grad_z (kgrad_dz.hip)
__global__ void sparse_auu2_kernel(const double *__restrict__ S, int64_t lds, int64_t M, const double *__restrict__ beta,
                                   double *__restrict__ dst, int64_t ldd)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= M) return;
    const int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    dst[i * ldd + j] = S[hi * lds + lo] - beta[i] * beta[j];
}

int launch_sparse_auu2(hipStream_t st, const double *S, int64_t lds, int64_t M, const double *beta, double *dst, int64_t ldd)
{
    if (M < 1 || M > 65535 || lds < M || ldd < M || !S || !beta || !dst) {
        gpt_set_error("sparse_auu2: bad arguments (M=%lld, row strides %lld and %lld)", (long long)M, (long long)lds, (long long)ldd);
        return GPT_E_ARG;
    }
    hipLaunchKernelGGL(sparse_auu2_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)M), dim3(256), 0, st, S, lds, M, beta, dst, ldd);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// ---- batched fits (gpt_sparse_fit_batch, api_sparse_batch.inc) ----------------------------------------------------------
// The fit's four kernel groups carry the element of a batch in a grid dimension -- element b on its own chunk buffer V + b vstride, its
// own k(x_i, x_i), residual, per-row values, running sums, partial tiles, G and B -- and each is the single fit's source, above: the row
// pass one inlined body under two kernels (noise_var by value / noise_var[b]), the Gram the BATCH flag of sparse_gram_kernel, the
// running sums, the Gram's reduce and the assembly one plain kernel each that the single launchers run with one element.  An element
// therefore carries the bits it has alone; what a batch adds is strides.  Only the kernel below has no single twin here.

// A_b[i][i] = 1 for i in [n_valid, n_pad) of every element: the unit padding diagonal of the batch's K_uu + jitter I (the rows are zero
// already), what launch_fill_pad leaves in the single fit's
__global__ void sparse_unit_pad_batch_kernel(double *__restrict__ A, int64_t lda, int64_t bstride, int64_t n_valid, int64_t n_pad)
{
    const int64_t i = n_valid + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pad) A[(int64_t)blockIdx.y * bstride + i * lda + i] = 1.0;
}

int launch_sparse_unit_pad_batch(hipStream_t st, int64_t nbatch, double *A, int64_t lda, int64_t bstride, int64_t n_valid, int64_t n_pad)
{
    if (n_pad <= n_valid || nbatch <= 0) return GPT_OK;
    if (n_valid < 0 || n_pad > lda || bstride < n_pad * lda || nbatch > 65535) return GPT_E_ARG;
    hipLaunchKernelGGL(sparse_unit_pad_batch_kernel, dim3((unsigned)((n_pad - n_valid + 127) / 128), (unsigned)nbatch), dim3(128), 0, st, A, lda,
                       bstride, n_valid, n_pad);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
