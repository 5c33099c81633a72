// kgreedy.hip -- greedy conditional-variance selection of inducing inputs: the partial pivoted Cholesky of K_ff, gfx950 (DESIGN.md
// section 18.10; gpt_sparse_select_inducing, api_sparse_select.inc).
//
// The factor L is COLUMN-major: ld = the candidates rounded up to 64, column t at L + t * ld.  Step j, three launches:
//   greedy_pick_kernel    one workgroup: reduces the per-workgroup partials the previous launch left -- (largest residual, lowest row
//                         at that value, sum of max(residual, 0)) -- writes trace[j], applies the stop rule, writes idx[j] and dmax[j],
//                         marks the pivot p, gathers x_p into a staging point and row p of L, columns [0, j), into a staging vector;
//   the builder           k(x_p, x_i) for every candidate i into column j of L (the model's own pair functions; api_sparse_select.inc);
//   greedy_update_kernel  the hot path, one thread per candidate row i: s_i = sum_{t < j} L[i,t] L[p,t], l_i = (L[i,j] - s_i) / sqrt(dmax),
//                         L[i,j] = l_i, d_i -= l_i^2, and the workgroup's partial for the next pick.
// Nothing returns to the host between the steps: the pivot and dmax live in device memory (GPT_GREEDY_S_* / GPT_GREEDY_W_*, gpt_hip.h), and once the
// stop rule has raised words[GPT_GREEDY_W_STOP] both kernels return before they read or write anything else.
//
// Determinism: no floating-point atomics and no "last workgroup" counters -- a workgroup writes ONE partial, the next launch (a launch of
// its own) reduces them; every sum has the fixed order stated at its place; (value, row) pairs are compared by "larger value, at equal
// values (equal as doubles) the lower row", which is associative and commutative, so its order does not matter.
#include "common.hpp"

// The inner product s_i runs in GREEDY_UNROLL independent chains: chain u takes the columns t = u, u + GREEDY_UNROLL, ... in ascending
// order (fma), and the chains are joined pairwise, ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)) and so on up the tree.  Per wave
// and column the load is one contiguous 512-byte segment; GREEDY_UNROLL of them are in flight per wave before the first is used:
// 16 waves per CU hold 128 KiB in flight, four waves (N = 65536 over 256 CUs) 32 KiB -- the kernel is bound by reading 8 N j bytes.
static_assert(GREEDY_UNROLL == 16, "the join below is written for 16 chains");

// (value, row): a is better than b
__device__ __forceinline__ bool greedy_better(double va, int32_t ia, double vb, int32_t ib) { return va > vb || (va == vb && ia < ib); }

// This thread's (bv, bi, bs) -> the workgroup's in thread 0.  Within a wave by shuffles, lane l takes lane l + off for off = 32, 16, ..,
// 1 (the sums in that order); the four waves in LDS, ((w0 + w1) + w2) + w3.
__device__ __forceinline__ void greedy_wg_reduce(double &bv, int32_t &bi, double &bs)
{
    __shared__ double sv[GREEDY_WG / 64], ss[GREEDY_WG / 64];
    __shared__ int32_t si[GREEDY_WG / 64];
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off), os = __shfl_down(bs, off);
        const int32_t oi = __shfl_down(bi, off);
        bs += os;
        if (greedy_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        sv[wave] = bv;
        si[wave] = bi;
        ss[wave] = bs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < GREEDY_WG / 64; w++) {
            bs += ss[w];
            if (greedy_better(sv[w], si[w], bv, bi)) {
                bv = sv[w];
                bi = si[w];
            }
        }
    }
}

// Workgroup b's partial: part[b] the largest residual among its unselected rows (-inf: none), pidx[b] the lowest row at that value
// (INT32_MAX: none), part[nparts + b] the sum
__device__ __forceinline__ void greedy_write_partial(double bv, int32_t bi, double bs, double *__restrict__ part, int32_t *__restrict__ pidx,
                                                     int64_t nparts)
{
    greedy_wg_reduce(bv, bi, bs);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = bv;
        part[nparts + blockIdx.x] = bs;
        pidx[blockIdx.x] = bi;
    }
}

// Before step 0: nothing is selected, the residuals are k(x_i, x_i) as the pair pass left them; trace_0 is their plain sum
__global__ __launch_bounds__(GREEDY_WG) void greedy_init_kernel(int64_t rows, const double *__restrict__ resid, int32_t *__restrict__ mark,
                                                                double *__restrict__ part, int32_t *__restrict__ pidx, int64_t nparts)
{
    const int64_t i = (int64_t)blockIdx.x * GREEDY_WG + threadIdx.x;
    double bv = -INFINITY, bs = 0.0;
    int32_t bi = INT32_MAX;
    if (i < rows) {
        mark[i] = 0;
        bv = bs = resid[i];
        bi = (int32_t)i;
    }
    greedy_write_partial(bv, bi, bs, part, pidx, nparts);
}

// Step j of the factorisation for every row: L (columns [0, j) read, never written), col = column j (in: k(x_i, x_p); out: l_i), prow[t] =
// L[p, t].  l_i is a DIVISION by the correctly rounded sqrt(dmax), not a multiplication by a reciprocal: with dmax a power of four the
// scaling is exact.  d_i - l_i^2 is a rounded product and a subtraction (the library is compiled without contraction).  Rows >= rows
// are neither read nor written; selected rows (mark != 0) are updated like every row and contribute nothing to the partial.
__global__ __launch_bounds__(GREEDY_WG) __attribute__((amdgpu_waves_per_eu(1, 4))) void greedy_update_kernel(const double *__restrict__ L, int64_t ld, int64_t rows, int64_t j,
                                                                  double *__restrict__ col, double *__restrict__ resid,
                                                                  const int32_t *__restrict__ mark, const double *__restrict__ prow,
                                                                  const double *__restrict__ scal, const int32_t *__restrict__ words,
                                                                  double *__restrict__ part, int32_t *__restrict__ pidx, int64_t nparts)
{
    if (words[GPT_GREEDY_W_STOP] != 0) return;
    const int64_t i = (int64_t)blockIdx.x * GREEDY_WG + threadIdx.x;
    double bv = -INFINITY, bs = 0.0;
    int32_t bi = INT32_MAX;
    if (i < rows) {
        const double *Li = L + i;
        double acc[GREEDY_UNROLL];
#pragma unroll
        for (int u = 0; u < GREEDY_UNROLL; u++) acc[u] = 0.0;
        int64_t t = 0;
        for (; t + GREEDY_UNROLL <= j; t += GREEDY_UNROLL) {
            double v[GREEDY_UNROLL];
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; u++) v[u] = Li[(t + u) * ld];
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; u++) acc[u] = fma(v[u], prow[t + u], acc[u]);      // (prow: a uniform address)
        }
        if (t < j) {      // the last, partial group: every load is issued (the columns past j - 1 read column j - 1 again and are dropped)
            double v[GREEDY_UNROLL];
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; u++) v[u] = Li[((t + u < j) ? t + u : j - 1) * ld];
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; u++) acc[u] = (t + u < j) ? fma(v[u], prow[(t + u < j) ? t + u : j - 1], acc[u]) : acc[u];
        }
#pragma unroll
        for (int w = 1; w < GREEDY_UNROLL; w *= 2)
#pragma unroll
            for (int u = 0; u < GREEDY_UNROLL; u += 2 * w) acc[u] = acc[u] + acc[u + w];
        const double l = (col[i] - acc[0]) / sqrt(scal[GPT_GREEDY_S_DMAX]);
        col[i] = l;
        const double d = resid[i] - l * l;
        resid[i] = d;
        if (mark[i] == 0) {
            bv = d;
            bs = fmax(d, 0.0);
            bi = (int32_t)i;
        }
    }
    greedy_write_partial(bv, bi, bs, part, pidx, nparts);
}

// The pick of step j (one workgroup).  Partial q is read by thread q % GREEDY_WG, a thread adds its partials' sums in ascending q, then
// greedy_wg_reduce.  trace[j] is written first -- it belongs to the steps done so far -- and with j == M nothing else happens (the
// closing launch).  Stop (words[GPT_GREEDY_W_STOP] = 1, words[GPT_GREEDY_W_COUNT] = j): dmax is not a positive finite number (at j = 0 also
// words[GPT_GREEDY_W_BAD] = 1), or j > 0 and dmax <= tol * dmax_0.  Otherwise idx[j] = cand[p] (cand NULL: p), dmax[j], mark[p] = 1,
// scal[GPT_GREEDY_S_DMAX] = dmax (at j = 0 scal[GPT_GREEDY_S_DMAX0] too), words[GPT_GREEDY_W_PIVOT] = p, words[GPT_GREEDY_W_COUNT] = j + 1,
// xp[0 .. D) = X[p], prow[t] = L[p + t * ld] for t < j.
__global__ __launch_bounds__(GREEDY_WG) void greedy_pick_kernel(int64_t j, int64_t M, double tol, const double *__restrict__ part,
                                                                const int32_t *__restrict__ pidx, int64_t nparts,
                                                                const int32_t *__restrict__ cand, const double *__restrict__ X, int D,
                                                                const double *__restrict__ L, int64_t ld, int32_t *__restrict__ mark,
                                                                double *__restrict__ scal, int32_t *__restrict__ words,
                                                                int32_t *__restrict__ idx, double *__restrict__ dmax, double *__restrict__ trace,
                                                                double *__restrict__ xp, double *__restrict__ prow)
{
    __shared__ int32_t sh_p;
    if (words[GPT_GREEDY_W_STOP] != 0) return;
    double bv = -INFINITY, bs = 0.0;
    int32_t bi = INT32_MAX;
    for (int64_t q = threadIdx.x; q < nparts; q += GREEDY_WG) {
        bs += part[nparts + q];
        if (greedy_better(part[q], pidx[q], bv, bi)) {
            bv = part[q];
            bi = pidx[q];
        }
    }
    greedy_wg_reduce(bv, bi, bs);
    if (threadIdx.x == 0) {
        int32_t p = -1;
        trace[j] = bs;
        if (j < M) {
            bool go = bv > 0.0 && bv < INFINITY;
            if (go && j > 0 && bv <= tol * scal[GPT_GREEDY_S_DMAX0]) go = false;
            if (go) {
                p = bi;
                idx[j] = cand ? cand[p] : p;
                dmax[j] = bv;
                mark[p] = 1;
                scal[GPT_GREEDY_S_DMAX] = bv;
                if (j == 0) scal[GPT_GREEDY_S_DMAX0] = bv;
                words[GPT_GREEDY_W_PIVOT] = p;
                words[GPT_GREEDY_W_COUNT] = (int32_t)(j + 1);
            } else {
                words[GPT_GREEDY_W_COUNT] = (int32_t)j;
                if (j == 0) words[GPT_GREEDY_W_BAD] = 1;
                words[GPT_GREEDY_W_STOP] = 1;
            }
        }
        sh_p = p;
    }
    __syncthreads();
    const int64_t p = sh_p;
    if (p < 0) return;
    if ((int)threadIdx.x < D) xp[threadIdx.x] = X[p * D + threadIdx.x];
    for (int64_t t = threadIdx.x; t < j; t += GREEDY_WG) prow[t] = L[p + t * ld];
}

// Xc[r] = X[cand[r]], nc[r] = 0: the candidates as a point set of their own
__global__ __launch_bounds__(256) void greedy_gather_kernel(const double *__restrict__ X, const int32_t *__restrict__ cand, int64_t ncand, int D,
                                                            double *__restrict__ Xc, int32_t *__restrict__ nc)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ncand * D) return;
    const int64_t r = e / D;
    Xc[e] = X[(int64_t)cand[r] * D + (e - r * D)];
    nc[e] = 0;
}

int64_t greedy_blocks(int64_t rows) { return (rows + GREEDY_WG - 1) / GREEDY_WG; }

static int greedy_rows_ok(const char *who, int64_t rows, int64_t ld)
{
    if (rows < 1 || rows > ld || rows > INT32_MAX - 1) {
        gpt_set_error("%s: %lld rows in a factor of column stride %lld", who, (long long)rows, (long long)ld);
        return GPT_E_ARG;
    }
    return GPT_OK;
}

int launch_greedy_init(hipStream_t st, int64_t rows, const double *resid, int32_t *mark, double *part, int32_t *pidx)
{
    if (int rc = greedy_rows_ok("greedy_init", rows, rows)) return rc;
    const int64_t nb = greedy_blocks(rows);
    hipLaunchKernelGGL(greedy_init_kernel, dim3((unsigned)nb), dim3(GREEDY_WG), 0, st, rows, resid, mark, part, pidx, nb);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_greedy_update(hipStream_t st, const double *L, int64_t ld, int64_t rows, int64_t j, double *col, double *resid, const int32_t *mark,
                         const double *prow, const double *scal, const int32_t *words, double *part, int32_t *pidx)
{
    if (int rc = greedy_rows_ok("greedy_update", rows, ld)) return rc;
    if (j < 0) return GPT_E_ARG;
    const int64_t nb = greedy_blocks(rows);
    hipLaunchKernelGGL(greedy_update_kernel, dim3((unsigned)nb), dim3(GREEDY_WG), 0, st, L, ld, rows, j, col, resid, mark, prow, scal, words, part,
                       pidx, nb);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_greedy_pick(hipStream_t st, int64_t j, int64_t M, double tol, const double *part, const int32_t *pidx, int64_t nparts,
                       const int32_t *cand, const double *X, int D, const double *L, int64_t ld, int32_t *mark, double *scal, int32_t *words,
                       int32_t *idx, double *dmax, double *trace, double *xp, double *prow)
{
    if (j < 0 || j > M || nparts < 1 || D < 1 || D > GPT_MAX_DIM || !(tol >= 0.0)) {
        gpt_set_error("greedy_pick: step %lld of %lld, %lld partials, num_dim %d, tol %g", (long long)j, (long long)M, (long long)nparts, D, tol);
        return GPT_E_ARG;
    }
    hipLaunchKernelGGL(greedy_pick_kernel, dim3(1), dim3(GREEDY_WG), 0, st, j, M, tol, part, pidx, nparts, cand, X, D, L, ld, mark, scal, words, idx,
                       dmax, trace, xp, prow);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

int launch_greedy_gather(hipStream_t st, const double *X, const int32_t *cand, int64_t ncand, int D, double *Xc, int32_t *nc)
{
    if (ncand < 1) return GPT_OK;
    hipLaunchKernelGGL(greedy_gather_kernel, dim3((unsigned)((ncand * D + 255) / 256)), dim3(256), 0, st, X, cand, ncand, D, Xc, nc);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}
