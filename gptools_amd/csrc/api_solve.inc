// api_solve.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Many-right-hand-side solves against the resident factor: block inverses, right-TRSM by GEMMs, split-k; pinned host buffers.
// ------------------------------------------------------------------------------------------------
// solves with many right-hand sides against the resident factor: 512-column leaves by explicit block inverses
// ------------------------------------------------------------------------------------------------
// B (m x n) <- B L^-T is a chain of n/128 (leaf TRSM + update) pairs, ~20 us each: 2.5 ms at N = 8192 however few rows B
// has (predict at a handful of points, gpt_solve_L).  With W_j = L_jj^-1 of the 512x512 diagonal blocks at hand (built
// once per factorisation, on first use: 10 launches per block) a leaf is one copy and one GEMM, B_j <- B_j W_j^T, and
// the chain has a quarter of the links: predict with std at M <= 256, N = 8192 goes from 2.55 to ~0.7 ms once the
// inverses exist.
// W (nfull x nb, block j at row j): the inverses of the nb x nb diagonal blocks of the resident factor, built on first
// use after a factorisation (identity pushed through the panel TRSM, transposed).  nb = 512 for every solve, and
// additionally nb = 1024 for solves with at most GPT_FEW_ROWS rows, whose time is the LENGTH of the chain of dependent
// GEMMs (two per block), not their flops.
#define GPT_FEW_ROWS 128
__global__ void eye_strip_kernel(double *__restrict__ U, int64_t n, int64_t w)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) U[i * w + i % w] = 1.0;
}

// W_b (w x w) = U_b^T for every block b of a strip (blockIdx.z), through a 32x33 LDS tile
__global__ __launch_bounds__(256) void transpose_strip_kernel(const double *__restrict__ U, double *__restrict__ W, int64_t w)
{
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32, o = (int64_t)blockIdx.z * w * w;
    for (int i = ty; i < 32; i += 8) t[i][tx] = U[o + (r0 + i) * w + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8) W[o + (c0 + i) * w + r0 + tx] = t[tx][i];
}

// The inverses of ALL 512 x 512 diagonal blocks of the resident factor at once: U (strip, block j at rows [512 j, 512 j + 512),
// row stride 512) = L_jj^-T, W = L_jj^-1 = its transpose.  The recursion of trtri_u -- leaves by the panel TRSM on the identity,
// U12 = -(U11 L21^T) L22^-T per level -- with every launch BATCHED over the blocks (blockIdx.y; the three operands of the
// GEMMs lie in three arrays with a stride each): 2 + 4 + 4 + 4 + 1 = 15 launches whatever the order, where the per-block
// loop of round 3 needed 10 per block (N = 8192: 160 launches, ~1.3 ms before the first predict / gradient / alpha).
// (Rounds 2-4's builder: since round 5 only behind option binv_launches = 1 -- the default is ONE launch, solve.hip trinv512_kernel,
// 205 -> 59 us at N = 8192 -- kept as the same-process A/B baseline and as a second implementation for the tests.)
static int build_block_inverses_512(gpt_ctx *c, hipStream_t st, int64_t nblk, double *U, double *W)
{
    const int64_t nb = 512, bs = nb * nb, NP = c->NP, bsl = nb * (NP + 1), WS = GPT_WS_BLOCK;
    GPT_HIP_CHECK(hipMemsetAsync(U, 0, (size_t)nblk * bs * sizeof(double), st));
    hipLaunchKernelGGL(eye_strip_kernel, dim3((unsigned)((nblk * nb + 255) / 256)), dim3(256), 0, st, U, nblk * nb, nb);
    GPT_LAUNCH_CHECK();
    for (int p = 0; p < 4; p++)                                        // leaves: the identity through the panel TRSM
        GPT_TRY(launch_trsm_panel(st, 128, nullptr, 0, c->d_invd + p * WS, U + (int64_t)p * 128 * nb + p * 128, nb, nullptr, EdgeSig(),
                                  nblk, bs, 4 * WS));
    for (int q = 0; q < 4; q += 2) {                                   // 128 -> 256: the pairs (0, 1) and (2, 3) of every block
        const int64_t lo = q * 128, mid = lo + 128;
        GPT_TRY(launch_gemm_nt(st, 128, 128, 128, -1.0, U + lo * nb + lo, nb, c->dA + mid * NP + lo, NP, 0.0, U + lo * nb + mid, nb, 0,
                               0, 0, nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0, nblk, bs, EdgeSig(), bsl, bs));
        GPT_TRY(launch_trsm_panel(st, 128, nullptr, 0, c->d_invd + (q + 1) * WS, U + lo * nb + mid, nb, nullptr, EdgeSig(), nblk, bs,
                                  4 * WS));
    }
    // 256 -> 512: U12 = -(U11 L21^T), then the right-TRSM against L22 in two 128-column leaves
    GPT_TRY(launch_gemm_nt(st, 256, 256, 256, -1.0, U, nb, c->dA + 256 * NP, NP, 0.0, U + 256, nb, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                           EdgeSig(), 0, nblk, bs, EdgeSig(), bsl, bs));
    GPT_TRY(launch_trsm_panel(st, 256, nullptr, 0, c->d_invd + 2 * WS, U + 256, nb, nullptr, EdgeSig(), nblk, bs, 4 * WS));
    GPT_TRY(launch_gemm_nt(st, 256, 128, 128, -1.0, U + 256, nb, c->dA + 384 * NP + 256, NP, 1.0, U + 384, nb, 0, 0, 0, nullptr, nullptr, 0,
                           EdgeSig(), EdgeSig(), 0, nblk, bs, EdgeSig(), bsl, bs));
    GPT_TRY(launch_trsm_panel(st, 256, nullptr, 0, c->d_invd + 3 * WS, U + 384, nb, nullptr, EdgeSig(), nblk, bs, 4 * WS));
    hipLaunchKernelGGL(transpose_strip_kernel, dim3((unsigned)(nb / 32), (unsigned)(nb / 32), (unsigned)nblk), dim3(256), 0, st, U, W, nb);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

// (ADVICE r3: the inverses are always built for the WHOLE padded order -- floor(NP / nb) blocks -- whatever extent `nfull` the
// caller is going to use: gpt_ll_grad asks for floor(NP / 512) blocks, the solves for floor(round_up(N, 128) / 512), one block
// less at N = 512 k - 128; a strip sized for the smaller request used to be reallocated, and not rebuilt, by the larger one)
static int ensure_block_inverses_wide(gpt_ctx *c, int64_t nb, int64_t nfull, double **out);
static int ensure_block_inverses(gpt_ctx *c, int64_t nb, int64_t nfull, double **out, double **out_u, hipStream_t on)
{
    if (nb == GPT_BINV_NB2) return ensure_block_inverses_wide(c, nb, nfull, out);
    const int64_t nall = (c->NP / nb) * nb;
    if (nfull > nall || nall <= 0) {
        gpt_set_error("block inverses: extent %lld exceeds the padded order %lld", (long long)nfull, (long long)c->NP);
        return GPT_E_ARG;
    }
    double *W, *Us = nullptr;
    GPT_TRY(ensure(c, SLOT_BINV, (size_t)nall * nb * sizeof(double), (void **)&W));
    GPT_TRY(ensure(c, SLOT_BINVU, (size_t)nall * nb * sizeof(double), (void **)&Us));
    *out = W;
    if (out_u) *out_u = Us;
    if (c->binv_valid) return GPT_OK;
    hipStream_t st = on ? on : c->stream;
    if (c->binv_launches) {
        GPT_TRY(build_block_inverses_512(c, st, nall / nb, Us, W));
    } else {
        // one launch (solve.hip) -- of the blocks that were not built under the last panel (enqueue_early_block_inverses)
        // (the late blocks first, THEN the wait for the early ones: they are disjoint pieces of the strips, and the early launch
        // -- on the main stream, under the last panel -- may still be running when the factorisation ends)
        const int64_t b0 = c->binv_early;
        GPT_TRY(launch_trinv512(st, nall / nb - b0, c->dA + b0 * nb * (c->NP + 1), c->NP, c->d_invd + b0 * (nb / 128) * GPT_WS_BLOCK,
                                Us + b0 * nb * nb, W + b0 * nb * nb));
        if (b0 > 0 && c->e_binv_early && st != c->stream) GPT_HIP_CHECK(hipStreamWaitEvent(st, c->e_binv_early, 0));
        c->binv_early = 0;                 // (consumed: belongs to the factorisation that has just ended)
    }
    c->binv_valid = true;
    return GPT_OK;
}

// Eager alpha (option eager_alpha), called by potrf_enqueue when the main stream has issued its last trailing update: the columns
// [0, cols_final) of the factor are final there (the main stream has waited for the panel that ends there), the panel stream still
// has the last panel(s) to factor (~70-100 us at N = 8192) and the main stream is idle: the inverses of the whole 512 x 512 diagonal
// blocks left of the last panel (column `cols`) are built NOW, on the main stream (one trinv512 launch, ~55 us), instead of behind
// the factorisation, where the launch was the first 59 us of alpha's critical path; the blocks right of them follow there (one
// block at N = 8192: 39 us).  Only as many as lie inside [0, cols_final): usually all of them (cols_final == cols), fewer when the
// panel in front of a 128-wide last one is still being factored.  c->binv_early says how many were done here, e_binv_early orders
// other streams behind them.
static int enqueue_early_block_inverses(gpt_ctx *c, hipStream_t S, int64_t cols, int64_t cols_final)
{
    const int64_t nb = GPT_BINV_NB, nall = (c->NP / nb) * nb;
    int64_t b = cols / nb;
    c->binv_early = 0;
    if (c->binv_launches || nall < 2 * nb || b <= 0 || b >= nall / nb) return GPT_OK;
    if (b * nb > cols_final) b = cols_final / nb;
    if (b <= 0) return GPT_OK;
    double *W, *Us = nullptr;
    GPT_TRY(ensure(c, SLOT_BINV, (size_t)nall * nb * sizeof(double), (void **)&W));
    GPT_TRY(ensure(c, SLOT_BINVU, (size_t)nall * nb * sizeof(double), (void **)&Us));
    GPT_TRY(launch_trinv512(S, b, c->dA, c->NP, c->d_invd, Us, W));
    if (!c->e_binv_early) GPT_HIP_CHECK(hipEventCreateWithFlags(&c->e_binv_early, hipEventDisableTiming));
    GPT_HIP_CHECK(hipEventRecord(c->e_binv_early, S));
    c->binv_early = b;
    return GPT_OK;
}

// The 2048 x 2048 diagonal blocks' inverses, for solves with at most GPT_FEW_ROWS rows against a large factor (the chain of
// dependent GEMMs -- two per block -- is what such a solve costs: 4 blocks at N = 8192 instead of 8 or 16).  Built from the
// 512-wide inverses by the GEMM-only triangular inverse of the gradient path (trtri_u_gemm: U = L^-T of the block, N^3/3 flop
// with the block's zeros skipped -- the identity pushed through the panel TRSM would cost 6 x that), then transposed.
#define GPT_BINV_NB3 2048
static int ensure_block_inverses_wide(gpt_ctx *c, int64_t nb, int64_t nfull, double **out)
{
    // (nb = 1024 -- solves with very few rows against factors of 4096 <= n < 8192 -- went through the substitution leaves block
    // by block until round 5: a dozen dependent launches per block)
    const bool w3 = (nb == GPT_BINV_NB3);
    double *W, *U, *T, *Wb;
    if (nfull > (c->NP / nb) * nb) {
        gpt_set_error("block inverses: extent %lld exceeds the padded order %lld", (long long)nfull, (long long)c->NP);
        return GPT_E_ARG;
    }
    nfull = (c->NP / nb) * nb;                                  // (always the whole padded order, see ensure_block_inverses)
    GPT_TRY(ensure(c, w3 ? SLOT_BINV3 : SLOT_BINV2, (size_t)nfull * nb * sizeof(double), (void **)&W));
    *out = W;
    bool &valid = w3 ? c->binv3_valid : c->binv2_valid;
    if (valid) return GPT_OK;
    GPT_TRY(ensure_block_inverses(c, GPT_BINV_NB, nfull, &Wb));
    // U strip (nfull x nb, block J at rows [J nb, J nb + nb)) followed by a strip of the same shape for the products
    GPT_TRY(ensure(c, SLOT_BINV3U, (size_t)2 * nfull * nb * sizeof(double), (void **)&U));
    T = U + nfull * nb;
    hipStream_t st = c->stream;
    GPT_HIP_CHECK(hipMemsetAsync(U, 0, (size_t)nfull * nb * sizeof(double), st));
    const WideBatch wb = {nfull / nb, nb * nb, nb * nb, nb * (c->NP + 1), nb * GPT_BINV_NB};
    GPT_TRY(trtri_u_gemm_b(c, st, 0, nb, Wb, U, nb, T, nb, wb));
    hipLaunchKernelGGL(transpose_rect_kernel, dim3((unsigned)(nb / 32), (unsigned)(nb / 32), (unsigned)wb.n), dim3(256), 0, st, U, nb, W, nb, nb,
                       nb, nb * nb, nb * nb);
    GPT_LAUNCH_CHECK();
    valid = true;
    // (ADVICE r5: the two scratch strips are 2 x NP x nb doubles -- 1 GB at N = 32768 -- and are needed again only after the next
    // factorisation; a large one goes back to the device here.  The build is tens of ms at those sizes, the synchronisation is not
    // what a first predict after a fit waits for.)
    if (c->slots[SLOT_BINV3U].cap > ((size_t)256 << 20)) {
        GPT_HIP_CHECK(hipStreamSynchronize(st));
        DevBuf &b = c->slots[SLOT_BINV3U];
        GPT_HIP_CHECK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    return GPT_OK;
}

// Columns [lo, hi) of V <- the same columns of B L^-T (multiples of nb) by halving; a leaf is ONE out-of-place GEMM against
// the block inverse, V_j = B_j W_j^T, the update in between B[:, mid:hi] -= V[:, lo:mid] L[mid:hi, lo:mid]^T.  B is consumed.
static int trsm_rlt_binv(gpt_ctx *c, hipStream_t st, int64_t m, int64_t nb, int64_t lo, int64_t hi, const double *W, double *B,
                         int64_t ldb, double *V, int64_t ldv)
{
    const int64_t n = hi - lo;
    if (n == nb) return gemm_nt(c, st, m, nb, nb, 1.0, B + lo, ldb, W + lo * nb, nb, 0.0, V + lo, ldv, 0);
    const int64_t h = (n / (2 * nb)) * nb > 0 ? (n / (2 * nb)) * nb : nb;
    const int64_t mid = lo + h;
    GPT_TRY(trsm_rlt_binv(c, st, m, nb, lo, mid, W, B, ldb, V, ldv));
    GPT_TRY(gemm_nt(c, st, m, hi - mid, h, -1.0, V + lo, ldv, c->dA + mid * c->NP + lo, c->NP, 1.0, B + mid, ldb, 0));
    return trsm_rlt_binv(c, st, m, nb, mid, hi, W, B, ldb, V, ldv);
}

// V (m x n128, ldv) <- B L^-T for the resident factor (n128 = N rounded up to 128); B (m x n128, ldb) is consumed.
// C = beta * C + P_0 + P_1 + ... + P_{S-1} (each m x n, row stride n, `pstride` doubles apart), summed in that order
__global__ __launch_bounds__(256) void splitk_reduce_kernel(int64_t m, int64_t n2, int S, const double2 *__restrict__ P, int64_t pstride2,
                                                            double beta, double *__restrict__ C, int64_t ldc)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m * n2) return;
    const int64_t r = i / n2, q = i - r * n2;
    double2 *cp = reinterpret_cast<double2 *>(C + r * ldc) + q;
    double2 acc = make_double2(0.0, 0.0);
    if (beta != 0.0) {
        acc = *cp;
        acc.x *= beta;
        acc.y *= beta;
    }
    // (S is a power of two >= 2: pairs, fours or eights of loads in flight, added in slab order)
    if (S % 8 == 0) {
        for (int s = 0; s < S; s += 8) {
            double2 p[8];
#pragma unroll
            for (int q = 0; q < 8; q++) p[q] = P[(int64_t)(s + q) * pstride2 + i];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                acc.x += p[q].x;
                acc.y += p[q].y;
            }
        }
    } else {
        for (int s = 0; s < S; s += 2) {
            const double2 p0 = P[(int64_t)s * pstride2 + i], p1 = P[(int64_t)(s + 1) * pstride2 + i];
            acc.x = (acc.x + p0.x) + p1.x;
            acc.y = (acc.y + p0.y) + p1.y;
        }
    }
    *cp = acc;
}

// A GEMM of a few-rows solve: m <= 256 rows against k in the thousands is a handful of 32x32 tiles (128 at m = 64, n = 2048: half the
// chip idle) each walking a long k loop at ~0.3 us per 16-wide k-tile -- 37 us for 0.5 GFLOP.  Split along k instead: S chunks as the
// batch dimension of ONE launch (chunk s reads columns [s k/S, (s+1) k/S) of A and B and writes alpha * A_s B_s^T to its own m x n slab),
// then one pass adds the slabs to C in chunk order -- a fixed summation order, so results repeat bit for bit run to run (they differ in
// rounding from the unsplit sum; option `splitk` 0 restores that).  Measured (scratch/r05_splitk_ab.py, N = 8192, predict with std):
// 16 / 64 / 128 points 0.352 / 0.352 / 0.467 -> 0.281 / 0.280 / 0.424 ms; the leaf GEMM 37 -> 22 us + 4.8 us for the sum.  A split
// launch is bound by the 32x32 kernel's throughput with four workgroups per CU (~25 TFLOP/s), no longer by one workgroup's k loop.
// Not for k = 512 (the blocks of solves with 129..256 rows): one launch is 11 us there against 7.6 + 4.8 split in two.
// `tri`: the caller needs the lower triangle of C only (the predictive covariance: k = N against at most 256 x 256 outputs -- a
// dozen tiles walking 512 k-tiles each, 150 us at N = 8192); a split launch computes all of C, an unsplit one the lower tiles.
static int gemm_nt_few(gpt_ctx *c, hipStream_t st, int64_t m, int64_t n, int64_t k, double alpha, const double *A, int64_t lda,
                       const double *B, int64_t ldb, double beta, double *C, int64_t ldc, int tri = 0)
{
    const int64_t tiles = ((m + 31) / 32) * ((n + 31) / 32);
    int64_t S = 1;
    if (c->splitk && !c->use_graph && c->tile == 0 && k >= 1024 && (n % 2) == 0 && (ldc % 2) == 0)
        while (S < 32 && tiles * S < c->splitk && (k / (2 * S)) >= 256 && (k % (2 * S * 16)) == 0) S *= 2;
    if (S == 1) return gemm_nt(c, st, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, tri);
    double *P;
    const int64_t pstride = ((m + 31) / 32) * 32 * n;
    GPT_TRY(ensure(c, SLOT_SPLITK, (size_t)S * pstride * sizeof(double), (void **)&P));
    const int64_t kc = k / S;
    GPT_TRY(launch_gemm_nt(st, m, n, kc, alpha, A, lda, B, ldb, 0.0, P, n, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0, S, kc,
                           EdgeSig(), kc, pstride));
    const int64_t n2 = n / 2, tot = m * n2;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, m, n2, (int)S,
                       reinterpret_cast<const double2 *>(P), pstride / 2, beta, C, ldc);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

static int solve_rows_resident(gpt_ctx *c, hipStream_t st, int64_t m, int64_t n128, double *B, int64_t ldb, double *V, int64_t ldv)
{
    const int64_t nfull = (n128 / GPT_BINV_NB) * GPT_BINV_NB;
    if (nfull < 2 * GPT_BINV_NB) {
        GPT_TRY(launch_copy2d(st, m, n128, B, ldb, V, ldv));
        return trsm_rlt(c, st, m, n128, c->dA, c->NP, c->d_invd, V, ldv);
    }
    double *W;
    GPT_TRY(ensure_block_inverses(c, GPT_BINV_NB, nfull, &W));
    const int64_t rem = n128 - nfull;
    if (m <= 256) {
        // few rows: the halving recursion ends in updates with 64..256 rows and k of thousands -- a handful of workgroups
        // walking long k loops (1.6 ms at N = 8192).  Right-looking instead: after each leaf (one out-of-place GEMM against the
        // block inverse) one update of everything to its right.  What such a solve costs is the LENGTH of that chain of
        // dependent GEMMs, so up to GPT_FEW_ROWS rows the widest inverses that fit are used: 2048-wide blocks, then 1024-wide,
        // then 512-wide ones for what is left (predict with std at 64 points, N = 8192: 16 / 8 / 4 blocks -> 0.91 / 0.43 / ~0.35 ms).
        double *W3 = nullptr, *W2 = nullptr;
        int64_t n3 = 0, n2 = 0;
        if (m <= GPT_FEW_ROWS && n128 >= 4 * GPT_BINV_NB3) {
            n3 = (n128 / GPT_BINV_NB3) * GPT_BINV_NB3;
            GPT_TRY(ensure_block_inverses_wide(c, GPT_BINV_NB3, n3, &W3));
        } else if (m <= GPT_FEW_ROWS && n128 >= 4 * GPT_BINV_NB2) {
            n2 = (n128 / GPT_BINV_NB2) * GPT_BINV_NB2;
            GPT_TRY(ensure_block_inverses(c, GPT_BINV_NB2, n2, &W2));
        }
        int64_t j = 0;
        while (j < nfull) {
            const int64_t nb = (j + GPT_BINV_NB3 <= n3) ? GPT_BINV_NB3 : (j + GPT_BINV_NB2 <= n2) ? GPT_BINV_NB2 : GPT_BINV_NB;
            const double *Wj = (nb == GPT_BINV_NB3) ? W3 + j * nb : (nb == GPT_BINV_NB2) ? W2 + j * nb : W + j * nb;
            GPT_TRY(gemm_nt_few(c, st, m, nb, nb, 1.0, B + j, ldb, Wj, nb, 0.0, V + j, ldv));
            const int64_t r0 = j + nb;
            if (r0 < n128)
                GPT_TRY(gemm_nt_few(c, st, m, n128 - r0, nb, -1.0, V + j, ldv, c->dA + r0 * c->NP + j, c->NP, 1.0, B + r0, ldb));
            j = r0;
        }
    } else {
        GPT_TRY(trsm_rlt_binv(c, st, m, GPT_BINV_NB, 0, nfull, W, B, ldb, V, ldv));
        if (rem > 0) GPT_TRY(gemm_nt(c, st, m, rem, nfull, -1.0, V, ldv, c->dA + nfull * c->NP, c->NP, 1.0, B + nfull, ldb, 0));
    }
    if (rem > 0) {
        GPT_TRY(launch_copy2d(st, m, rem, B + nfull, ldb, V + nfull, ldv));
        GPT_TRY(trsm_rlt(c, st, m, rem, c->dA + nfull * c->NP + nfull, c->NP, c->d_invd + (nfull / 128) * GPT_WS_BLOCK, V + nfull, ldv));
    }
    return GPT_OK;
}

// ------------------------------------------------------------------------------------------------
// results to the host
// ------------------------------------------------------------------------------------------------
// Rows of a device matrix to host memory on the context's copy stream.  Pinned destinations (gpt_host_alloc, or anything
// hipHostRegister'ed / hipHostMalloc'ed by the caller) are written by the DMA engine directly and asynchronously; pageable
// ones go through a two-slot pinned ring with a host memcpy behind each slot (the runtime's own pageable path is a
// synchronous version of the same).  d2h_finish drains the ring.
#define GPT_STAGE_BYTES ((size_t)16 << 20)
struct StagePending { double *dst; int64_t ldd, rows, cols; bool on; };
static thread_local StagePending g_stage_pend[2] = {{nullptr, 0, 0, 0, false}, {nullptr, 0, 0, 0, false}};
static thread_local int g_stage_next = 0;

static bool host_ptr_is_pinned(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

static int stage_drain(gpt_ctx *c, int slot)
{
    StagePending &p = g_stage_pend[slot];
    if (!p.on) return GPT_OK;
    GPT_HIP_CHECK(hipEventSynchronize(c->cev[slot]));
    const double *src = c->h_stage + (size_t)slot * (GPT_STAGE_BYTES / sizeof(double));
    for (int64_t r = 0; r < p.rows; r++) memcpy(p.dst + r * p.ldd, src + r * p.cols, (size_t)p.cols * sizeof(double));
    p.on = false;
    return GPT_OK;
}

static int d2h_rows(gpt_ctx *c, double *dst, int64_t ldd, const double *dsrc, int64_t lds, int64_t rows, int64_t cols)
{
    if (host_ptr_is_pinned(dst)) {
        GPT_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ldd * sizeof(double), dsrc, (size_t)lds * sizeof(double),
                                       (size_t)cols * sizeof(double), (size_t)rows, hipMemcpyDeviceToHost, c->copy_stream));
        return GPT_OK;
    }
    if (!c->h_stage) GPT_HIP_CHECK(hipHostMalloc((void **)&c->h_stage, 2 * GPT_STAGE_BYTES, hipHostMallocDefault));
    const int64_t per = (int64_t)(GPT_STAGE_BYTES / sizeof(double)) / cols;      // rows per slot
    if (per < 1) {
        gpt_set_error("d2h_rows: a row of %lld doubles exceeds the staging slot", (long long)cols);
        return GPT_E_ARG;
    }
    for (int64_t r0 = 0; r0 < rows; r0 += per) {
        const int64_t nr = (rows - r0 < per) ? rows - r0 : per;
        const int slot = g_stage_next;
        g_stage_next ^= 1;
        GPT_TRY(stage_drain(c, slot));
        double *ring = c->h_stage + (size_t)slot * (GPT_STAGE_BYTES / sizeof(double));
        GPT_HIP_CHECK(hipMemcpy2DAsync(ring, (size_t)cols * sizeof(double), dsrc + r0 * lds, (size_t)lds * sizeof(double),
                                       (size_t)cols * sizeof(double), (size_t)nr, hipMemcpyDeviceToHost, c->copy_stream));
        GPT_HIP_CHECK(hipEventRecord(c->cev[slot], c->copy_stream));
        g_stage_pend[slot] = StagePending{dst + r0 * ldd, ldd, nr, cols, true};
    }
    return GPT_OK;
}

static int d2h_finish(gpt_ctx *c)
{
    GPT_TRY(stage_drain(c, g_stage_next));
    GPT_TRY(stage_drain(c, g_stage_next ^ 1));
    GPT_HIP_CHECK(hipStreamSynchronize(c->copy_stream));
    return GPT_OK;
}

// Pinned host memory for large results (the (M, M) predictive covariance): hipHostMalloc / hipHostFree.  gpt_predict writes
// into such a buffer with asynchronous DMA, overlapped with the computation; into pageable memory it stages.
extern "C" int gpt_host_alloc(int64_t bytes, void **out)
{
    if (!out || bytes <= 0) return GPT_E_ARG;
    *out = nullptr;
    GPT_HIP_CHECK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return GPT_OK;
}

// Free / total device memory of the context's GPU (hipMemGetInfo): callers that size scratch by what is there (the batched
// evaluator of GaussianProcess.ll_batch) ask first instead of failing in hipMalloc.
extern "C" int gpt_mem_info(gpt_ctx *c, int64_t *free_bytes, int64_t *total_bytes)
{
    CTX_ENTER(c);
    size_t f = 0, t = 0;
    GPT_HIP_CHECK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return GPT_OK;
}

// Returns the scratch of the batched evaluator (gpt_fit_batch*: nbatch matrices) to the device: the slots are otherwise kept
// until the context is destroyed, which suits a grid walked in many chunks and nobody else.
extern "C" int gpt_release_batch_scratch(gpt_ctx *c)
{
    CTX_ENTER(c);
    GPT_HIP_CHECK(hipStreamSynchronize(c->stream));
    GPT_HIP_CHECK(hipStreamSynchronize(c->panel_stream));
    c->batch_gen++;                                                   // (no batch resident any more)
    for (int slot : {SLOT_BATCH_A, SLOT_BATCH_WS, SLOT_BATCH_MISC, SLOT_PB_V, SLOT_PB_COV, SLOT_PB_MISC, SLOT_GB_U, SLOT_GB_W, SLOT_GB_MISC,
                     SLOT_SPB_LU, SLOT_SPB_LB, SLOT_SPB_V, SLOT_SPB_G, SLOT_SPB_PART, SLOT_SPB_MISC}) {
        DevBuf &b = c->slots[slot];
        if (b.p) GPT_HIP_CHECK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    return GPT_OK;
}

extern "C" int gpt_host_free(void *p)
{
    if (p) GPT_HIP_CHECK(hipHostFree(p));
    return GPT_OK;
}
