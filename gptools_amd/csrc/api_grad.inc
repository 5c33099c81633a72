// api_grad.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Triangular inverses (gpt_dev_trinv), the analytic LML gradient gpt_ll_grad and the per-pair differenced one,
// gpt_ll_grad_diff; grad_weights is the half the two share, grad_trinv its first half (all that gpt_loo needs), and grad_diff_run
// the body that gpt_ll_grad_diff shares with gpt_loo_grad_diff (api_loo.inc).
// ------------------------------------------------------------------------------------------------
// analytic gradient of the LML data term (ref: gptools/gaussian_process.py:1471-1520; SURVEY.md 8f-1)
// ------------------------------------------------------------------------------------------------
// U = L^-T (upper triangular, row-major) for the block range [lo, hi) of the resident factor.  U must hold the identity
// on its 128x128 diagonal blocks and zeros elsewhere on entry.  [[U11, U12], [0, U22]] with
// U12 = -(U11 L21^T) L22^-T: one NT GEMM and one right-TRSM per level, leaves by the packed-inverse panel kernel.
static int trtri_u(gpt_ctx *c, hipStream_t st, int64_t lo, int64_t hi, const double *L, int64_t ldl, const double *ws,
                   double *U, int64_t ldu)
{
    const int64_t n = hi - lo;
    if (n == 128)
        return launch_trsm_panel(st, 128, L + lo * ldl + lo, ldl, ws + (lo / 128) * GPT_WS_BLOCK, U + lo * ldu + lo, ldu);
    const int64_t h = (n / 256) * 128 > 0 ? (n / 256) * 128 : 128, mid = lo + h;
    GPT_TRY(trtri_u(c, st, lo, mid, L, ldl, ws, U, ldu));
    GPT_TRY(trtri_u(c, st, mid, hi, L, ldl, ws, U, ldu));
    double *U12 = U + lo * ldu + mid;
    // U11 is upper triangular: row chunk q only has non-zeros from its own first column on, so its k range starts there
    const int64_t nq = (h >= 2048) ? 8 : (h >= 512 ? 4 : 1), hc = h / nq;
    for (int64_t q = 0; q < nq; q++) {
        const int64_t o = q * hc;
        GPT_TRY(gemm_nt(c, st, hc, hi - mid, h - o, -1.0, U + (lo + o) * ldu + lo + o, ldu, L + mid * ldl + lo + o, ldl,
                        0.0, U12 + o * ldu, ldu, 0));
    }
    return trsm_rlt(c, st, h, hi - mid, L + mid * ldl + mid, ldl, ws + (mid / 128) * GPT_WS_BLOCK, U12, ldu);
}

__global__ void eye_blocks_kernel(double *__restrict__ U, int64_t ldu, int64_t n, int64_t bstride = 0)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) U[(int64_t)blockIdx.y * bstride + i * ldu + i] = 1.0;      // (blockIdx.y: a batch of equal matrices)
}

// W (n x n, row-major) = U^T through a 32x33 LDS tile
__global__ __launch_bounds__(256) void transpose_kernel(const double *__restrict__ U, int64_t ldu, double *__restrict__ W,
                                                        int64_t ldw, int64_t n)
{
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < n && c0 + tx < n) t[i][tx] = U[(r0 + i) * ldu + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < n && r0 + tx < n) W[(c0 + i) * ldw + r0 + tx] = t[tx][i];
}

// dW (n x n, row-major, zeros above the diagonal) <- L^-1 for a factored diagonal block and its workspace: the identity
// pushed through the panel TRSM (U = I L^-T) and one transpose.  With it the TRSM of a tall block of
// rows becomes ONE fp64-MFMA GEMM, X = B * (L^-1)^T = gemm_nt(B, dW) -- twice the flops of the substitution, but at the
// GEMM's rate instead of four latency-bound 128-column leaves and three narrow updates (31k x 512: 0.33 against
// 0.86 ms).  Used by gptools_amd/dist.py for the rows of a panel below its head.
extern "C" int gpt_dev_trinv(gpt_ctx *c, int64_t n, const double *dL, int64_t ldl, const double *d_invd, double *dW,
                             int64_t ldw)
{
    CTX_ENTER(c);
    if (n <= 0 || n % 128 || ldl < n || ldw < n || !dL || !d_invd || !dW) {
        gpt_set_error("trinv: n must be a positive multiple of 128");
        return GPT_E_ARG;
    }
    hipStream_t st = c->stream;
    double *U;
    GPT_TRY(ensure(c, SLOT_UINV, (size_t)n * n * sizeof(double), (void **)&U));
    // (the partitioned engines' block size: one launch instead of ten -- 69 -> ~43 us on the panel chain and nine launches less of
    // host enqueue per panel; solve.hip trinv512_kernel)
    if (n == 512 && ldw == 512 && !c->binv_launches) return launch_trinv512(st, 1, dL, ldl, d_invd, U, dW);
    GPT_HIP_CHECK(hipMemsetAsync(U, 0, (size_t)n * n * sizeof(double), st));
    hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, U, n, n);
    GPT_LAUNCH_CHECK();
    // U = I L^-T by the panel TRSM (7 launches at n = 512; the structured trtri_u of the gradient path needs 12 and the
    // zeros it would skip are not worth a launch at this size)
    GPT_TRY(trsm_rlt(c, st, n, n, dL, ldl, d_invd, U, n));
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, st, U, n,
                       dW, ldw, n);
    GPT_LAUNCH_CHECK();
    return GPT_OK;
}

#define GPT_BINV_NB 512
#define GPT_BINV_NB2 1024
static int trsm_rlt_binv(gpt_ctx *c, hipStream_t st, int64_t m, int64_t nb, int64_t lo, int64_t hi, const double *W, double *B,
                         int64_t ldb, double *V, int64_t ldv);

// dst (rows x cols, ldd) = src (cols x rows, lds)^T through a 32x33 LDS tile
__global__ __launch_bounds__(256) void transpose_rect_kernel(const double *__restrict__ src, int64_t lds, double *__restrict__ dst,
                                                             int64_t ldd, int64_t rows, int64_t cols, int64_t sstride = 0,
                                                             int64_t dstride = 0)
{
    __shared__ double t[32][33];
    src += (int64_t)blockIdx.z * sstride;                   // (blockIdx.z: a batch of equal blocks)
    dst += (int64_t)blockIdx.z * dstride;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;      // tile of dst
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) t[i][tx] = src[(c0 + i) * lds + r0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && c0 + tx < cols) dst[(r0 + i) * ldd + c0 + tx] = t[tx][i];
}

// U = L^-T over the block range [lo, hi) of the resident factor (multiples of GPT_BINV_NB = 512), GEMMs only:
//   leaf:   U_jj = W_j^T, W_j = L_jj^-1 the 512 x 512 block inverses that the many-right-hand-side solves keep anyway;
//   level:  U12 = -(U11 L21^T) L22^-T -- the product into the scratch matrix T (row chunks of U11 start their k range at
//           their own first column: U11 is upper triangular), then the right-TRSM against L22 as trsm_rlt_binv, whose
//           leaves are GEMMs against the block inverses and whose result lands in U.
// Round 2 did the TRSM by substitution in 128-column leaves (trtri_u above, kept for the ragged last block): 45 ms at
// N = 16384, 32 TFLOP/s on N^3/3.
static int trtri_u_gemm(gpt_ctx *c, hipStream_t st, int64_t lo, int64_t hi, const double *Wb, double *U, int64_t ldu, double *T,
                        int64_t ldt)
{
    const int64_t nb = GPT_BINV_NB, n = hi - lo;
    if (n == nb) {
        hipLaunchKernelGGL(transpose_rect_kernel, dim3((unsigned)(nb / 32), (unsigned)(nb / 32)), dim3(256), 0, st, Wb + lo * nb, nb,
                           U + lo * ldu + lo, ldu, nb, nb);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    }
    const int64_t h = (n / (2 * nb)) * nb > 0 ? (n / (2 * nb)) * nb : nb, mid = lo + h;
    GPT_TRY(trtri_u_gemm(c, st, lo, mid, Wb, U, ldu, T, ldt));
    GPT_TRY(trtri_u_gemm(c, st, mid, hi, Wb, U, ldu, T, ldt));
    const double *L = c->dA;
    const int64_t ldl = c->NP;
    const int64_t nq = (h >= 2048) ? 8 : (h >= 1024 ? 4 : 1), hc = h / nq;
    for (int64_t q = 0; q < nq; q++) {
        const int64_t o = q * hc;
        GPT_TRY(gemm_nt(c, st, hc, hi - mid, h - o, -1.0, U + (lo + o) * ldu + lo + o, ldu, L + mid * ldl + lo + o, ldl, 0.0,
                        T + (lo + o) * ldt + mid, ldt, 0));
    }
    return trsm_rlt_binv(c, st, h, nb, mid, hi, Wb, T + lo * ldt, ldt, U + lo * ldu, ldu);
}

// The same for `nbatch` equal diagonal blocks at once (the nb-wide inverses of few-rows solves: nb = 1024 / 2048, block J at
// factor rows [J nb, J nb + nb)): every GEMM and transpose of the recursion is ONE launch with the blocks as its batch dimension
// (round 5; block by block the 2048-wide inverses of N = 8192 were 64 dependent launches, 0.9 ms of the first predict after a fit).
// Indices are those of block 0; U and T are strips of nb-wide blocks (block J at rows [J nb, J nb + nb), row stride nb).
struct WideBatch { int64_t n, sU, sT, sL, sW; };
static int gemm_b(hipStream_t st, int64_t m, int64_t n, int64_t k, double alpha, const double *A, int64_t lda, int64_t sA, const double *B,
                  int64_t ldb, int64_t sB, double beta, double *C, int64_t ldc, int64_t sC, int64_t nbatch)
{
    return launch_gemm_nt(st, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(), EdgeSig(), 0, nbatch, sA,
                          EdgeSig(), sB, sC);
}
static int trsm_rlt_binv_b(gpt_ctx *c, hipStream_t st, int64_t m, int64_t nb, int64_t lo, int64_t hi, const double *W, double *B, int64_t ldb,
                           double *V, int64_t ldv, const WideBatch &wb)
{
    const int64_t n = hi - lo;
    if (n == nb) return gemm_b(st, m, nb, nb, 1.0, B + lo, ldb, wb.sT, W + lo * nb, nb, wb.sW, 0.0, V + lo, ldv, wb.sU, wb.n);
    const int64_t h = (n / (2 * nb)) * nb > 0 ? (n / (2 * nb)) * nb : nb;
    const int64_t mid = lo + h;
    GPT_TRY(trsm_rlt_binv_b(c, st, m, nb, lo, mid, W, B, ldb, V, ldv, wb));
    GPT_TRY(gemm_b(st, m, hi - mid, h, -1.0, V + lo, ldv, wb.sU, c->dA + mid * c->NP + lo, c->NP, wb.sL, 1.0, B + mid, ldb, wb.sT, wb.n));
    return trsm_rlt_binv_b(c, st, m, nb, mid, hi, W, B, ldb, V, ldv, wb);
}
static int trtri_u_gemm_b(gpt_ctx *c, hipStream_t st, int64_t lo, int64_t hi, const double *Wb, double *U, int64_t ldu, double *T, int64_t ldt,
                          const WideBatch &wb)
{
    const int64_t nb = GPT_BINV_NB, n = hi - lo;
    if (n == nb) {
        hipLaunchKernelGGL(transpose_rect_kernel, dim3((unsigned)(nb / 32), (unsigned)(nb / 32), (unsigned)wb.n), dim3(256), 0, st,
                           Wb + lo * nb, nb, U + lo * ldu + lo, ldu, nb, nb, wb.sW, wb.sU);
        GPT_LAUNCH_CHECK();
        return GPT_OK;
    }
    const int64_t h = (n / (2 * nb)) * nb > 0 ? (n / (2 * nb)) * nb : nb, mid = lo + h;
    GPT_TRY(trtri_u_gemm_b(c, st, lo, mid, Wb, U, ldu, T, ldt, wb));
    GPT_TRY(trtri_u_gemm_b(c, st, mid, hi, Wb, U, ldu, T, ldt, wb));
    const int64_t nq = (h >= 1024) ? 2 : 1, hc = h / nq;          // (row chunks of U11 start their k range at their own first column)
    for (int64_t q = 0; q < nq; q++) {
        const int64_t o = q * hc;
        GPT_TRY(gemm_b(st, hc, hi - mid, h - o, -1.0, U + (lo + o) * ldu + lo + o, ldu, wb.sU, c->dA + mid * c->NP + lo + o, c->NP, wb.sL, 0.0,
                       T + (lo + o) * ldt + mid, ldt, wb.sT, wb.n));
    }
    return trsm_rlt_binv_b(c, st, h, nb, mid, hi, Wb, T + lo * ldt, ldt, U + lo * ldu, ldu, wb);
}

// The weights of a gradient's pair pass, G = alpha' alpha'^T - W' over Np points: W' (lower triangle, row stride ldwp) and alpha'.
// Without a transform W' = W = K_tot^-1 and alpha' = alpha over the N training points; with T, W' = T^T W T and alpha' = T^T alpha
// over the Nx latent points.  W: K_tot^-1 itself (NP x NP), which the noise entry of a transformed model reads (grad_noise_trace_T).
struct GradWeights {
    const double *Wp = nullptr, *ap = nullptr;
    int64_t Np = 0, ldwp = 0;
    double *W = nullptr, *U = nullptr;      // U = L^-T (SLOT_UINV): dead for the LML once W exists, the leave-one-out terms read it
};

// The first half of grad_weights, and all that the leave-one-out VALUE needs (gpt_loo, api_loo.inc): U = L^-T (NP x NP, SLOT_UINV)
// on the panel stream `st` behind the main stream, with SLOT_WINV as the recursion's scratch matrix -- *Wout, whose content is
// scratch afterwards.  alpha is enqueued on the main stream; the caller joins it (stream_follows main -> st) before reading it.
// ge (GPT_GRAD_TIMING; else NULL): [0] and [1] recorded here, before and after the inverse.
static int grad_trinv(gpt_ctx *c, hipStream_t st, hipEvent_t *ge, double **Uout, double **Wout)
{
    const int64_t NP = c->NP;
    // Everything here runs on the panel stream: it is not CU-masked (the main stream leaves 32 of the 256 CUs to it), and
    // nothing else is in flight.
    GPT_TRY(stream_follows(c, c->stream, st, 0));
    double *U, *W;
    // K_tot^-1 = L^-T L^-1 = U U^T: triangular inverse (N^3/3 flop), then the lower half of U U^T block row by block row
    // with k starting at the diagonal (N^3/3) -- all on the fp64-MFMA GEMM
    if (ge) GPT_HIP_CHECK(hipEventRecord(ge[0], st));
    const int64_t nfull = (NP / GPT_BINV_NB) * GPT_BINV_NB;
    double *Wb = nullptr;
    GPT_TRY(ensure(c, SLOT_UINV, (size_t)NP * NP * sizeof(double), (void **)&U));
    GPT_TRY(ensure(c, SLOT_WINV, (size_t)NP * NP * sizeof(double), (void **)&W));
    if (nfull >= 2 * GPT_BINV_NB) {
        // (the block inverses are built on the main stream with the head of SLOT_UINV as their scratch: before U is touched)
        GPT_TRY(ensure_block_inverses(c, GPT_BINV_NB, nfull, &Wb));
        GPT_TRY(stream_follows(c, c->stream, st, 1));
    }
    GPT_TRY(ensure_alpha(c));                                  // (main stream; joined below before the pair pass)
    if (c->debug_poison)                                       // test aid: every byte 0xff = NaN in whatever is not written below
        GPT_HIP_CHECK(hipMemsetAsync(W, 0xff, (size_t)NP * NP * sizeof(double), st));
    GPT_HIP_CHECK(hipMemsetAsync(U, 0, (size_t)NP * NP * sizeof(double), st));
    if (Wb) {
        GPT_TRY(trtri_u_gemm(c, st, 0, nfull, Wb, U, NP, W, NP));           // (W doubles as the scratch matrix T)
        if (nfull < NP) {
            // ragged last block [nfull, NP): by substitution, then its column block of U as above with an in-place TRSM
            hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((NP - nfull + 255) / 256)), dim3(256), 0, st,
                               U + nfull * NP + nfull, NP, NP - nfull);
            GPT_LAUNCH_CHECK();
            GPT_TRY(trtri_u(c, st, nfull, NP, c->dA, NP, c->d_invd, U, NP));
            const int64_t nq = 8, hc = nfull / nq / 64 * 64;
            for (int64_t o = 0; o < nfull; o += hc) {
                const int64_t rows = (nfull - o < hc || o + 2 * hc > nfull) ? nfull - o : hc;
                GPT_TRY(gemm_nt(c, st, rows, NP - nfull, nfull - o, -1.0, U + o * NP + o, NP, c->dA + nfull * NP + o, NP, 0.0,
                                U + o * NP + nfull, NP, 0));
                if (rows != hc) break;
            }
            GPT_TRY(trsm_rlt(c, st, nfull, NP - nfull, c->dA + nfull * NP + nfull, NP, c->d_invd + (nfull / 128) * GPT_WS_BLOCK,
                             U + nfull, NP));
        }
    } else {
        hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, st, U, NP, NP);
        GPT_LAUNCH_CHECK();
        GPT_TRY(trtri_u(c, st, 0, NP, c->dA, NP, c->d_invd, U, NP));
    }
    if (ge) GPT_HIP_CHECK(hipEventRecord(ge[1], st));
    *Uout = U;
    *Wout = W;
    return GPT_OK;
}

// The half that gpt_ll_grad, gpt_ll_grad_diff and gpt_loo_grad_diff share: the triangular inverse (grad_trinv), U U^T and the T
// branch, enqueued on the panel stream `st` behind the main stream; the pair pass of the caller follows on `st`.  ge
// (GPT_GRAD_TIMING; else NULL): four events, [0] .. [2] recorded here -- before the inverse, after it, after U U^T.
static int grad_weights(gpt_ctx *c, hipStream_t st, hipEvent_t *ge, GradWeights *gw)
{
    const int64_t N = c->N, NP = c->NP;
    double *U, *W;
    GPT_TRY(grad_trinv(c, st, ge, &U, &W));
    // (block rows of about NP/8: skinnier launches exploit more of U's zeros but run the GEMM far below its rate)
    int64_t nbdiv = 8;
    if (const char *e = getenv("GPT_GRAD_ROWS_DIV")) nbdiv = atoi(e) > 0 ? atoi(e) : 8;
    const int64_t nb = (NP / nbdiv >= 512) ? (NP / nbdiv) / 128 * 128 : 512;
    for (int64_t r0 = 0; r0 < NP; r0 += nb) {
        const int64_t rows = (NP - r0 < nb) ? NP - r0 : nb;
        // the block row left of the diagonal block as a rectangle, the diagonal block itself as a lower trapezoid (the pair
        // pass reads the lower triangle of W only)
        if (r0 > 0)
            GPT_TRY(gemm_nt(c, st, rows, r0, NP - r0, 1.0, U + r0 * NP + r0, NP, U + r0, NP, 0.0, W + r0 * NP, NP, 0));
        GPT_TRY(gemm_nt(c, st, rows, rows, NP - r0, 1.0, U + r0 * NP + r0, NP, U + r0 * NP + r0, NP, 0.0, W + r0 * NP + r0, NP, 1));
    }
    if (ge) GPT_HIP_CHECK(hipEventRecord(ge[2], st));
    GPT_TRY(stream_follows(c, c->stream, st, 0));             // alpha (main stream) is needed from here on
    // With a linear transform (ref :1499-1500, dK_tot = T dK T^T):  tr(K_tot^-1 T dK T^T) = tr((T^T K_tot^-1 T) dK) and
    // alpha^T T dK T^T alpha = (T^T alpha)^T dK (T^T alpha): the pair pass runs over the Nx LATENT points with
    // W' = T^T W T (two GEMMs with the resident T) and alpha' = T^T alpha.  The noise entry (out[nh]) is taken from the
    // untransformed pair afterwards (see below).
    const double *Wp = W, *ap = c->d_alpha;
    int64_t Np = N, ldwp = NP;
    double *Wt = nullptr, *at = nullptr;
    if (c->dT) {
        const int64_t Nx = c->Nx, NxP = c->NxP, NyP = round_up(N, 64), NxQ = round_up(Nx, 64);
        double *TT, *Yt;
        // T^T (NxQ x NyP, zero padded), Y^T = T^T W (NxQ x NyP; W made fully symmetric first), W' = T^T Y (lower)
        GPT_TRY(ensure(c, SLOT_TK, (size_t)NxQ * NyP * sizeof(double) * 2, (void **)&TT));
        Yt = TT + NxQ * NyP;
        GPT_HIP_CHECK(hipMemsetAsync(TT, 0, (size_t)NxQ * NyP * sizeof(double), st));
        hipLaunchKernelGGL(transpose_rect_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((Nx + 31) / 32)), dim3(256), 0, st,
                           c->dT, NxP, TT, NyP, Nx, N);
        GPT_LAUNCH_CHECK();
        // (the GEMM below runs its k loop to NyP = round_up(N, 64) and reads W[j][k] for every j, k < NyP: the whole NyP x NyP
        // block must hold finite numbers -- its lower triangle does (rows >= N: the inverse of the padded matrix' augmented /
        // padding part, multiplied by the zero padding of T^T), the strictly upper entries only once mirrored.  Mirroring just
        // the N x N part left the columns [N, NyP) to whatever the scratch slot held: ADVICE r3.)
        GPT_TRY(launch_mirror_rows(st, W, NP, 0, NyP, NyP));
        GPT_TRY(gemm_nt(c, st, NxQ, NyP, NyP, 1.0, TT, NyP, W, NP, 0.0, Yt, NyP, 0));
        GPT_TRY(ensure(c, SLOT_KFULL, ((size_t)NxQ * NxQ + (size_t)NxQ) * sizeof(double), (void **)&Wt));
        at = Wt + NxQ * NxQ;
        GPT_TRY(gemm_nt(c, st, NxQ, NxQ, NyP, 1.0, TT, NyP, Yt, NyP, 0.0, Wt, NxQ, 1));
        GPT_TRY(launch_gemv_n(st, Nx, N, TT, NyP, c->d_alpha, at));
        Wp = Wt;
        ap = at;
        Np = Nx;
        ldwp = NxQ;
    }
    gw->Wp = Wp;
    gw->ap = ap;
    gw->Np = Np;
    gw->ldwp = ldwp;
    gw->W = W;
    gw->U = U;
    return GPT_OK;
}

// The noise entry with a transform: the reference differentiates the DiagonalNoiseKernel as 2 sigma_n I over the
// OBSERVATIONS, not transformed by T (ref :1482-1488, dK = 2 sigma_n eye(len(y))): 1/2 sum_i (alpha_i^2 - (K_tot^-1)_ii) from the
// untransformed pair, replacing what the pass over the latent points left in its place.
static int grad_noise_trace_T(gpt_ctx *c, hipStream_t st, const double *W, double *dpart, double *out)
{
    GPT_TRY(launch_alpha_trace(st, c->d_alpha, W, c->NP, c->N, dpart));
    double tr = 0.0;
    GPT_HIP_CHECK(hipMemcpyAsync(&tr, dpart, sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    *out = 0.5 * tr;
    return GPT_OK;
}

// GPT_GRAD_TIMING: the four events of a gradient's three phases, owned by the entry point -- destroyed on every way out of it, an
// early error return included
struct GradTimer {
    hipEvent_t ge[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    int init()
    {
        on = getenv("GPT_GRAD_TIMING") != nullptr;
        if (on)
            for (auto &e : ge) GPT_HIP_CHECK(hipEventCreate(&e));
        return GPT_OK;
    }
    hipEvent_t *events() { return on ? ge : nullptr; }
    ~GradTimer()
    {
        for (auto &e : ge)
            if (e) hipEventDestroy(e);
    }
};

// ... and the phases on stderr (ge as grad_weights took it; [3] recorded here)
static int grad_timing_report(const char *who, int64_t N, hipStream_t st, hipEvent_t *ge)
{
    GPT_HIP_CHECK(hipEventRecord(ge[3], st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    float a = 0, b = 0, d = 0;
    hipEventElapsedTime(&a, ge[0], ge[1]);
    hipEventElapsedTime(&b, ge[1], ge[2]);
    hipEventElapsedTime(&d, ge[2], ge[3]);
    fprintf(stderr, "%s N=%lld: triangular inverse %.2f ms, U U^T %.2f ms, pair pass %.2f ms\n", who, (long long)N, a, b, d);
    return GPT_OK;
}

// The partial rows of one launch of a pair pass -- nblk workgroups x (GPT_GRAD_MAXH + 1) slots -- copied to the host, and the sum of a
// slot over the workgroups in index order, left to right: what gpt_ll_grad, grad_diff_run and the Z-Z pass of gpt_sparse_grad_diff
// turn into an entry.  fetch() synchronises `st`.
struct GradPartials {
    int nblk;
    std::vector<double> h;
    explicit GradPartials(int nblk_) : nblk(nblk_), h((size_t)nblk_ * (GPT_GRAD_MAXH + 1)) {}
    size_t bytes() const { return h.size() * sizeof(double); }
    int fetch(hipStream_t st, const double *dpart)
    {
        GPT_HIP_CHECK(hipMemcpyAsync(h.data(), dpart, bytes(), hipMemcpyDeviceToHost, st));
        GPT_HIP_CHECK(hipStreamSynchronize(st));
        return GPT_OK;
    }
    double sum(int q) const
    {
        double s = 0.0;
        for (int b = 0; b < nblk; b++) s += h[(size_t)b * (GPT_GRAD_MAXH + 1) + q];
        return s;
    }
};

extern "C" int gpt_ll_grad(gpt_ctx *c, int nh, const int *term_idx, const int *local_idx, double *out)
{
    CTX_ENTER(c);
    GPT_TRY(refuse_warp(c, "gpt_ll_grad"));
    NEED_FACTOR(c);
    if (!c->have_kernel) {
        gpt_set_error("gpt_ll_grad needs a factorisation produced by gpt_fit / gpt_fit_sum");
        return GPT_E_STATE;
    }
    if (nh < 0 || (nh > 0 && (!term_idx || !local_idx)) || !out) return GPT_E_ARG;
    for (int h = 0; h < nh; h++) {
        if (term_idx[h] < 0 || term_idx[h] >= c->model.nterms) return GPT_E_ARG;
        if (c->model.f1[term_idx[h]].kernel_id != GPT_KERNEL_SE || c->model.second(term_idx[h])) {
            gpt_set_error("hyper-parameter derivatives exist for the squared-exponential kernel only "
                          "(ref: matern.py:543-544)");
            return GPT_E_NOTIMPL;
        }
        if (local_idx[h] < 0 || local_idx[h] > c->D) return GPT_E_ARG;
    }
    hipStream_t st = c->panel_stream;
    GradTimer timer;
    GPT_TRY(timer.init());
    GradWeights gw;
    GPT_TRY(grad_weights(c, st, timer.events(), &gw));
    const double *Wp = gw.Wp, *ap = gw.ap;
    const int64_t Np = gw.Np, ldwp = gw.ldwp;
    double *dpart;
    // sum_ab (alpha_a alpha_b - W_ab) dK_h[a][b], per kernel term, GPT_GRAD_MAXH parameters per launch
    const int nblk = grad_reduce_blocks(Np);
    GradPartials hpart(nblk);
    GPT_TRY(ensure(c, SLOT_GPART, hpart.bytes(), (void **)&dpart));
    bool have_trace = false;
    const int nterms = c->model.nterms;
    for (int t = 0; t < nterms || !have_trace; t++) {
        std::vector<int> hs, where;
        if (t < nterms)
            for (int h = 0; h < nh; h++)
                if (term_idx[h] == t) {
                    hs.push_back(local_idx[h]);
                    where.push_back(h);
                }
        if (hs.empty() && have_trace) continue;
        const KParams &kp = c->model.f1[t < nterms ? t : 0];
        for (size_t b0 = 0; b0 < hs.size() || !have_trace; b0 += GPT_GRAD_MAXH) {
            const int cnt = (int)((hs.size() - b0 < (size_t)GPT_GRAD_MAXH) ? hs.size() - b0 : (size_t)GPT_GRAD_MAXH);
            KParams ks = kp;
            ks.symmetric = 1;
            GPT_TRY(launch_grad_reduce(st, ks, cnt > 0 ? cnt : 0, cnt > 0 ? hs.data() + b0 : nullptr, c->dX, c->dn, Np,
                                       ap, Wp, ldwp, dpart));
            GPT_TRY(hpart.fetch(st, dpart));
            for (int q = 0; q < cnt; q++) out[where[b0 + q]] = 0.5 * hpart.sum(q);
            if (!have_trace) {
                out[nh] = 0.5 * hpart.sum(GPT_GRAD_MAXH);
                have_trace = true;
            }
            if (cnt <= 0) break;
        }
    }
    if (c->dT) GPT_TRY(grad_noise_trace_T(c, st, gw.W, dpart, &out[nh]));
    if (timer.on) GPT_TRY(grad_timing_report("gpt_ll_grad", c->N, st, timer.ge));
    return stream_follows(c, st, c->stream, 1);     // the main stream continues behind this (the block inverses stay valid for predict)
}


// The leave-one-out half of grad_diff_run (api_loo.inc).  LooOut: the host outputs of the leave-one-out entry points, NULL members
// are not written; LooDev: what loo_terms / loo_weights left on the device.
struct LooOut {
    double *ll = nullptr, *resid = nullptr, *var = nullptr, *u = nullptr;
};
struct LooDev {
    double *d = nullptr, *r = nullptr, *se = nullptr, *term = nullptr, *u = nullptr, *sum = nullptr, *V = nullptr;
};
static int loo_terms(gpt_ctx *c, hipStream_t st, const double *U, LooDev *ld);
static int loo_weights(gpt_ctx *c, hipStream_t st, double *U, double *W, LooDev *ld);
static int loo_read_back(gpt_ctx *c, hipStream_t st, const LooDev &ld, const LooOut &lo);

// The gradient of the LML -- or, with `loo`, of the leave-one-out objective -- for ANY term of the resident model, by central
// differences of the pair function taken per pair (kgrad.hip): parameter h is given as its term's complete parameter vector at the
// two stencil points, and every stencil point goes through parse_model as a one-term model with the ids and parameter counts the
// fit was given -- whatever that refuses is refused here, before anything is launched.  After K_tot^-1 a parameter costs two O(N^2)
// evaluations of its term instead of a factorisation.  The body of gpt_ll_grad_diff (loo == NULL: the weights alpha alpha^T - W)
// and of gpt_loo_grad_diff (u alpha^T + alpha u^T - V, loo_weights): the same checks, the same launch groups.
static int grad_diff_run(gpt_ctx *c, const char *who, int nh, const int *term_idx, const double *params_a, const double *params_b,
                         const double *denom, double *out, const LooOut *loo)
{
    GPT_TRY(refuse_warp(c, who));
    NEED_FACTOR(c);
    if (!c->have_kernel) {
        gpt_set_error("%s needs a factorisation produced by gpt_fit / gpt_fit_sum / gpt_fit_terms", who);
        return GPT_E_STATE;
    }
    if (loo && c->dT) {
        gpt_set_error("%s: not with a linear transform T -- dK_tot = T dK T^T needs the leave-one-out weights carried to the latent "
                      "points, which is not implemented", who);
        return GPT_E_NOTIMPL;
    }
    if (nh < 0 || (nh > 0 && (!term_idx || !params_a || !params_b || !denom)) || !out) return GPT_E_ARG;
    const ModelKernel &m = c->model;
    GradStencil gs;
    GPT_TRY(grad_stencil_build(who, c->D, c->n_maxsum, c->n_colmax, m, nh, term_idx, params_a, params_b, denom, &gs));
    const std::vector<KParams> &kp1 = gs.kp1, &kp2 = gs.kp2;
    hipStream_t st = c->panel_stream;
    GradTimer timer;
    GPT_TRY(timer.init());
    GradWeights gw;
    GPT_TRY(grad_weights(c, st, timer.events(), &gw));
    // the pair pass's weight matrix and second vector: W and none, or V and u
    const double *pw = gw.Wp, *pu = nullptr;
    LooDev ld;
    if (loo) {
        GPT_TRY(loo_terms(c, st, gw.U, &ld));
        GPT_TRY(loo_weights(c, st, gw.U, gw.W, &ld));
        pw = ld.V;
        pu = ld.u;
    }
    const int nblk = grad_reduce_blocks(gw.Np);
    double *dpart;
    KParams *dkp;
    GradPartials hpart(nblk);
    GPT_TRY(ensure(c, SLOT_GPART, hpart.bytes(), (void **)&dpart));
    const size_t nk = kp1.size() > 0 ? kp1.size() : 1;      // (nh == 0: one launch for the trace, which reads no KParams)
    GPT_TRY(ensure(c, SLOT_GKP, 2 * nk * sizeof(KParams), (void **)&dkp));
    if (!kp1.empty()) {
        GPT_HIP_CHECK(hipMemcpyAsync(dkp, kp1.data(), kp1.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
        GPT_HIP_CHECK(hipMemcpyAsync(dkp + nk, kp2.data(), kp2.size() * sizeof(KParams), hipMemcpyHostToDevice, st));
        GPT_HIP_CHECK(hipStreamSynchronize(st));      // (pageable sources: the vectors may not change before the copies are through)
    }
    // one launch group: its entries, and the noise trace from the first one
    bool have_trace = false;
    auto group = [&](int b0, int cnt, int t) -> int {
        GPT_TRY(launch_kgrad_diff(st, m.f1[t].kernel_id, m.second(t) ? m.f2[t].kernel_id : -1, c->D, dkp + 2 * b0, dkp + nk + 2 * b0, cnt,
                                  c->dX, c->dn, gw.Np, gw.ap, pw, gw.ldwp, dpart, 1, pu));
        GPT_TRY(hpart.fetch(st, dpart));
        for (int q = 0; q < cnt; q++) out[gs.where[b0 + q]] = 0.5 * hpart.sum(q) / denom[gs.where[b0 + q]];
        if (!have_trace) {
            out[nh] = 0.5 * hpart.sum(GPT_GRAD_MAXH);
            have_trace = true;
        }
        return GPT_OK;
    };
    GPT_TRY(for_each_group(gs, group));
    if (!have_trace) GPT_TRY(group(0, 0, 0));                 // (nh == 0: one launch for the trace alone)
    if (c->dT) GPT_TRY(grad_noise_trace_T(c, st, gw.W, dpart, &out[nh]));
    if (loo) GPT_TRY(loo_read_back(c, st, ld, *loo));
    if (timer.on) GPT_TRY(grad_timing_report(who, c->N, st, timer.ge));
    return stream_follows(c, st, c->stream, 1);
}

extern "C" int gpt_ll_grad_diff(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b,
                                const double *denom, double *out)
{
    CTX_ENTER(c);
    return grad_diff_run(c, "gpt_ll_grad_diff", nh, term_idx, params_a, params_b, denom, out, nullptr);
}
