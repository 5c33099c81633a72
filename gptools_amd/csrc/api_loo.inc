// api_loo.inc -- part of api.hip (ONE translation unit: included from there, behind api_grad.inc).  Leave-one-out cross-validation
// from the resident factor (Rasmussen & Williams 5.4.2; DESIGN.md 17): gpt_loo, the value and the per-point residuals and variances
// from U = L^-T alone, and gpt_loo_grad_diff, the gradient of L_LOO through the pair pass of gpt_ll_grad_diff with another weight
// matrix (grad_diff_run, api_grad.inc).  Kernels: kloo.hip.
//
// Where everything lives (NP the padded order):
//   SLOT_UINV     U = L^-T; dead once W and the terms exist, then A = W diag(sqrt e), full NP x NP
//   SLOT_WINV     W = K_tot^-1, lower triangle by grad_weights; loo_weights completes the upper one (the lower stays what it was)
//   SLOT_LOO_V    V = A A^T, lower triangle
//   SLOT_LOO_VEC  d, r, sqrt(e), the rows' terms of L_LOO, u = W r (NP doubles each) and the sum of the terms

// d, r, sqrt(e), the terms and their sum from U (every entry of the five vectors' first four written; rows >= N: 1, 0, 0, 0), on
// `st`, which has joined alpha already
static int loo_terms(gpt_ctx *c, hipStream_t st, const double *U, LooDev *ld)
{
    const int64_t N = c->N, NP = c->NP;
    double *v;
    const size_t bytes = ((size_t)5 * NP + 8) * sizeof(double);
    GPT_TRY(ensure(c, SLOT_LOO_VEC, bytes, (void **)&v));
    if (c->debug_poison) GPT_HIP_CHECK(hipMemsetAsync(v, 0xff, bytes, st));
    ld->d = v;
    ld->r = v + NP;
    ld->se = v + 2 * NP;
    ld->term = v + 3 * NP;
    ld->u = v + 4 * NP;
    ld->sum = v + 5 * NP;
    return launch_loo_terms(st, U, NP, c->d_alpha, N, NP, ld->d, ld->r, ld->se, ld->term, ld->sum);
}

// The gradient's weights behind loo_terms: W mirrored to a full matrix, A = W diag(sqrt e) over U (dead by now), the lower half of
// V = A A^T block row by block row as grad_weights forms U U^T -- but A is full, so every k loop runs over all NP columns: NP^3
// flop -- and u = W r.
static int loo_weights(gpt_ctx *c, hipStream_t st, double *U, double *W, LooDev *ld)
{
    const int64_t N = c->N, NP = c->NP;
    double *V;
    GPT_TRY(ensure(c, SLOT_LOO_V, (size_t)NP * NP * sizeof(double), (void **)&V));
    if (c->debug_poison) {
        GPT_HIP_CHECK(hipMemsetAsync(V, 0xff, (size_t)NP * NP * sizeof(double), st));
        GPT_HIP_CHECK(hipMemsetAsync(U, 0xff, (size_t)NP * NP * sizeof(double), st));
    }
    // (the GEMMs below read every entry of A, so every entry of W must hold a finite number: its lower triangle does over all NP
    // rows -- the rows >= N are the inverse of the augmented / padding part -- and the mirror fills the rest from it, over the
    // whole padded order and not just the N x N part: see the T branch of grad_weights)
    GPT_TRY(launch_mirror_rows(st, W, NP, 0, NP, NP));
    GPT_TRY(launch_loo_scale_cols(st, W, NP, ld->se, NP, U, NP));
    const double *A = U;
    const int64_t nb = (NP / 8 >= 512) ? (NP / 8) / 128 * 128 : 512;
    for (int64_t r0 = 0; r0 < NP; r0 += nb) {
        const int64_t rows = (NP - r0 < nb) ? NP - r0 : nb;
        // the block row left of the diagonal block as a rectangle, the diagonal block itself as a lower trapezoid
        if (r0 > 0) GPT_TRY(gemm_nt(c, st, rows, r0, NP, 1.0, A + r0 * NP, NP, A, NP, 0.0, V + r0 * NP, NP, 0));
        GPT_TRY(gemm_nt(c, st, rows, rows, NP, 1.0, A + r0 * NP, NP, A + r0 * NP, NP, 0.0, V + r0 * NP + r0, NP, 1));
    }
    GPT_TRY(launch_gemv_n(st, N, N, W, NP, ld->r, ld->u));
    ld->V = V;
    return GPT_OK;
}

// the host outputs that were asked for, from `st`; synchronises it
static int loo_read_back(gpt_ctx *c, hipStream_t st, const LooDev &ld, const LooOut &lo)
{
    const size_t nb = (size_t)c->N * sizeof(double);
    std::vector<double> d(lo.var ? (size_t)c->N : 0);
    if (lo.ll) GPT_HIP_CHECK(hipMemcpyAsync(lo.ll, ld.sum, sizeof(double), hipMemcpyDeviceToHost, st));
    if (lo.resid) GPT_HIP_CHECK(hipMemcpyAsync(lo.resid, ld.r, nb, hipMemcpyDeviceToHost, st));
    if (lo.var) GPT_HIP_CHECK(hipMemcpyAsync(d.data(), ld.d, nb, hipMemcpyDeviceToHost, st));
    if (lo.u && ld.V) GPT_HIP_CHECK(hipMemcpyAsync(lo.u, ld.u, nb, hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    if (lo.var)
        for (int64_t i = 0; i < c->N; i++) lo.var[i] = 1.0 / d[(size_t)i];
    return GPT_OK;
}

extern "C" int gpt_loo(gpt_ctx *c, double *loo_ll, double *resid, double *var)
{
    CTX_ENTER(c);
    NEED_FACTOR(c);
    if (!loo_ll) return GPT_E_ARG;
    hipStream_t st = c->panel_stream;
    double *U, *W;
    GPT_TRY(grad_trinv(c, st, nullptr, &U, &W));
    GPT_TRY(stream_follows(c, c->stream, st, 0));             // alpha (main stream)
    LooDev ld;
    GPT_TRY(loo_terms(c, st, U, &ld));
    LooOut lo;
    lo.ll = loo_ll;
    lo.resid = resid;
    lo.var = var;
    GPT_TRY(loo_read_back(c, st, ld, lo));
    return stream_follows(c, st, c->stream, 1);
}

extern "C" int gpt_loo_grad_diff(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b,
                                 const double *denom, double *out, double *loo_ll, double *resid, double *var, double *u)
{
    CTX_ENTER(c);
    LooOut lo;
    lo.ll = loo_ll;
    lo.resid = resid;
    lo.var = var;
    lo.u = u;
    return grad_diff_run(c, "gpt_loo_grad_diff", nh, term_idx, params_a, params_b, denom, out, &lo);
}
