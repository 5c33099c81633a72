// api_dev.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Device API (gpt_dev_*): raw device pointers on the context's streams, for the one-process-per-GPU engines.
// ------------------------------------------------------------------------------------------------
// device API
// ------------------------------------------------------------------------------------------------
extern "C" int gpt_dev_kbuild(gpt_ctx *c, int kernel_id, const double *params_host, int nparams, const double *dXi,
                              const int32_t *dni, int64_t M, const double *dXj, const int32_t *dnj, int64_t P, int D,
                              int hyper_deriv, int symmetric, const int32_t *noise_n_host, int lower_only, int64_t i0,
                              int64_t j0, const double *d_err_y, double noise_var, double diag_add, double *dK,
                              int64_t ldk)
{
    CTX_ENTER(c);
    KParams kp;
    GPT_TRY(make_kparams(kernel_id, params_host, nparams, D, hyper_deriv, symmetric, noise_n_host, &kp));
    return launch_kbuild(c->stream, kp, nullptr, {dXi, dni, M, dXj, dnj, P, lower_only, i0, j0, d_err_y, noise_var, diag_add, dK, ldk});
}

extern "C" int gpt_dev_gemm_nt(gpt_ctx *c, int64_t m, int64_t n, int64_t k, double alpha, const double *dA,
                               int64_t lda, const double *dB, int64_t ldb, double beta, double *dC, int64_t ldc,
                               int tri)
{
    CTX_ENTER(c);
    return gemm_nt(c, c->stream, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, tri);
}

extern "C" int gpt_dev_gemm_nt_stair(gpt_ctx *c, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha,
                                     const double *dA, int64_t lda, const double *dB, int64_t ldb, int64_t b_stride,
                                     int64_t row_step, double beta, double *dC, int64_t ldc)
{
    CTX_ENTER(c);
    // profiled like the single-GPU updates (bench.py's roofline object of the partitioned line): algorithmic flops =
    // 2k per element of the staircase (segment q: lower trapezoid of (m - q row_step) x seg_cols)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->prof_gemm && !c->use_graph) {
        double elems = 0.0;
        for (int64_t q = 0; q < nseg; q++) {
            const double mq = (double)(m - q * row_step), w = (double)seg_cols;
            if (mq > 0) elems += 0.5 * w * (w + 1.0) + (mq - w > 0 ? (mq - w) * w : 0.0);
        }
        const double flops = 2.0 * (double)k * elems;
        if (flops >= 1.0e9) {
            if (c->gprof_used == c->gprof.size()) {
                gpt_ctx::GemmProf g;
                GPT_HIP_CHECK(hipEventCreate(&g.e0));
                GPT_HIP_CHECK(hipEventCreate(&g.e1));
                g.flops = 0;
                g.stop = g.e1;
                c->gprof.push_back(g);
            }
            gpt_ctx::GemmProf *gp = &c->gprof[c->gprof_used++];
            gp->flops = flops;
            gp->stop = gp->e1;
            e0 = gp->e0;
            e1 = gp->e1;
        }
    }
    return launch_gemm_nt_stair(c->stream, m, nseg, seg_cols, k, alpha, dA, lda, dB, ldb, b_stride, row_step, beta, dC,
                                ldc, (int)c->dev_gemm_pad, e0, e1);
}

// Trailing update of one rank of the 2-D block-cyclic engine in one launch (gemm.hip launch_gemm_nt_gridstair; profiled like the
// staircase above).
extern "C" int gpt_dev_gemm_nt_gridstair(gpt_ctx *c, int64_t m, int64_t nseg, int64_t seg_cols, int64_t k, double alpha,
                                         const double *dA, int64_t lda, const double *dB, int64_t ldb, int64_t off, int64_t num,
                                         int64_t den, int64_t base, double beta, double *dC, int64_t ldc)
{
    CTX_ENTER(c);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->prof_gemm && !c->use_graph && den > 0 && seg_cols > 0) {
        double elems = 0.0;
        for (int64_t q = 0; q < nseg; q++) {
            const int64_t v = off + q * num, rs = (v + den - 1) / den - base;
            const double mq = (double)(m - rs * seg_cols), w = (double)seg_cols;
            if (mq <= 0) continue;
            elems += (v % den == 0) ? 0.5 * w * (w + 1.0) + (mq - w > 0 ? (mq - w) * w : 0.0) : mq * w;
        }
        const double flops = 2.0 * (double)k * elems;
        if (flops >= 1.0e9) {
            if (c->gprof_used == c->gprof.size()) {
                gpt_ctx::GemmProf g;
                GPT_HIP_CHECK(hipEventCreate(&g.e0));
                GPT_HIP_CHECK(hipEventCreate(&g.e1));
                g.flops = 0;
                g.stop = g.e1;
                c->gprof.push_back(g);
            }
            gpt_ctx::GemmProf *gp = &c->gprof[c->gprof_used++];
            gp->flops = flops;
            gp->stop = gp->e1;
            e0 = gp->e0;
            e1 = gp->e1;
        }
    }
    const int lds_pad = c->lookahead ? c->gemm_pad : (int)c->dev_gemm_pad;
    return launch_gemm_nt_gridstair(c->stream, m, nseg, seg_cols, k, alpha, dA, lda, dB, ldb, off, num, den, base, beta, dC, ldc,
                                    lds_pad, e0, e1);
}

extern "C" int gpt_dev_row_sumsq(gpt_ctx *c, const double *d_row, int64_t w, double *d_acc)
{
    CTX_ENTER(c);
    return launch_row_sumsq(c->stream, d_row, w, d_acc);
}

extern "C" int gpt_dev_potrf_panel(gpt_ctx *c, int64_t m, int64_t nb, double *dA, int64_t lda, double *d_invd,
                                   int32_t *d_info, int64_t info_base)
{
    CTX_ENTER(c);
    if (nb <= 0 || nb % 128 || m < nb || m % 16) {
        gpt_set_error("potrf_panel: need nb a multiple of 128 and m >= nb, m a multiple of 16");
        return GPT_E_ARG;
    }
    return panel_rec(c, c->stream, dA, lda, m, nb, d_invd, d_info, info_base);
}

extern "C" int gpt_dev_potrf(gpt_ctx *c, int64_t n, double *dA, int64_t lda, double *d_invd, int32_t *d_info)
{
    CTX_ENTER(c);
    return potrf_run(c, n, dA, lda, d_invd, d_info);
}

extern "C" int gpt_dev_trsm_rlt(gpt_ctx *c, int64_t m, int64_t n, const double *dL, int64_t ldl, const double *d_invd,
                                double *dB, int64_t ldb)
{
    CTX_ENTER(c);
    if (n <= 0 || n % 128 || m % 16) {
        gpt_set_error("trsm_rlt: n must be a multiple of 128 and m a multiple of 16");
        return GPT_E_ARG;
    }
    return trsm_rlt(c, c->stream, m, n, dL, ldl, d_invd, dB, ldb);
}

extern "C" int gpt_dev_copy2d(gpt_ctx *c, int64_t rows, int64_t cols, const double *d_src, int64_t lds, double *d_dst,
                              int64_t ldd)
{
    CTX_ENTER(c);
    return launch_copy2d(c->stream, rows, cols, d_src, lds, d_dst, ldd);
}

extern "C" int gpt_dev_copy2d_on(gpt_ctx *c, void *stream, int64_t rows, int64_t cols, const double *d_src, int64_t lds, double *d_dst,
                                 int64_t ldd)
{
    CTX_ENTER(c);
    return launch_copy2d(stream ? (hipStream_t)stream : c->stream, rows, cols, d_src, lds, d_dst, ldd);
}

extern "C" int gpt_dev_pad_block(gpt_ctx *c, double *dA, int64_t lda, int64_t c0, int64_t nb, int64_t n_valid,
                                 int64_t n_pad, const double *d_y, double big)
{
    CTX_ENTER(c);
    return launch_pad_block(c->stream, dA, lda, c0, nb, n_valid, n_pad, d_y, big);
}

extern "C" int gpt_dev_panel_scalars(gpt_ctx *c, const double *dP, int64_t ldp, int64_t w, int64_t zrow, double *d_acc)
{
    CTX_ENTER(c);
    return launch_panel_scalars(c->stream, dP, ldp, w, zrow, d_acc);
}
