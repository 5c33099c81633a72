// api_grad_batch.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  gpt_ll_grad_diff_batch: the gradient half of a resident batch.
// ------------------------------------------------------------------------------------------------
// gpt_ll_grad_diff for every element of the batch the last gpt_fit_batch* left resident
// ------------------------------------------------------------------------------------------------
// A multi-start optimiser asks for value + gradient at one point per start (GaussianProcess.ll_gradient_batch under
// gptools_amd/multistart.py); at N of a few hundred to a few thousand one gpt_ll_grad_diff is, like one fit, a chain of latency-bound
// launches and one host synchronisation per launch group.  Here every launch carries the batch in a grid dimension, as in the
// batched fit, and the host synchronises once.  Per element b, from the factor L_b in SLOT_BATCH_A and the leaves' packed
// workspaces in SLOT_BATCH_WS (both only read: the batch stays resident, gpt_predict_batch returns what it returned before):
//   U_b = L_b^-T       the right-solve X L^T = I, left-looking over the 128-column leaves like gpt_predict_batch's V = K*^T L^-T with
//                      K* = I: leaf j first takes the update of all leaves before it (one batched GEMM), then the panel TRSM against
//                      the workspace the fit left.  U is upper triangular, so leaf j has rows [0, 128 j + 128) only and the update
//                      rows [0, 128 j): half the flops of the dense solve.
//   W_b = U_b U_b^T    lower triangle, 512 block rows: the rectangle left of the diagonal block and the diagonal block as a
//                      triangular launch, k from the block row's first column on (U holds zeros before it).
//   alpha_b = U_b z_b  z_b = L_b^-1 y_b the augmented row (kgrad_batch_alpha_kernel).
//   the pair pass      kgrad_diff_kernel with the element as the grid's second dimension, GPT_GRAD_MAXH parameters of one term per
//                      launch, and the sum of the per-workgroup partial rows in index order on the device.
// The factor is the AUGMENTED one, order NP: row N holds [z_b^T, d] with d^2 = 1e300 - z^T z, the rows behind it a unit diagonal.
// The leading N x N block of its inverse transpose is L_b^-T, which is all the pair pass and alpha read (rows and columns < N).
// Column N of U holds -(U_b z_b) / d, some 1e-150 of alpha, and the columns behind it exact zeros in the rows < N (the padding
// rows of the factor are zero left of their diagonal): in U U^T they add (alpha alpha^T) 1e-300 to entries of order one -- nothing
// representable -- so the products run over all NP columns and nothing is cleared first.
// PER-ELEMENT INDEPENDENCE: every launch has the geometry of ONE element (launch_gemm_nt picks its tiles by the single matrix, no
// GEMM is split along k, the pair pass and both reductions know the element's own data only), so an element's gradient does not
// depend on nbatch, on its place in the batch or on its neighbours -- the promise the batched fit makes for ll.
// An element with keep[b] == 0 (its factor is not positive definite or holds NaN) still rides along -- with the stencil of the first
// kept element, so that no parameter of a point the fit refused reaches a kernel -- and its rows come back as NaN.
extern "C" int gpt_ll_grad_diff_batch(gpt_ctx *c, int nh, const int *term_idx, const double *params_a, const double *params_b,
                                      const double *denom, const int32_t *keep, double *out, double *alpha_out)
{
    CTX_ENTER(c);
    GPT_TRY(refuse_warp(c, "gpt_ll_grad_diff_batch"));
    if (c->rb_warped && c->rb_nbatch > 0 && c->rb_gen == c->batch_gen) {
        gpt_set_error("gpt_ll_grad_diff_batch is not available for a batch that was fitted with warps (gpt_set_warp_batch)");
        return GPT_E_NOTIMPL;
    }
    if (c->rb_nbatch <= 0 || c->rb_gen != c->batch_gen) {
        gpt_set_error("gpt_ll_grad_diff_batch: no batch resident (call gpt_fit_batch* first; gpt_set_data, gpt_set_T, gpt_cov_sample and "
                      "gpt_release_batch_scratch end its residency)");
        return GPT_E_STATE;
    }
    if (c->dT) {
        gpt_set_error("gpt_ll_grad_diff_batch: not implemented with a linear transform (gpt_set_T)");
        return GPT_E_NOTIMPL;
    }
    if (nh < 0 || (nh > 0 && (!term_idx || !params_a || !params_b || !denom)) || !keep || !out) {
        gpt_set_error("gpt_ll_grad_diff_batch: bad arguments");
        return GPT_E_ARG;
    }
    const ModelKernel &m = c->rb_model;
    const int nbatch = c->rb_nbatch, nout = nh + 1;
    const int64_t N = c->rb_N, NP = round_up(N + 1, 128), nleaf = NP / 128, bs = NP * NP, bws = nleaf * GPT_WS_BLOCK;
    const double qnan = NAN;
    // the entries term by term, GPT_GRAD_MAXH of one term to a launch group (nh == 0: one group for the trace, which reads no KParams)
    // (the steps are the elements' own, denom[b][h]: checked below, element by element, as the stencil points are parsed)
    GradStencil gs;
    GPT_TRY(grad_stencil_layout("gpt_ll_grad_diff_batch", m, nh, term_idx, nullptr, &gs));
    const std::vector<int> &where = gs.where, &term_of = gs.term_of;
    const std::vector<size_t> &off = gs.off;
    struct Group { int first, cnt, term; };
    std::vector<Group> groups;
    for_each_group(gs, [&](int b0, int cnt, int t) {
        groups.push_back(Group{b0, cnt, t});
        return GPT_OK;
    });
    if (groups.empty()) groups.push_back(Group{0, 0, 0});
    std::vector<int> group_of((size_t)nh, 0);
    std::vector<int32_t> src((size_t)round_up(nout, 2), 0);
    for (size_t g = 0; g < groups.size(); g++)
        for (int q = 0; q < groups[g].cnt; q++) {
            group_of[groups[g].first + q] = (int)g;
            src[where[groups[g].first + q]] = (int32_t)(g * (GPT_GRAD_MAXH + 1) + (size_t)q);
        }
    src[nh] = GPT_GRAD_MAXH;                                    // the noise trace: slot GPT_GRAD_MAXH of the first group
    // every stencil point of every kept element through parse_model, before anything is launched.  Device layout: group after
    // group, within a group [element][2 cnt]: the stencil points a, b of its parameters (kp2: the second factors, same layout)
    const size_t nk = (size_t)nbatch * 2 * (size_t)(nh > 0 ? nh : 1);
    std::vector<KParams> kp((m.any_prod ? 2 : 1) * nk);
    auto at = [&](int b, int idx, int s) {
        const Group &g = groups[group_of[idx]];
        return (size_t)nbatch * 2 * (size_t)g.first + (size_t)b * 2 * (size_t)g.cnt + 2 * (size_t)(idx - g.first) + (size_t)s;
    };
    int first_kept = -1;
    for (int b = 0; b < nbatch; b++) {
        if (!keep[b]) continue;
        if (first_kept < 0) first_kept = b;
        for (int idx = 0; idx < nh; idx++) {
            const int h = where[idx], t = term_of[idx];
            const double dn = denom[(size_t)b * nh + h];
            if (!(dn != 0.0) || std::isinf(dn)) {
                gpt_set_error("gpt_ll_grad_diff_batch: denom[%d][%d] = %g", b, h, dn);
                return GPT_E_ARG;
            }
            KParams f1[2], f2[2];
            const size_t o = (size_t)b * off[nh] + off[h];
            GPT_TRY(grad_stencil_entry(c->D, c->n_maxsum, c->n_colmax, m, t, params_a + o, params_b + o, f1, f2));
            for (int s = 0; s < 2; s++) {
                kp[at(b, idx, s)] = f1[s];
                if (m.any_prod) kp[nk + at(b, idx, s)] = f2[s];
            }
        }
    }
    for (int b = 0; b < nbatch; b++) {
        for (int j = 0; j < nout; j++) out[(size_t)b * nout + j] = qnan;
        if (alpha_out)
            for (int64_t i = 0; i < N; i++) alpha_out[(size_t)b * N + i] = qnan;
    }
    if (first_kept < 0) return GPT_OK;                          // nothing to evaluate
    for (int b = 0; b < nbatch; b++)
        if (!keep[b])
            for (int idx = 0; idx < nh; idx++)
                for (int s = 0; s < 2; s++) {
                    kp[at(b, idx, s)] = kp[at(first_kept, idx, s)];
                    if (m.any_prod) kp[nk + at(b, idx, s)] = kp[nk + at(first_kept, idx, s)];
                }
    // scratch of its own (gpt_release_batch_scratch frees it): U and W, nbatch matrices each, and one slot for the rest --
    // [src: nout int32 | KParams (| second factors) | alpha: nbatch NP | out: nbatch nout | partial rows: groups x nbatch x nblk]
    const int nblk = grad_reduce_blocks(N);
    const size_t b_src = src.size() * sizeof(int32_t), b_kp = kp.size() * sizeof(KParams);
    const size_t n_alpha = (size_t)nbatch * NP, n_out = (size_t)nbatch * nout;
    const size_t n_part = groups.size() * (size_t)nbatch * nblk * (GPT_GRAD_MAXH + 1);
    double *dU, *dW;
    char *dmisc;
    GPT_TRY(ensure(c, SLOT_GB_U, (size_t)nbatch * bs * sizeof(double), (void **)&dU));
    GPT_TRY(ensure(c, SLOT_GB_W, (size_t)nbatch * bs * sizeof(double), (void **)&dW));
    GPT_TRY(ensure(c, SLOT_GB_MISC, b_src + b_kp + (n_alpha + n_out + n_part) * sizeof(double), (void **)&dmisc));
    const int32_t *dsrc = reinterpret_cast<const int32_t *>(dmisc);
    const KParams *dkp = reinterpret_cast<const KParams *>(dmisc + b_src);
    const KParams *dkp2 = m.any_prod ? dkp + nk : nullptr;
    double *dalpha = reinterpret_cast<double *>(dmisc + b_src + b_kp), *dout = dalpha + n_alpha, *dpart = dout + n_out;
    std::vector<char> hin(b_src + b_kp);
    memcpy(hin.data(), src.data(), b_src);
    memcpy(hin.data() + b_src, kp.data(), b_kp);
    const double *dA = (const double *)c->slots[SLOT_BATCH_A].p, *dws = (const double *)c->slots[SLOT_BATCH_WS].p;
    EvalScope scope(c, true);
    hipStream_t st = c->panel_stream;                      // (unmasked, as the batched fit and gpt_predict_batch)
    GPT_TRY(stream_follows(c, c->stream, st, 0));
    GPT_HIP_CHECK(hipMemcpyAsync(dmisc, hin.data(), hin.size(), hipMemcpyHostToDevice, st));
    // U_b = L_b^-T
    GPT_TRY(launch_zero2d(st, (int64_t)nbatch * NP, NP, dU, NP));
    hipLaunchKernelGGL(eye_blocks_kernel, dim3((unsigned)((NP + 255) / 256), (unsigned)nbatch), dim3(256), 0, st, dU, NP, NP, bs);
    GPT_LAUNCH_CHECK();
    for (int64_t lc = 0; lc < NP; lc += 128) {
        if (lc > 0)
            GPT_TRY(launch_gemm_nt(st, lc, 128, lc, -1.0, dU, NP, dA + lc * NP, NP, 0.0, dU + lc, NP, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                                   EdgeSig(), 0, nbatch, bs, EdgeSig(), bs, bs));
        GPT_TRY(launch_trsm_panel(st, lc + 128, nullptr, 0, dws + (lc / 128) * GPT_WS_BLOCK, dU + lc, NP, nullptr, EdgeSig(), nbatch, bs, bws));
    }
    // W_b = U_b U_b^T, lower triangle
    const int64_t nb = 512;
    for (int64_t r0 = 0; r0 < NP; r0 += nb) {
        const int64_t rows = (NP - r0 < nb) ? NP - r0 : nb;
        const double *Ur = dU + r0 * NP + r0;
        if (r0 > 0)
            GPT_TRY(launch_gemm_nt(st, rows, r0, NP - r0, 1.0, Ur, NP, dU + r0, NP, 0.0, dW + r0 * NP, NP, 0, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                                   EdgeSig(), 0, nbatch, bs, EdgeSig(), bs, bs));
        GPT_TRY(launch_gemm_nt(st, rows, rows, NP - r0, 1.0, Ur, NP, Ur, NP, 0.0, dW + r0 * NP + r0, NP, 1, 0, 0, nullptr, nullptr, 0, EdgeSig(),
                               EdgeSig(), 0, nbatch, bs, EdgeSig(), bs, bs));
    }
    GPT_TRY(launch_kgrad_batch_alpha(st, dU, NP, bs, dA, NP, bs, N, nbatch, dalpha, NP));
    // the pair pass, group by group, and the sums
    for (size_t g = 0; g < groups.size(); g++) {
        const int t = groups[g].term;
        const size_t o = (size_t)nbatch * 2 * (size_t)groups[g].first;
        GPT_TRY(launch_kgrad_diff(st, m.f1[t].kernel_id, m.second(t) ? m.f2[t].kernel_id : -1, c->D, dkp + o, m.second(t) ? dkp2 + o : nullptr,
                                  groups[g].cnt, c->dX, c->dn, N, dalpha, dW, NP, dpart + g * (size_t)nbatch * nblk * (GPT_GRAD_MAXH + 1), nbatch));
    }
    GPT_TRY(launch_kgrad_batch_finish(st, dpart, dsrc, nout, nblk, nbatch, dout));
    std::vector<double> hout(n_out), halpha(alpha_out ? n_alpha : 0);
    GPT_HIP_CHECK(hipMemcpyAsync(hout.data(), dout, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
    if (alpha_out) GPT_HIP_CHECK(hipMemcpyAsync(halpha.data(), dalpha, n_alpha * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < nbatch; b++) {
        if (!keep[b]) continue;
        for (int h = 0; h < nh; h++) out[(size_t)b * nout + h] = hout[(size_t)b * nout + h] / denom[(size_t)b * nh + h];
        out[(size_t)b * nout + nh] = hout[(size_t)b * nout + nh];
        if (alpha_out) memcpy(alpha_out + (size_t)b * N, halpha.data() + (size_t)b * NP, (size_t)N * sizeof(double));
    }
    return GPT_OK;
}
