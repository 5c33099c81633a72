// grad_stencil.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  The stencil of a differenced gradient, read in ONE place for gpt_ll_grad_diff, gpt_loo_grad_diff,
// gpt_ll_grad_diff_batch, gpt_sparse_grad_diff and gpt_dev_sparse_grad_pairs: entry h is term term_idx[h] of a model with the term's
// complete parameter vector at the two stencil points a and b.  Every stencil point goes through parse_model as a one-term model with
// the ids and parameter counts the fit was given -- whatever the fit refuses is refused here, before anything is launched -- and the
// entries are laid out term by term, because the parameters of one launch belong to one term.  Needs nothing of the device: KParams,
// ModelKernel and parse_model (api_kparams.inc) only.
struct GradStencil {
    std::vector<KParams> kp1, kp2;      // [a, b] per entry in launch order (kp2: the second factors; kernel_id < 0 where the term is no product)
    std::vector<int> where, term_of;    // the caller's index h of each entry in launch order, and its term
    std::vector<size_t> off;            // entry h's parameters start at params_a / params_b + off[h]; off[nh]: the doubles of one stencil
};

// Launch order and offsets of nh entries.  Checked here, entry by entry in the caller's order: term_idx[h], then (denom given) denom[h].
static int grad_stencil_layout(const char *who, const ModelKernel &m, int nh, const int *term_idx, const double *denom, GradStencil *s)
{
    s->off.assign((size_t)nh + 1, 0);
    for (int h = 0; h < nh; h++) {
        if (term_idx[h] < 0 || term_idx[h] >= m.nterms) return GPT_E_ARG;
        if (denom && (!(denom[h] != 0.0) || std::isinf(denom[h]))) {
            gpt_set_error("%s: denom[%d] = %g", who, h, denom[h]);
            return GPT_E_ARG;
        }
        s->off[h + 1] = s->off[h] + (size_t)m.np[term_idx[h]];
    }
    for (int t = 0; t < m.nterms; t++)
        for (int h = 0; h < nh; h++)
            if (term_idx[h] == t) {
                s->where.push_back(h);
                s->term_of.push_back(t);
            }
    return GPT_OK;
}

// The stencil points a, b of one entry of term t (its parameter vectors pa, pb) into f1[0 .. 1] and f2[0 .. 1]: the only parse_model of
// a stencil point.  D, maxsum, colmax: the order rules the points of the pass are held to.
static int grad_stencil_entry(int D, long maxsum, const long *colmax, const ModelKernel &m, int t, const double *pa, const double *pb,
                              KParams *f1, KParams *f2)
{
    const bool prod = m.abi_id2[t] >= 0;
    int s = 0;
    for (const double *p : {pa, pb}) {
        ModelKernel one;
        GPT_TRY(parse_model(D, maxsum, colmax, 1, &m.abi_id1[t], prod ? &m.abi_id2[t] : nullptr, p, &m.np[t], prod ? &m.np1[t] : nullptr, &one));
        f1[s] = one.f1[0];
        f2[s] = one.f2[0];
        s++;
    }
    return GPT_OK;
}

// Layout, then every entry in launch order.  denom NULL: not checked (the caller has none, or checks its own).
static int grad_stencil_build(const char *who, int D, long maxsum, const long *colmax, const ModelKernel &m, int nh, const int *term_idx,
                              const double *params_a, const double *params_b, const double *denom, GradStencil *s)
{
    GPT_TRY(grad_stencil_layout(who, m, nh, term_idx, denom, s));
    for (size_t idx = 0; idx < s->where.size(); idx++) {
        KParams f1[2], f2[2];
        const size_t o = s->off[s->where[idx]];
        GPT_TRY(grad_stencil_entry(D, maxsum, colmax, m, s->term_of[idx], params_a + o, params_b + o, f1, f2));
        s->kp1.insert(s->kp1.end(), f1, f1 + 2);
        s->kp2.insert(s->kp2.end(), f2, f2 + 2);
    }
    return GPT_OK;
}

// The launch groups in launch order: fn(b0, cnt, t) for the entries [b0, b0 + cnt) -- one term t, GPT_GRAD_MAXH at most.  The first
// status other than GPT_OK ends the walk and is returned.  No entries: no call.
template <class F>
static int for_each_group(const GradStencil &s, F &&fn)
{
    const int total = (int)s.where.size();
    for (int b0 = 0; b0 < total;) {
        const int t = s.term_of[b0];
        int cnt = 0;
        while (b0 + cnt < total && cnt < GPT_GRAD_MAXH && s.term_of[b0 + cnt] == t) cnt++;
        GPT_TRY(fn(b0, cnt, t));
        b0 += cnt;
    }
    return GPT_OK;
}
