// api_kernels.inc -- part of api.hip (ONE translation unit: included from there, in this order; the parts share struct gpt_ctx and
// static helpers).  Kernel.__call__ and compute_Kij: gpt_kpairs, gpt_kbuild, gpt_kpairs2, gpt_kbuild2 -- one body per shape of the
// result (kpairs_run, kbuild_run), taking one KParams or the two factors of a product; the entry points make the KParams.
// ------------------------------------------------------------------------------------------------
// Kernel.__call__ / compute_Kij
// ------------------------------------------------------------------------------------------------
// The pair list of k1, or of the product k1 * k2 (k2 != NULL), over M pairs of points
static int kpairs_run(gpt_ctx *c, const KParams &k1, const KParams *k2, const double *Xi, const double *Xj, const int32_t *ni,
                      const int32_t *nj, int64_t M, int D, double *out)
{
    if (M < 0 || (M > 0 && (!Xi || !Xj || !ni || !nj || !out))) return GPT_E_ARG;
    if (M == 0) return GPT_OK;
    GPT_TRY(check_pair_orders(k1, k2, ni, M, nj, M, D, true));
    double *dXi, *dXj, *dout;
    int32_t *dni, *dnj;
    const size_t xb = (size_t)M * D * sizeof(double), nb = (size_t)M * D * sizeof(int32_t);
    GPT_TRY(ensure(c, SLOT_XI, xb, (void **)&dXi));
    GPT_TRY(ensure(c, SLOT_XJ, xb, (void **)&dXj));
    GPT_TRY(ensure(c, SLOT_NI, nb, (void **)&dni));
    GPT_TRY(ensure(c, SLOT_NJ, nb, (void **)&dnj));
    GPT_TRY(ensure(c, SLOT_OUT, (size_t)M * sizeof(double), (void **)&dout));
    hipStream_t st = c->stream;
    GPT_HIP_CHECK(hipMemcpyAsync(dXi, Xi, xb, hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dXj, Xj, xb, hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dni, ni, nb, hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dnj, nj, nb, hipMemcpyHostToDevice, st));
    GPT_TRY(launch_kpairs(st, k1, dXi, dXj, dni, dnj, M, dout, 0, k2));
    GPT_HIP_CHECK(hipMemcpyAsync(out, dout, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}

// With warp layers set (gpt_set_warp) a Gram block's uploaded points are warped in place, their slope factors go to two slots of
// their own; the builder then takes the WARP instantiation.
static int warp_kbuild_check(const gpt_ctx *c, const int32_t *ni, int64_t M, const int32_t *nj, int64_t P, int D)
{
    if (D != c->warp.D) {
        gpt_set_error("kbuild: the warp layers are set for num_dim %d, the points have %d", c->warp.D, D);
        return GPT_E_ARG;
    }
    GPT_TRY(check_warp_orders(ni, M, D));
    return check_warp_orders(nj, P, D);
}

static int warp_kbuild_points(gpt_ctx *c, hipStream_t st, double *dXi, const int32_t *dni, int64_t M, double *dXj,
                              const int32_t *dnj, int64_t P, double **dSi, double **dSj)
{
    GPT_TRY(ensure(c, SLOT_SI, (size_t)M * sizeof(double), (void **)dSi));
    GPT_TRY(ensure(c, SLOT_SJ, (size_t)P * sizeof(double), (void **)dSj));
    GPT_TRY(launch_warp_points(st, c->warp, dXi, dni, M, dXi, *dSi));
    return launch_warp_points(st, c->warp, dXj, dnj, P, dXj, *dSj);
}

// The M x P Gram block of k1, or of the product k1 * k2 (k2 != NULL); Xj == NULL: of Xi with itself.
// Contract for an EMPTY block (M == 0 or P == 0), the same for gpt_kbuild and gpt_kbuild2: the parameters are checked (by the
// caller, in front of this), the points are not -- there is no pair that could break an order rule, and the call returns GPT_OK
// without touching K_out.
static int kbuild_run(gpt_ctx *c, const KParams &k1, const KParams *k2, const double *Xi, const int32_t *ni, int64_t M,
                      const double *Xj, const int32_t *nj, int64_t P, int D, double *K_out)
{
    if (!Xj) {
        Xj = Xi;
        nj = ni;
        P = M;
    }
    if (M < 0 || P < 0) return GPT_E_ARG;
    if (M == 0 || P == 0) return GPT_OK;
    if (!Xi || !ni || !Xj || !nj || !K_out) return GPT_E_ARG;
    GPT_TRY(check_pair_orders(k1, k2, ni, M, nj, P, D, false));
    const bool warp = c->warp.nlayers > 0 && native_fit_kernel(k1.kernel_id);      // (the noise kernels are never warped)
    if (warp) GPT_TRY(warp_kbuild_check(c, ni, M, nj, P, D));
    double *dXi, *dXj, *dK, *dSi = nullptr, *dSj = nullptr;
    int32_t *dni, *dnj;
    GPT_TRY(ensure(c, SLOT_XI, (size_t)M * D * sizeof(double), (void **)&dXi));
    GPT_TRY(ensure(c, SLOT_NI, (size_t)M * D * sizeof(int32_t), (void **)&dni));
    GPT_TRY(ensure(c, SLOT_XJ, (size_t)P * D * sizeof(double), (void **)&dXj));
    GPT_TRY(ensure(c, SLOT_NJ, (size_t)P * D * sizeof(int32_t), (void **)&dnj));
    GPT_TRY(ensure(c, SLOT_OUT, (size_t)M * P * sizeof(double), (void **)&dK));
    hipStream_t st = c->stream;
    GPT_HIP_CHECK(hipMemcpyAsync(dXi, Xi, (size_t)M * D * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dni, ni, (size_t)M * D * sizeof(int32_t), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dXj, Xj, (size_t)P * D * sizeof(double), hipMemcpyHostToDevice, st));
    GPT_HIP_CHECK(hipMemcpyAsync(dnj, nj, (size_t)P * D * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (warp) GPT_TRY(warp_kbuild_points(c, st, dXi, dni, M, dXj, dnj, P, &dSi, &dSj));
    GPT_TRY(launch_kbuild(st, k1, k2, {dXi, dni, M, dXj, dnj, P, 0, 0, 0, nullptr, 0.0, 0.0, dK, P, 0, dSi, dSj}));
    GPT_HIP_CHECK(hipMemcpyAsync(K_out, dK, (size_t)M * P * sizeof(double), hipMemcpyDeviceToHost, st));
    GPT_HIP_CHECK(hipStreamSynchronize(st));
    return GPT_OK;
}

extern "C" int gpt_kpairs(gpt_ctx *c, int kernel_id, const double *params, int nparams, const double *Xi,
                          const double *Xj, const int32_t *ni, const int32_t *nj, int64_t M, int D,
                          int hyper_deriv, int symmetric, const int32_t *noise_n, double *out)
{
    CTX_ENTER(c);
    if (!params) return GPT_E_ARG;
    KParams kp;
    GPT_TRY(make_kparams(kernel_id, params, nparams, D, hyper_deriv, symmetric, noise_n, &kp));
    return kpairs_run(c, kp, nullptr, Xi, Xj, ni, nj, M, D, out);
}

extern "C" int gpt_kbuild(gpt_ctx *c, int kernel_id, const double *params, int nparams, const double *Xi,
                          const int32_t *ni, int64_t M, const double *Xj, const int32_t *nj, int64_t P, int D,
                          int hyper_deriv, const int32_t *noise_n, double *K_out)
{
    CTX_ENTER(c);
    if (!params) return GPT_E_ARG;
    KParams kp;
    GPT_TRY(make_kparams(kernel_id, params, nparams, D, hyper_deriv, Xj == nullptr, noise_n, &kp));
    return kbuild_run(c, kp, nullptr, Xi, ni, M, Xj, nj, P, D, K_out);
}

// Kernel.__call__ / compute_Kij of the product of two native kernels (ProductKernel, ref: kernel/core.py:587-671)
static int make_product(int kid1, const double *p1, int n1, int kid2, const double *p2, int n2, int D, KParams *k1, KParams *k2)
{
    if (!p1 || !p2) return GPT_E_ARG;
    if (!native_fit_kernel(GPT_KERNEL_BASE_ID(kid1)) || !native_fit_kernel(GPT_KERNEL_BASE_ID(kid2))) {
        gpt_set_error("product factors must be SE, Matern52, RationalQuadratic, Matern or Gibbs kernels");
        return GPT_E_ARG;
    }
    GPT_TRY(make_kparams(kid1, p1, n1, D, -1, 0, nullptr, k1, true));
    return make_kparams(kid2, p2, n2, D, -1, 0, nullptr, k2, true);
}

extern "C" int gpt_kpairs2(gpt_ctx *c, int kernel_id1, const double *params1, int nparams1, int kernel_id2,
                           const double *params2, int nparams2, const double *Xi, const double *Xj, const int32_t *ni,
                           const int32_t *nj, int64_t M, int D, double *out)
{
    CTX_ENTER(c);
    KParams k1, k2;
    GPT_TRY(make_product(kernel_id1, params1, nparams1, kernel_id2, params2, nparams2, D, &k1, &k2));
    return kpairs_run(c, k1, &k2, Xi, Xj, ni, nj, M, D, out);
}

extern "C" int gpt_kbuild2(gpt_ctx *c, int kernel_id1, const double *params1, int nparams1, int kernel_id2,
                           const double *params2, int nparams2, const double *Xi, const int32_t *ni, int64_t M,
                           const double *Xj, const int32_t *nj, int64_t P, int D, double *K_out)
{
    CTX_ENTER(c);
    KParams k1, k2;
    GPT_TRY(make_product(kernel_id1, params1, nparams1, kernel_id2, params2, nparams2, D, &k1, &k2));
    return kbuild_run(c, k1, &k2, Xi, ni, M, Xj, nj, P, D, K_out);
}
