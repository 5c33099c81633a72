// api_kparams.inc -- part of api.hip (ONE translation unit: included from there, in front of struct gpt_ctx, which holds a
// ModelKernel by value; nothing here reads the context).  The model kernel and what the entry points check about it:
// make_kparams (one native kernel's parameters -> KParams), ModelKernel + parse_model (a sum of native kernels and products of
// two, from the id / parameter-count arrays of the ABI), and the derivative-order rules -- the primitives check_m52_orders,
// check_rq_orders, check_gibbs_orders, check_warp_orders and, built on them, ONE function per family of entry points:
// check_train_orders (the fits), check_test_orders (the predictions), check_pair_orders (gpt_kpairs* / gpt_kbuild*).
// ------------------------------------------------------------------------------------------------
// factor: the kernel is a factor of a product -- the only place of a GPT_KERNEL_ON_DIM id
static int make_kparams(int kernel_id, const double *params, int nparams, int D, int hyper_deriv, int symmetric,
                        const int32_t *noise_n, KParams *kp, bool factor = false)
{
    if (D < 1 || D > GPT_MAX_DIM) {
        gpt_set_error("num_dim %d out of range [1, %d]", D, GPT_MAX_DIM);
        return GPT_E_ARG;
    }
    // GPT_KERNEL_ON_DIM(id, d): a 1-D Gibbs kernel on coordinate d of num_dim <= GPT_GIBBS_ON_DIM_MAX_D (a product factor: the
    // builders have that form only as GPT_KID_PRODUCT_GM / _GB, kbuild_kernel.hpp).  From here on kernel_id is the plain id
    const int on_dim = GPT_KERNEL_DIM_OF(kernel_id);
    if (on_dim >= 0) {
        kernel_id = GPT_KERNEL_BASE_ID(kernel_id);
        if (!factor) {
            gpt_set_error("kernel %d on coordinate %d: a Gibbs kernel on one coordinate is a product factor (on its own: times SE [1, inf ..])",
                          kernel_id, on_dim);
            return GPT_E_ARG;
        }
        if (!gibbs_kid(kernel_id)) {
            gpt_set_error("kernel %d: only a Gibbs kernel id carries a coordinate (GPT_KERNEL_ON_DIM)", kernel_id);
            return GPT_E_ARG;
        }
        if (D > GPT_GIBBS_ON_DIM_MAX_D) {
            gpt_set_error("a Gibbs kernel on one coordinate needs num_dim <= %d, got %d", GPT_GIBBS_ON_DIM_MAX_D, D);
            return GPT_E_ARG;
        }
        if (on_dim >= D) {
            gpt_set_error("kernel %d on coordinate %d of num_dim %d", kernel_id, on_dim, D);
            return GPT_E_ARG;
        }
    }
    memset(kp, 0, sizeof(*kp));
    kp->kernel_id = kernel_id;
    kp->g_dim = on_dim >= 0 ? on_dim : 0;
    kp->D = D;
    kp->hyper_deriv = hyper_deriv < 0 ? -1 : hyper_deriv;
    kp->symmetric = symmetric ? 1 : 0;
    if (kernel_id == GPT_KERNEL_SE || kernel_id == GPT_KERNEL_M52) {
        if (nparams != D + 1) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, D + 1, nparams);
            return GPT_E_ARG;
        }
        if (kernel_id == GPT_KERNEL_M52 && hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");
            return GPT_E_NOTIMPL;
        }
        if (hyper_deriv >= nparams) {
            gpt_set_error("hyper_deriv %d out of range", hyper_deriv);
            return GPT_E_ARG;
        }
        kp->sigma = params[0];
        for (int d = 0; d < D; d++) {
            const double l = params[1 + d];
            kp->l[d] = l;
            kp->inv_l[d] = 1.0 / l;
            kp->inv_var[d] = 1.0 / (l * l);
            // (from the value the pair functions multiply by: a SUBNORMAL length scale has 1 / l = inf as well, and 0 * inf on the
            // diagonal / for coincident points would be NaN where the reference divides 0 / l = 0, core.py:416 -- ADVICE r4)
            if (l == 0.0 || std::isinf(kp->inv_l[d])) kp->zero_l = 1;
        }
    } else if (kernel_id == GPT_KERNEL_RQ) {
        // RationalQuadraticKernel: [sigma_f, alpha, l_1 .. l_D] (ref: rational_quadratic.py:30-45)
        if (nparams != D + 2) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, D + 2, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: core.py:723-726
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        kp->alpha = params[1];
        for (int d = 0; d < D; d++) {
            const double l = params[2 + d];
            kp->l[d] = l;
            kp->inv_l[d] = 1.0 / l;
            kp->inv_var[d] = 1.0 / (l * l);
        }
    } else if (kernel_id == GPT_KERNEL_MATERN) {
        // MaternKernel: [sigma_f, nu, l_1 .. l_D] (ref: matern.py:299-306); the Gamma-function constants the device code
        // needs (Temme's series, the reference's small-y series at nu or nu -+ 0.001) are formed here, in libm
        if (nparams != D + 2) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, D + 2, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: core.py:723-726
            return GPT_E_NOTIMPL;
        }
        const double nu = params[1];
        if (!(nu > 0.0) || !(nu < 60.0)) {
            gpt_set_error("MaternKernel: the order nu must lie in (0, 60), got %g", nu);
            return GPT_E_VALUE;
        }
        kp->sigma = params[0];
        kp->alpha = nu;
        for (int d = 0; d < D; d++) {
            const double l = params[2 + d];
            kp->l[d] = l;
            kp->inv_l[d] = 1.0 / l;
            kp->inv_var[d] = 1.0 / (l * l);
            if (std::isinf(l)) kp->inf_l = 1;      // (matern_pair's guard for an order in a masked-out dimension, kpair.hpp)
        }
        kp->m_cnu = pow(2.0, 1.0 - nu) / tgamma(nu);
        kp->m_nint = (int)floor(nu + 0.5);
        kp->m_mu = nu - (double)kp->m_nint;
        kp->m_isint = (nu == floor(nu)) ? 1 : 0;
        {
            const double mu = kp->m_mu, mu2 = mu * mu;
            kp->m_gampl = 1.0 / tgamma(1.0 + mu);
            kp->m_gammi = 1.0 / tgamma(1.0 - mu);
            kp->m_gam2 = 0.5 * (kp->m_gammi + kp->m_gampl);
            // (1/Gamma(1-mu) - 1/Gamma(1+mu)) / (2 mu); near mu = 0 from the Taylor series of 1/Gamma(1+t)
            kp->m_gam1 = (fabs(mu) < 1.0e-3)
                             ? -(0.57721566490153286 + mu2 * (-0.042002635034095236 + mu2 * (-0.0072189432466630995)))
                             : (kp->m_gammi - kp->m_gampl) / (2.0 * mu);
        }
        for (int q = 0; q < 2; q++) {
            const double nus = kp->m_isint ? nu + (q == 0 ? -0.001 : 0.001) : nu;      // utils.py:1481-1483 (nu_step)
            kp->m_nus[q] = nus;
            kp->m_g[q] = tgamma(nus);
            kp->m_gm[q] = tgamma(-nus);
        }
    } else if (kernel_id == GPT_KERNEL_GIBBS_TANH || kernel_id == GPT_KERNEL_GIBBS_DTANH) {
        // GibbsKernel1dTanh [sigma_f, l_1, l_2, l_w, x_0] (ref: gibbs.py:426-498); GibbsKernel1dDoubleTanh [sigma_f, l_c, l_m,
        // l_e, l_a, l_b, x_a, x_b] (ref: gibbs.py:508-590).  Both as l(x) = g_c + sum_q g_amp[q] tanh((x - g_x0[q]) / g_w[q])
        const bool dbl = kernel_id == GPT_KERNEL_GIBBS_DTANH;
        if (D != 1 && on_dim < 0) {
            gpt_set_error("Gibbs kernel only supports 1d data.");
            return GPT_E_ARG;
        }
        if (nparams != (dbl ? 8 : 5)) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, dbl ? 8 : 5, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: gibbs.py:319-322
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        if (!dbl) {
            const double l1 = params[1], l2 = params[2];
            kp->g_nt = 1;
            kp->g_c = (l1 + l2) / 2.0;
            kp->g_amp[0] = -((l1 - l2) / 2.0);
            kp->g_w[0] = params[3];
            kp->g_x0[0] = params[4];
        } else {
            // the reference's a, b, c: dot([[-0.5, 0, 0.5], [0, 0.5, -0.5], [0.5, 0.5, 0]], [l_c, l_e, l_m]) (gibbs.py:546-551)
            const double lc = params[1], lm = params[2], le = params[3];
            kp->g_nt = 2;
            kp->g_amp[0] = -0.5 * lc + 0.0 * le + 0.5 * lm;
            kp->g_amp[1] = 0.0 * lc + 0.5 * le - 0.5 * lm;
            kp->g_c = 0.5 * lc + 0.5 * le + 0.0 * lm;
            kp->g_w[0] = params[4];
            kp->g_w[1] = params[5];
            kp->g_x0[0] = params[6];
            kp->g_x0[1] = params[7];
        }
    } else if (kernel_id == GPT_KERNEL_GIBBS_CUBIC || kernel_id == GPT_KERNEL_GIBBS_QUINTIC || kernel_id == GPT_KERNEL_GIBBS_EXPGAUSS) {
        // GibbsKernel1dCubicBucket / GibbsKernel1dQuinticBucket [sigma_f, l_1, l_2, l_3, x_0, w_1, w_2, w_3] (ref: gibbs.py:603-801);
        // GibbsKernel1dExpGauss [sigma_f, l_0, mu_1..G, sigma_1..G, beta_1..G] (ref: gibbs.py:804-902).  The parameters after
        // sigma_f go to the device as they are (gibbs_lfunc.hpp forms l and l' from them in the reference's order of operations)
        const bool eg = kernel_id == GPT_KERNEL_GIBBS_EXPGAUSS;
        if (D != 1 && on_dim < 0) {
            gpt_set_error("Gibbs kernel only supports 1d data.");
            return GPT_E_ARG;
        }
        if (eg) {
            if (nparams < 5 || (nparams - 2) % 3 != 0) {
                gpt_set_error("kernel %d expects 3 G + 2 params (G >= 1 Gaussians), got %d", kernel_id, nparams);
                return GPT_E_ARG;
            }
            if ((nparams - 2) / 3 > GPT_GIBBS_MAX_GAUSS) {
                gpt_set_error("kernel %d: %d Gaussians, the device kernel takes GPT_GIBBS_MAX_GAUSS = %d at most", kernel_id,
                              (nparams - 2) / 3, GPT_GIBBS_MAX_GAUSS);
                return GPT_E_ARG;
            }
        } else if (nparams != 8) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, 8, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: gibbs.py:319-322
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        kp->g_nt = eg ? (nparams - 2) / 3 : 0;
        for (int q = 1; q < nparams; q++) kp->g_raw[q - 1] = params[q];
    } else if (kernel_id == GPT_KERNEL_GIBBS_BSPLINE) {
        // GibbsKernel1dBSpline, cubic [sigma_f, t_1 .. t_nt, C_1 .. C_{nt+2}] (ref: gibbs.py:905-992); the ABI carries no integer
        // besides nparams, so nt = (nparams - 3) / 2.  Knots and coefficients go to the device as they are (gibbs_lfunc.hpp)
        if (D != 1 && on_dim < 0) {
            gpt_set_error("Gibbs kernel only supports 1d data.");
            return GPT_E_ARG;
        }
        const int nt = (nparams - 3) / 2;
        if (nparams < 3 || (nparams - 3) % 2 != 0 || nt < 2 || nt > GPT_GIBBS_MAX_KNOTS) {
            gpt_set_error("kernel %d expects 2 nt + 3 params (cubic, 2 <= nt <= GPT_GIBBS_MAX_KNOTS = %d knots), got %d", kernel_id,
                          GPT_GIBBS_MAX_KNOTS, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: gibbs.py:319-322
            return GPT_E_NOTIMPL;
        }
        // (ref: splines.py:54-55 compares the knots with their sorted copy, which also refuses a NaN among them)
        for (int q = 1; q < nt; q++)
            if (!(params[q] <= params[q + 1])) {
                gpt_set_error("Knots must be in increasing order!");
                return GPT_E_VALUE;
            }
        kp->sigma = params[0];
        kp->g_nt = nt;
        for (int q = 1; q < nparams; q++) kp->g_raw[q - 1] = params[q];
    } else if (kernel_id == GPT_KERNEL_GIBBS_GP) {
        // GibbsKernel1dGP with a nested 1-D squared-exponential kernel, [sigma_f, l, x_1 .. x_m, c_1 .. c_m] (ref: gibbs.py:995-1095): the
        // c_j are the nested GP's weights, solved for by the caller (gpt_hip.h); m = (nparams - 2) / 2.  As they are to the device
        if (D != 1 && on_dim < 0) {
            gpt_set_error("Gibbs kernel only supports 1d data.");
            return GPT_E_ARG;
        }
        const int m = (nparams - 2) / 2;
        if (nparams < 4 || (nparams - 2) % 2 != 0) {
            gpt_set_error("kernel %d expects 2 m + 2 params (1 <= m <= GPT_GIBBS_MAX_GP_POINTS = %d points), got %d", kernel_id,
                          GPT_GIBBS_MAX_GP_POINTS, nparams);
            return GPT_E_ARG;
        }
        if (m > GPT_GIBBS_MAX_GP_POINTS) {
            gpt_set_error("kernel %d: %d points, the device kernel takes GPT_GIBBS_MAX_GP_POINTS = %d at most", kernel_id, m,
                          GPT_GIBBS_MAX_GP_POINTS);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");      // ref: gibbs.py:319-322
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        kp->g_nt = m;
        for (int q = 1; q < nparams; q++) kp->g_raw[q - 1] = params[q];
    } else if (kernel_id == GPT_KERNEL_PERIODIC) {
        // PeriodicKernel: [sigma_f, l_1 .. l_D, p_1 .. p_D] (gpt_hip.h; periodic.hpp).  inv_var = 1 / l^2 (0 for l = +inf: the dimension
        // is masked out), inv_l = 1 / p -- the unit the argument is reduced in -- and l the raw length scale
        if (nparams != 2 * D + 1) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, 2 * D + 1, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        for (int d = 0; d < D; d++) {
            const double l = params[1 + d], p = params[1 + D + d];
            if (!std::isfinite(p) || !(p > 0.0) || std::isinf(1.0 / p)) {      // (a subnormal period: 1 / p overflows)
                gpt_set_error("PeriodicKernel: the period of dimension %d must be finite and positive, got %g", d + 1, p);
                return GPT_E_VALUE;
            }
            const double a = 1.0 / (l * l);
            if (l != l || l == 0.0 || std::isinf(a)) {
                gpt_set_error("PeriodicKernel: the length scale of dimension %d must not be NaN or zero (1 / l^2 finite), got %g", d + 1, l);
                return GPT_E_VALUE;
            }
            kp->l[d] = l;
            kp->inv_l[d] = 1.0 / p;
            kp->inv_var[d] = a;
        }
    } else if (kernel_id == GPT_KERNEL_SPECTRAL) {
        // SpectralKernel, one component of the spectral mixture: [sigma_f, mu_1 .. mu_D, l_1 .. l_D] (gpt_hip.h; spectral.hpp).
        // inv_var = 1 / l^2 (0 for l = +inf: no envelope in that dimension) and, in the place of the raw length scale, l[] = mu
        if (nparams != 2 * D + 1) {
            gpt_set_error("kernel %d expects %d params, got %d", kernel_id, 2 * D + 1, nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv >= 0) {
            gpt_set_error("Hyperparameter derivatives have not been implemented!");
            return GPT_E_NOTIMPL;
        }
        kp->sigma = params[0];
        for (int d = 0; d < D; d++) {
            const double mu = params[1 + d], l = params[1 + D + d];
            if (!std::isfinite(mu)) {
                gpt_set_error("SpectralKernel: the frequency of dimension %d must be finite, got %g", d + 1, mu);
                return GPT_E_VALUE;
            }
            const double a = 1.0 / (l * l);
            if (l != l || l == 0.0 || std::isinf(a)) {
                gpt_set_error("SpectralKernel: the length scale of dimension %d must not be NaN or zero (1 / l^2 finite), got %g", d + 1, l);
                return GPT_E_VALUE;
            }
            kp->l[d] = mu;
            kp->inv_var[d] = a;
        }
    } else if (kernel_id == GPT_KERNEL_DIAGNOISE || kernel_id == GPT_KERNEL_ZERO) {
        if (nparams != 1) {
            gpt_set_error("noise kernels expect 1 param, got %d", nparams);
            return GPT_E_ARG;
        }
        if (hyper_deriv > 0) {
            gpt_set_error("hyper_deriv %d out of range", hyper_deriv);
            return GPT_E_ARG;
        }
        kp->sigma = params[0];
        for (int d = 0; d < D; d++) kp->noise_n[d] = noise_n ? noise_n[d] : 0;
    } else {
        gpt_set_error("unknown kernel_id %d", kernel_id);
        return GPT_E_ARG;
    }
    return GPT_OK;
}

// Matern52 accepts only derivative orders summing to <= 1 per point (ref: kernel/matern.py:545-546).
static int check_m52_orders(const int32_t *n, int64_t M, int D)
{
    for (int64_t i = 0; i < M; i++) {
        long s = 0;
        for (int d = 0; d < D; d++) s += n[i * D + d];
        if (s > 1) {
            gpt_set_error("Matern52Kernel only supports 0th and 1st order derivatives");
            return GPT_E_VALUE;
        }
    }
    return GPT_OK;
}

// The device builder of the rational-quadratic kernel carries GPT_RQ_MAXORD + 1 Faa di Bruno coefficients: the derivative
// orders of any pair (row of ni + row of nj) may sum to GPT_RQ_MAXORD at most.  `pairwise`: rows are matched one to
// one (gpt_kpairs); otherwise every row of ni meets every row of nj (Gram blocks).
static int check_rq_orders(const int32_t *ni, int64_t M, const int32_t *nj, int64_t P, int D, bool pairwise)
{
    long mi = 0, mj = 0, mp = 0;
    for (int64_t i = 0; i < M; i++) {
        long s = 0;
        for (int d = 0; d < D; d++) s += ni[i * D + d];
        if (pairwise && i < P) {
            long t = s;
            for (int d = 0; d < D; d++) t += nj[i * D + d];
            if (t > mp) mp = t;
        }
        if (s > mi) mi = s;
    }
    for (int64_t j = 0; j < P && !pairwise; j++) {
        long s = 0;
        for (int d = 0; d < D; d++) s += nj[j * D + d];
        if (s > mj) mj = s;
    }
    const long worst = pairwise ? mp : mi + mj;
    if (worst > GPT_RQ_MAXORD) {
        gpt_set_error("RationalQuadraticKernel: derivative orders of a pair sum to %ld, the device builder supports %d",
                      worst, GPT_RQ_MAXORD);
        return GPT_E_VALUE;
    }
    return GPT_OK;
}

// RationalQuadratic / Matern: derivatives by the chain rule with GPT_RQ_MAXORD + 1 Faa di Bruno coefficients (check_rq_orders)
static bool is_chain(int kid)
{
    return kid == GPT_KERNEL_RQ || kid == GPT_KERNEL_MATERN;
}

// The Gibbs kernels evaluate derivative orders 0 and 1 per point (ref: gibbs.py:417-420 raises NotImplementedError beyond) -- in
// the coordinate `col` the kernel acts on (KParams::g_dim: 0 at num_dim 1, the coordinate of a GPT_KERNEL_ON_DIM factor).  The
// orders of the other coordinates belong to the other factor of the product and to its rules.
static const char *const GIBBS_ORDER_MSG = "Derivatives greater than [1, 1] are not supported!";
static int check_gibbs_orders(const int32_t *n, int64_t M, int D, int col)
{
    for (int64_t i = 0; i < M; i++)
        if (n[i * D + col] > 1) {
            gpt_set_error("%s", GIBBS_ORDER_MSG);
            return GPT_E_NOTIMPL;
        }
    return GPT_OK;
}

// warp layers set (gpt_set_warp): the chain rule w'(x) k'(w(x), .) covers orders 0 and 1 only (ref: kernel/warping.py:492-493)
static const char *const WARP_ORDER_MSG = "Derivative orders greater than one are not supported!";
static int check_warp_orders(const int32_t *n, int64_t M, int D)
{
    for (int64_t i = 0; i < M * D; i++)
        if (n[i] > 1) {
            gpt_set_error("%s", WARP_ORDER_MSG);
            return GPT_E_VALUE;
        }
    return GPT_OK;
}

// The periodic kernel runs its derivative recurrence per dimension: the COMBINED order of a pair in ONE dimension may reach
// GPT_PERIODIC_MAXORD.  mi[d] / mj[d]: the largest order of coordinate d on either side of a Gram block (pairwise lists: see
// check_pair_orders).  The spectral kernel has the same rule and the same limit (GPT_SPECTRAL_MAXORD); `who` names the kernel.
static_assert(GPT_SPECTRAL_MAXORD == GPT_PERIODIC_MAXORD, "one per-dimension limit for both kernels (check_test_orders)");
static int check_periodic_colmax(const long *mi, const long *mj, int D, const char *who = "PeriodicKernel")
{
    for (int d = 0; d < D; d++)
        if (mi[d] + mj[d] > GPT_PERIODIC_MAXORD) {
            gpt_set_error("%s: derivative orders of a pair sum to %ld in dimension %d, the device builder supports %d per dimension",
                          who, mi[d] + mj[d], d + 1, GPT_PERIODIC_MAXORD);
            return GPT_E_VALUE;
        }
    return GPT_OK;
}
// (the kernels with that rule; both live in the builders' PER forms)
static bool per_form_kid(int kid) { return kid == GPT_KERNEL_PERIODIC || kid == GPT_KERNEL_SPECTRAL; }
static const char *per_form_name(int k1, int k2)
{
    return (k1 == GPT_KERNEL_PERIODIC || k2 == GPT_KERNEL_PERIODIC) ? "PeriodicKernel" : "SpectralKernel";
}
static void order_colmax(const int32_t *n, int64_t M, int D, long *mx)
{
    for (int d = 0; d < D; d++) mx[d] = 0;
    for (int64_t i = 0; i < M; i++)
        for (int d = 0; d < D; d++)
            if (n[i * D + d] > mx[d]) mx[d] = n[i * D + d];
}
static const char *const PERIODIC_GIBBS_MSG = "a Periodic x Gibbs product is not evaluated on the device";
static const char *const SPECTRAL_GIBBS_MSG = "a Spectral x Gibbs product is not evaluated on the device";

static bool native_fit_kernel(int kid)
{
    return kid == GPT_KERNEL_SE || kid == GPT_KERNEL_M52 || is_chain(kid) || gibbs_kid(kid) || kid == GPT_KERNEL_PERIODIC || kid == GPT_KERNEL_SPECTRAL;
}

// ------------------------------------------------------------------------------------------------
// the model kernel
// ------------------------------------------------------------------------------------------------
// A sum of up to GPT_MAX_TERMS terms (SumKernel, ref: kernel/core.py:549-584), each one native kernel or the product of two
// (ProductKernel, ref: kernel/core.py:587-671).  The context holds the resident factorisation's by value (gpt_ctx::model), the
// resident batch its first element's (gpt_ctx::rb_model: ids, nterms and the product pattern are the same in every element).
#define GPT_MAX_TERMS 8
struct ModelKernel {
    int nterms = 0;
    int nparams = 0;                               // doubles one parameter set takes in the ABI's flat array (all terms, both factors)
    KParams f1[GPT_MAX_TERMS] = {}, f2[GPT_MAX_TERMS] = {};      // f2[t].kernel_id < 0: term t is not a product; zero beyond nterms
    bool any_prod = false, has_m52 = false, has_chain = false, has_gibbs = false;      // over all factors of all terms
    bool has_gb = false;      // ... a B-spline or nested-GP Gibbs kernel among them (gibbs_gb_kid): the batched launchers take the kernels with those branches
    bool has_on_dim = false;       // ... a Gibbs factor on one coordinate of num_dim > 1 (GPT_KERNEL_ON_DIM): likewise
    bool has_per = false;          // ... a Periodic or a Spectral kernel (GPT_GFORM_PER): likewise, and the per-dimension order rule of the test points
    // the terms as the ABI named them (ids with their GPT_KERNEL_ON_DIM coordinate; abi_id2 < 0: no product) and their parameter counts
    // (np: the whole term, np1: its first factor): what gpt_ll_grad_diff needs to send a stencil point of ONE term through parse_model again
    int abi_id1[GPT_MAX_TERMS] = {}, abi_id2[GPT_MAX_TERMS] = {}, np[GPT_MAX_TERMS] = {}, np1[GPT_MAX_TERMS] = {};
    int gibbs_form() const { return (has_gb ? GPT_GFORM_GB : 0) | (has_on_dim ? GPT_GFORM_ON_DIM : 0) | (has_per ? GPT_GFORM_PER : 0); }      // what those launchers take
    const KParams *second(int t) const { return f2[t].kernel_id >= 0 ? &f2[t] : nullptr; }
};

// Training points against ONE term k1 (* k2 where k2 >= 0); n_maxsum: the largest row sum of their derivative orders
// (gpt_set_data), gibbs_max1 / gibbs_max2: the largest order in the coordinate a Gibbs factor acts on (train_gibbs_max).  A Gibbs
// factor takes orders <= 1 there (1-D: the largest order IS n_maxsum); a pair of training points meets
// 2 n_maxsum in a RationalQuadratic / Matern factor, and in EITHER factor of a product (the SUM of both points' orders).  A lone
// SE or Matern52 term has no limit here (Matern52's own rule is the Python host's).
static int check_train_orders(int k1, int k2, long n_maxsum, long gibbs_max1, long gibbs_max2)
{
    if ((gibbs_kid(k1) && gibbs_max1 > 1) || (gibbs_kid(k2) && gibbs_max2 > 1)) {
        gpt_set_error("%s", GIBBS_ORDER_MSG);
        return GPT_E_NOTIMPL;
    }
    if ((is_chain(k1) || k2 >= 0) && 2 * n_maxsum > GPT_RQ_MAXORD) {
        gpt_set_error("derivative orders of a pair sum to %ld, the device builder supports %d for products and the "
                      "RationalQuadratic / Matern kernels", 2 * n_maxsum, GPT_RQ_MAXORD);
        return GPT_E_VALUE;
    }
    return GPT_OK;
}

// The ONE reader of the ABI's model arrays: term t is ids[t] with nparams[t] parameters, or -- ids2 given and ids2[t] >= 0 --
// the product ids[t] * ids2[t], the first nparams1[t] of its nparams[t] parameters the first factor's.  Term by term: ids, the
// training points' orders (check_train_orders), the parameter split, the parameters (make_kparams) -- the first refusal in that
// order is the call's status.  *m is overwritten whether or not the call succeeds: callers that keep a model parse into a local.
// the largest training order a Gibbs id meets: of its coordinate for a GPT_KERNEL_ON_DIM id inside num_dim, else of any row sum (num_dim 1:
// the same number; a plain Gibbs id at num_dim > 1 is refused by make_kparams after the order check, as it always was)
static long train_gibbs_max(int abi_id, int D, long n_maxsum, const long *n_colmax)
{
    const int d = GPT_KERNEL_DIM_OF(abi_id);
    return (d >= 0 && d < D) ? n_colmax[d] : n_maxsum;
}

// n_colmax[d]: the largest training order of coordinate d (gpt_set_data)
static int parse_model(int D, long n_maxsum, const long *n_colmax, int nterms, const int *ids, const int *ids2, const double *params, const int *nparams,
                       const int *nparams1, ModelKernel *m)
{
    if (nterms < 1 || nterms > GPT_MAX_TERMS || !ids || !params || !nparams || (ids2 && !nparams1)) return GPT_E_ARG;
    m->nterms = nterms;
    m->any_prod = m->has_m52 = m->has_chain = m->has_gibbs = m->has_gb = m->has_on_dim = m->has_per = false;      // (the factors beyond nterms stay as they are: never read, zero in a fresh model)
    const double *p = params;
    for (int t = 0; t < nterms; t++) {
        // (plain ids from here on; the coordinate of a GPT_KERNEL_ON_DIM id goes to make_kparams with the id as the ABI gave it)
        const int k1 = GPT_KERNEL_BASE_ID(ids[t]), k2 = (ids2 && ids2[t] >= 0) ? GPT_KERNEL_BASE_ID(ids2[t]) : -1;
        const bool prod = k2 >= 0;
        if (!prod && GPT_KERNEL_DIM_OF(ids[t]) >= 0) {
            gpt_set_error("gpt_fit: term %d: a Gibbs kernel on one coordinate is a product factor (its own term: times SE [1, inf ..])", t);
            return GPT_E_ARG;
        }
        if (!native_fit_kernel(k1) || (prod && !native_fit_kernel(k2))) {
            gpt_set_error("gpt_fit: kernel ids must be SE, Matern52, RationalQuadratic, Matern, Gibbs, Periodic or Spectral");
            return GPT_E_ARG;
        }
        GPT_TRY(check_train_orders(k1, k2, n_maxsum, train_gibbs_max(ids[t], D, n_maxsum, n_colmax),
                                   prod ? train_gibbs_max(ids2[t], D, n_maxsum, n_colmax) : 0));
        if (per_form_kid(k1) || per_form_kid(k2)) {
            if (gibbs_kid(k1) || gibbs_kid(k2)) {
                gpt_set_error("gpt_fit: term %d: %s", t, (k1 == GPT_KERNEL_SPECTRAL || k2 == GPT_KERNEL_SPECTRAL) ? SPECTRAL_GIBBS_MSG : PERIODIC_GIBBS_MSG);
                return GPT_E_ARG;
            }
            GPT_TRY(check_periodic_colmax(n_colmax, n_colmax, D, per_form_name(k1, k2)));      // a pair of training points meets 2 n_colmax[d] in dimension d
        }
        const int n1 = prod ? nparams1[t] : nparams[t];
        if (n1 < 1 || (prod && n1 >= nparams[t])) {
            gpt_set_error("gpt_fit: term %d: %d parameters, %d of them the first factor's", t, nparams[t], n1);
            return GPT_E_ARG;
        }
        GPT_TRY(make_kparams(ids[t], p, n1, D, -1, 1, nullptr, &m->f1[t], prod));
        m->f2[t] = KParams();
        m->f2[t].kernel_id = -1;
        if (prod) GPT_TRY(make_kparams(ids2[t], p + n1, nparams[t] - n1, D, -1, 1, nullptr, &m->f2[t], true));
        m->abi_id1[t] = ids[t];
        m->abi_id2[t] = prod ? ids2[t] : -1;
        m->np[t] = nparams[t];
        m->np1[t] = n1;
        m->any_prod = m->any_prod || prod;
        m->has_m52 = m->has_m52 || k1 == GPT_KERNEL_M52 || k2 == GPT_KERNEL_M52;
        m->has_chain = m->has_chain || is_chain(k1) || is_chain(k2);
        m->has_gibbs = m->has_gibbs || gibbs_kid(k1) || gibbs_kid(k2);
        m->has_gb = m->has_gb || gibbs_gb_kid(k1) || gibbs_gb_kid(k2);
        m->has_on_dim = m->has_on_dim || (D > 1 && (gibbs_kid(k1) || gibbs_kid(k2)));
        m->has_per = m->has_per || per_form_kid(k1) || per_form_kid(k2);
        p += nparams[t];
    }
    m->nparams = (int)(p - params);
    return GPT_OK;
}

// Test points against the model and the resident training points: Matern52 and Gibbs factors limit the test points' own orders,
// a RationalQuadratic / Matern factor or a product the orders of a (test, test) and of a (test, training) pair; `warp`: layers
// are set (gpt_set_warp).
// (n_colmax: the training points' largest order per coordinate, for the periodic kernel's per-dimension rule)
static int check_test_orders(const ModelKernel &m, long n_maxsum, const long *n_colmax, bool warp, const int32_t *nstar, int64_t M, int D)
{
    if (m.has_per) {
        long ms[GPT_MAX_DIM], other[GPT_MAX_DIM];
        order_colmax(nstar, M, D, ms);
        for (int d = 0; d < D; d++) other[d] = ms[d] > n_colmax[d] ? ms[d] : n_colmax[d];      // a (test, test) or a (test, training) pair
        bool periodic = false;
        for (int t = 0; t < m.nterms; t++)
            periodic = periodic || m.f1[t].kernel_id == GPT_KERNEL_PERIODIC || m.f2[t].kernel_id == GPT_KERNEL_PERIODIC;
        GPT_TRY(check_periodic_colmax(ms, other, D, periodic ? "PeriodicKernel" : "SpectralKernel"));
    }
    if (m.has_m52) GPT_TRY(check_m52_orders(nstar, M, D));
    if (m.has_gibbs)
        for (int t = 0; t < m.nterms; t++) {
            if (gibbs_kid(m.f1[t].kernel_id)) GPT_TRY(check_gibbs_orders(nstar, M, D, m.f1[t].g_dim));
            if (m.second(t) && gibbs_kid(m.f2[t].kernel_id)) GPT_TRY(check_gibbs_orders(nstar, M, D, m.f2[t].g_dim));
        }
    if (m.has_chain || m.any_prod) {
        long ms = 0;
        for (int64_t i = 0; i < M; i++) {
            long sn = 0;
            for (int d = 0; d < D; d++) sn += nstar[i * D + d];
            if (sn > ms) ms = sn;
        }
        if (ms + (ms > n_maxsum ? ms : n_maxsum) > GPT_RQ_MAXORD) {
            gpt_set_error("RationalQuadraticKernel: derivative orders of a pair sum to more than %d", GPT_RQ_MAXORD);
            return GPT_E_VALUE;
        }
    }
    if (warp) GPT_TRY(check_warp_orders(nstar, M, D));
    return GPT_OK;
}

// A free-standing pair list (`pairwise`: row i of ni meets row i of nj, M == P) or Gram block (every row meets every column) of
// k1, or of the product k1 * k2 where k2 != NULL: in a product either factor meets the combined order of a pair, and Leibniz
// hands a Gibbs / Matern52 factor at most the points' own orders (a Gibbs factor: those of its own coordinate).
static int check_pair_orders(const KParams &k1, const KParams *k2, const int32_t *ni, int64_t M, const int32_t *nj, int64_t P, int D,
                             bool pairwise)
{
    const int id1 = k1.kernel_id, id2 = k2 ? k2->kernel_id : -1;
    if (id1 == GPT_KERNEL_M52 || id2 == GPT_KERNEL_M52) {
        GPT_TRY(check_m52_orders(ni, M, D));
        GPT_TRY(check_m52_orders(nj, P, D));
    }
    if (is_chain(id1) || k2) GPT_TRY(check_rq_orders(ni, M, nj, P, D, pairwise));
    if (per_form_kid(id1) || per_form_kid(id2)) {
        if (gibbs_kid(id1) || gibbs_kid(id2)) {
            gpt_set_error("%s", (id1 == GPT_KERNEL_SPECTRAL || id2 == GPT_KERNEL_SPECTRAL) ? SPECTRAL_GIBBS_MSG : PERIODIC_GIBBS_MSG);
            return GPT_E_ARG;
        }
        long mi[GPT_MAX_DIM], mj[GPT_MAX_DIM];
        if (pairwise) {                                   // row i of ni meets row i of nj: the combined orders themselves
            for (int d = 0; d < D; d++) mi[d] = mj[d] = 0;
            for (int64_t i = 0; i < M; i++)
                for (int d = 0; d < D; d++)
                    if (ni[i * D + d] + nj[i * D + d] > mi[d]) mi[d] = ni[i * D + d] + nj[i * D + d];
        } else {
            order_colmax(ni, M, D, mi);
            order_colmax(nj, P, D, mj);
        }
        GPT_TRY(check_periodic_colmax(mi, mj, D, per_form_name(id1, id2)));
    }
    for (const KParams *k : {&k1, k2})
        if (k && gibbs_kid(k->kernel_id)) {
            GPT_TRY(check_gibbs_orders(ni, M, D, k->g_dim));
            GPT_TRY(check_gibbs_orders(nj, P, D, k->g_dim));
        }
    return GPT_OK;
}
