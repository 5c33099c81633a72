"""GPU suite (-m gpu): the gradient of the FITC / VFE / DTC objective -- gpt_sparse_grad_diff (api_sparse_grad.inc, ksparse.hip,
kgrad_rect.hip) through SparseGaussianProcess.sparse_gradient, and its kernels alone on raw pointers.

Yardsticks.  SE models: the host's adjoint form with the CPU oracle's exact dK (tests/sparse_grad_cases.py), the bound ten times the
host's own differencing error at the same input set (DIFF_ERR there), relative to the largest kernel-parameter entry.  Every other
family: central differences of the DEVICE value by fd_gradient's rule of tests/test_gpu_grad_diff.py (h = 1e-5 max(1, |theta|), rtol
2e-5, atol 1e-4 max|fd|).  Kernels alone: integer data where the result is exact, bounds from the number format elsewhere.  Each
figure is printed before it is asserted."""
import functools
import math
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_grad_cases as SG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@functools.lru_cache(maxsize=None)
def host_gradient(name, method):
    """(exact kernel-parameter entries, sum g_i) of an SE case by the host's adjoint form: computed once, shared, never modified."""
    from oracle import oracle as O
    O.build()
    exact, _, _, noise, adj = SG.se_gradients(O, name, method)
    return exact, noise[0], adj["alpha"]


def noise(g, d, free=True):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=S.NOISE, noise_bound=(0.0, 5.0), fixed_noise=not free)


def se_gp(g, name, method, chunk):
    c, d = S.CASES[name], S.case_data(name)
    p = c["terms"][0][1]
    k = g.SquaredExponentialKernel(num_dim=c["d"], initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
    return g.SparseGaussianProcess(k, d["Z"], noise_k=noise(g, c["d"]), n_Z=d["nZ"], method=method, jitter=S.JITTER, chunk_rows=chunk, X=d["X"],
                                   y=d["y"], err_y=d["err_y"], n=d["n"])


SE_PARAMS = [(name, m, ch) for name, chunks in SG.SE_CASES.items() for m in SG.METHODS for ch in chunks]


@pytest.mark.parametrize("name,method,chunk", SE_PARAMS)
def test_se_against_the_exact_host_gradient(g, name, method, chunk):
    """The kernel-parameter entries against the host's exact ones within ten times the host's differencing error; the noise entry,
    which no difference enters, 2 sigma_n sum g_i within 1e-7 of it (cond(K_uu + jitter I) u = 1e-8 of the terms alpha_i^2, 1 / Lambda_i
    and |w_i|^2 / Lambda_i^2, which cancel in it to about a tenth of their size); hyperparameters and K_up_to_date as they were."""
    exact, gsum, _ = host_gradient(name, method)
    gp = se_gp(g, name, method, chunk)
    theta = np.array(gp.free_params[:], dtype=float)
    grad = gp.sparse_gradient()
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    nk = len(exact)
    err = np.abs(grad[:nk] - exact).max() / np.abs(exact).max()
    nerr = abs(grad[nk] - 2.0 * S.NOISE * gsum) / abs(2.0 * S.NOISE * gsum)
    print("%s %s chunk %s: device - exact = %.3g of max|grad_k| = %.5g (bound %.3g); noise entry off by %.3g" % (
        name, method, chunk, err, np.abs(exact).max(), SG.bound(name), nerr))
    assert err <= SG.bound(name), (err, SG.bound(name))
    assert nerr <= 1e-7, nerr


def fd_gradient(gp, theta):
    """Central differences of the device log-posterior: tests/test_gpu_grad_diff.py's rule."""
    fd = np.zeros_like(theta)
    for i in range(len(theta)):
        h = 1e-5 * max(1.0, abs(theta[i]))
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (-gp.update_hyperparameters(tp) + gp.update_hyperparameters(tm)) / (2 * h)
    return fd


def check_against_fd(make, label):
    gp = make()
    theta = np.array(gp.free_params[:], dtype=float)
    assert np.isfinite(gp.update_hyperparameters(theta)) and gp._fit_mode == "sparse"
    grad = gp.sparse_gradient()
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    fd = fd_gradient(make(), theta)
    err = np.abs(grad - fd)
    print("%s: p = %d, max|fd| = %.4g, max|grad - fd| / max|fd| = %.3g" % (label, len(theta), np.abs(fd).max(), err.max() / np.abs(fd).max()))
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max(), err_msg=label)
    return gp, grad


def kernel_of(g, terms, d):
    cls = {"se": g.SquaredExponentialKernel, "m52": g.Matern52Kernel, "rq": g.RationalQuadraticKernel}

    def one(name, p):
        return cls[name](num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
    out = None
    for t in terms:
        k = one(t[0], t[1]) * one(t[2], t[3]) if len(t) == 4 else one(t[0], t[1])
        out = k if out is None else out + k
    return out


def case_gp(g, name, method):
    """A case of tests/sparse_cases.py as tests/test_gpu_sparse.py builds it, with the case's first chunk_rows."""
    c, d = S.CASES[name], S.case_data(name)
    return g.SparseGaussianProcess(kernel_of(g, c["terms"], c["d"]), d["Z"], noise_k=noise(g, c["d"]), n_Z=d["nZ"], method=method,
                                   jitter=S.JITTER, chunk_rows=c["chunks"][0], X=d["X"], y=d["y"], err_y=d["err_y"], n=d["n"])


@pytest.mark.parametrize("name,method", [("sum_prod_1100", "fitc"), ("rq_257", "vfe"), ("m52_m300", "fitc"), ("m52_m300", "vfe"),
                                         ("sum_m257", "fitc"), ("sum_m257", "vfe")])
def test_case_families_against_central_differences(g, name, method):
    """Sum and product terms (sum_prod_1100, sum_m257), derivative rows on Z (rq_257, m52_m300), M = 300 past the 256-thread stride."""
    check_against_fd(lambda: case_gp(g, name, method), "%s %s" % (name, method))


def data_1d(N=300, M=24, nder=30):
    X, n, y = S.inputs(N, 1, nder=nder)
    Z = np.random.RandomState(97).rand(M, 1)
    return X, n, y, Z


@pytest.mark.parametrize("method", ["fitc", "vfe"])
def test_gibbs_exp_gauss_eleven_parameters_cross_the_launch_group(g, method):
    """11 free parameters of one term: two launches (8 + 3) of either pair pass."""
    X, n, y, Z = data_1d()
    p = [1.1, 0.35, 0.2, 0.5, 0.8, 0.15, 0.2, 0.1, 0.4, -0.5, 0.3]
    gp, grad = check_against_fd(lambda: g.SparseGaussianProcess(
        g.GibbsKernel1dExpGauss(3, initial_params=p, param_bounds=[(-10.0, 10.0)] * 11), Z, noise_k=noise(g, 1, free=False), method=method,
        X=X, y=y, err_y=0.05, n=n), "gibbs exp-gauss " + method)
    assert len(grad) == 11 and np.all(grad != 0.0)


def test_periodic_term(g):
    X, n, y, Z = data_1d(nder=0)
    check_against_fd(lambda: g.SparseGaussianProcess(
        g.PeriodicKernel(num_dim=1, initial_params=[1.0, 0.9, 0.8], param_bounds=[(1e-2, 10.0)] * 3), Z, noise_k=noise(g, 1), method="fitc",
        X=X, y=y, err_y=0.05, n=n), "periodic")


def test_fixed_noise_and_a_zero_kernel(g):
    d = S.case_data("se_300")
    for nk in (noise(g, 2, free=False), g.ZeroKernel(num_dim=2)):
        gp, grad = check_against_fd(lambda: g.SparseGaussianProcess(
            g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.6], param_bounds=[(0.0, 1e3)] * 3), d["Z"], noise_k=nk, method="vfe",
            X=d["X"], y=d["y"], err_y=0.05, n=d["n"]), "fixed noise / zero kernel")
        assert len(grad) == 3


def test_mean_function_with_free_parameters(g):
    """alpha_out: the entries of a linear mean function's parameters are d mu . alpha."""
    d = S.case_data("se_300")
    n0 = np.zeros_like(d["n"])
    for method in ("fitc", "vfe"):
        gp, grad = check_against_fd(lambda: g.SparseGaussianProcess(
            g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3), d["Z"], noise_k=noise(g, 2),
            mu=g.LinearMeanFunction(num_dim=2, initial_params=[0.2, -0.1, 0.05]), method=method, chunk_rows=128, X=d["X"], y=d["y"],
            err_y=d["err_y"], n=n0), "linear mean " + method)
        assert len(grad) == 7


# ---- determinism and isolation ---------------------------------------------------------------------------------------------------
def stencil_of(theta, rel=6e-6):
    pa, pb, dn = [], [], []
    for h in range(len(theta)):
        ta, tb, den = SG.stencil(theta, h, rel)
        pa.append(ta)
        pb.append(tb)
        dn.append(den)
    return [0] * len(theta), pa, pb, dn


@pytest.mark.parametrize("method", SG.METHODS)
def test_two_calls_give_equal_bits_and_leave_everything_else_alone(g, method):
    """gpt_fit, gpt_sparse_fit and two gpt_sparse_grad_diff on ONE context: equal bits from the two calls, alpha against the host's, and
    no bit of c, of a following sparse prediction or of the dense factor's predictions changes."""
    from gptools_amd import _lib
    d = S.case_data("se_300")
    nk = noise(g, 2)
    ctx = _lib.Context()
    ctx.set_data(d["X"], d["n"])
    ctx.fit(_lib.KERNEL_SE, S.SE2, S.NOISE ** 2, d["y"], d["err_y"], 1e2 * np.finfo(float).eps)
    dense_before = ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    ctx.sparse_fit(_lib.SPARSE_METHODS[method], [(_lib.KERNEL_SE, S.SE2)], S.NOISE ** 2, d["y"], d["err_y"], S.JITTER, 128)
    c0 = ctx.sparse_get_c()
    sp_before = ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    tix, pa, pb, dn = stencil_of(S.SE2)
    out1, alpha1 = ctx.sparse_grad_diff(tix, pa, pb, dn, d["y"], d["err_y"], want_alpha=True)
    out2, alpha2 = ctx.sparse_grad_diff(tix, pa, pb, dn, d["y"], d["err_y"], want_alpha=True)
    assert np.array_equal(out1, out2) and np.array_equal(alpha1, alpha2) and np.all(np.isfinite(out1))
    exact, gsum, alpha = host_gradient("se_300", method)
    aerr = np.abs(alpha1 - alpha).max() / np.abs(alpha).max()
    print("%s: alpha device - host = %.3g of max|alpha|; gradient %s" % (method, aerr, out1))
    assert aerr <= 1e-7                                  # cond(K_uu + jitter I) u = 3e-9 of it, a margin of thirty
    assert np.abs(out1[:3] - exact).max() <= SG.bound("se_300") * np.abs(exact).max()
    # no entry without the noise trace, and nh = 0 gives the trace alone, the same bits
    out0, none = ctx.sparse_grad_diff([], [], [], [], d["y"], d["err_y"])
    assert none is None and out0.shape == (1,) and out0[0] == out1[3]
    assert np.array_equal(ctx.sparse_get_c(), c0)
    for a, b in zip(sp_before, ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(a, b)
    for a, b in zip(dense_before, ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_calls_out_of_order_and_refusals_of_the_library(g):
    from gptools_amd import _lib
    d = S.case_data("se_300")
    terms = [(_lib.KERNEL_SE, S.SE2)]
    tix, pa, pb, dn = stencil_of(S.SE2)

    def call(ctx, denom=dn):
        return ctx.sparse_grad_diff(tix, pa, pb, denom, d["y"], d["err_y"])
    ctx = _lib.Context()
    ctx.set_data(d["X"], d["n"])
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    ctx._sparse_nparams = [3]                                     # (the wrapper's own check aside: the library must answer)
    with pytest.raises(_lib.GPTBackendError):                     # GPT_E_STATE: no sparse fit
        call(ctx)
    ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    assert np.all(np.isfinite(call(ctx)[0]))
    with pytest.raises(ValueError):                               # GPT_E_ARG
        call(ctx, [dn[0], 0.0, dn[2]])
    ctx.set_T(np.eye(300))
    with pytest.raises(NotImplementedError):
        call(ctx)
    ctx.set_T(None)
    ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.set_warp([(_lib.WARP_LINEAR, [-0.5, -0.25, 1.5, 2.0])])
    with pytest.raises(NotImplementedError):
        call(ctx)
    ctx.set_warp(None)
    ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])                      # new inducing points drop the fit
    with pytest.raises(_lib.GPTBackendError):
        call(ctx)
    ctx.sparse_fit(0, terms, 0.01, d["y"], d["err_y"], S.JITTER)
    ctx.set_data(d["X"], d["n"])                                  # new data drop the inducing points and the fit
    with pytest.raises(_lib.GPTBackendError):
        call(ctx)


# ---- the kernels alone, on raw pointers --------------------------------------------------------------------------------------------
M_LIST = [1, 2, 255, 256, 257, 511, 512, 513, 1025]
#: W_ii and g_i take up to 7 correctly rounded operations (multiply, divide, fused multiply-add) in another order than numpy's: 8 units
#: of 2^-52 allowed; measured: 0 in all 27 cases (with these power-of-two Lambda_i every intermediate happens to be exact)
ULP8 = 8.0 * 2.0 ** -52


def _up(x, m):
    return (x + m - 1) // m * m


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("M", M_LIST)
def test_row_kernel_alone(M, method):
    """gpt_dev_sparse_grad_rows on six rows of integers: the three row sums are integers (exact in any order), so with Lambda_i = 4 or
    8 (powers of two) alpha_i, e_i (vfe, dtc), and both scaled copies are exact; W_ii and g_i within 8 ulp.  Then bad rows among good
    ones: flag word, zeros, the good rows' bits unchanged."""
    import torch
    from gptools_amd import _lib
    lib = _lib.load()
    rows, ld, ldr = 6, _up(M + 1, 128), 8
    rs = np.random.RandomState(2000 * method + M)
    V = np.zeros((rows, ld))
    W = np.zeros((rows, ld))
    V[:, :M] = rs.randint(-3, 4, size=(rows, M))
    W[:, :M] = rs.randint(-2, 3, size=(rows, M))
    V[:, M:] = 555.0                                       # (never read: the copies get zeros there)
    t = rs.randint(-2, 3, size=M).astype(float)
    q = (V[:, :M] ** 2).sum(1)
    kpart = np.array([1.0, 5.0, 1.0, 5.0, 1.0, 5.0])       # k_i - q_i: Lambda = 4 or 8 for fitc with s = 3
    r = rs.randint(-5, 6, size=rows).astype(float)
    ctx = _lib.Context()

    def run(kdiag, err, noise_var):
        dV, dW = torch.tensor(V, device="cuda"), torch.tensor(W, device="cuda")
        dk, dr, de, dt = (torch.tensor(np.asarray(a, dtype=float), device="cuda") for a in (kdiag, r, err, t))
        da, do = (torch.full((rows,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        dg = torch.full((2 * ldr,), -7.0, dtype=torch.float64, device="cuda")
        d1, d2 = (torch.full((rows, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        dbad = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.gpt_dev_sparse_grad_rows(ctx.handle, dV.data_ptr(), dW.data_ptr(), ld, rows, M, method, dk.data_ptr(), dr.data_ptr(),
                                                de.data_ptr(), noise_var, dt.data_ptr(), da.data_ptr(), do.data_ptr(), dg.data_ptr(), ldr,
                                                d1.data_ptr(), d2.data_ptr(), dbad.data_ptr()))
        ctx.synchronize()
        return [x.cpu().numpy() for x in (da, do, dg, d1, d2)] + [int(dbad.cpu()[0])]

    s = 3.0 if method == 0 else 4.0                        # noise_var 2 (fitc) / 3 with err 1
    lam = kpart + s if method == 0 else np.full(rows, s)
    ga, ge, gg, g1, g2, gbad = run(q + kpart, np.ones(rows), s - 1.0)
    assert gbad == 0
    alpha = (r - V[:, :M].dot(t)) / lam
    wii = alpha ** 2 - 1.0 / lam + (W[:, :M] ** 2).sum(1) / lam ** 2
    e = wii if method == 0 else (np.full(rows, -1.0 / s) if method == 1 else np.zeros(rows))
    gref = 0.5 * wii + (0.5 * kpart / s ** 2 if method == 1 else 0.0)
    assert np.array_equal(ga, alpha)
    if method:
        assert np.array_equal(ge, e)
    off = max((np.abs(ge - e) / np.maximum(np.abs(e), 1e-300)).max() if method == 0 else 0.0, (np.abs(gg[:rows] - gref) / np.maximum(np.abs(gref), 1e-300)).max())
    print("M %d method %d: e / g off by %.3g units of 2^-52" % (M, method, off * 2.0 ** 52))
    assert np.all(np.abs(ge - e) <= ULP8 * np.abs(e)) and np.all(np.abs(gg[:rows] - gref) <= ULP8 * np.abs(gref))
    assert np.array_equal(gg[ldr:ldr + rows], np.zeros(rows)) and np.array_equal(gg[rows:ldr], np.full(ldr - rows, -7.0))
    assert np.array_equal(g1[:, :M], V[:, :M] / lam[:, None]) and np.array_equal(g1[:, M:], np.zeros((rows, ld - M)))
    assert np.array_equal(g2[:, :M], V[:, :M] * ge[:, None]) and np.array_equal(g2[:, M:], np.zeros((rows, ld - M)))
    # ---- rows 1 and 4 bad
    kd = q + kpart
    if method == 0:
        kd[1], kd[4] = q[1] - 10.0, np.nan
        ba, be, bg, b1, b2, bbad = run(kd, np.ones(rows), s - 1.0)
    else:
        err = np.full(rows, 2.0)
        err[1], err[4] = 0.0, np.inf
        ba, be, bg, b1, b2, bbad = run(kd, err, 0.0)
    good = np.array([0, 2, 3, 5])
    assert bbad == 1
    for i in (1, 4):
        assert ba[i] == 0.0 and be[i] == 0.0 and bg[i] == 0.0 and not b1[i].any() and not b2[i].any()
    for a, b in ((ba, ga), (be, ge), (bg[:rows], gg[:rows]), (b1, g1), (b2, g2)):
        assert np.array_equal(a[good], b[good])


@pytest.mark.parametrize("rows,mg,nslices,wide", [(5, 64, 2, False), (130, 128, 0, True), (9, 1088, 1, False)])
def test_two_operand_gram_alone(rows, mg, nslices, wide):
    """gpt_dev_sparse_gram2 on integer data with weights of both signs: G += (e v)^T v exactly, one tile and 153 tiles, ldg > mg."""
    import torch
    from gptools_amd import _lib
    rs = np.random.RandomState(rows + mg)
    ldv = mg + 64
    V = rs.randint(-4, 5, size=(rows, ldv)).astype(float)
    e = rs.randint(-3, 4, size=rows).astype(float)
    A = V * e[:, None]
    ldg = mg + 64 if wide else mg
    Gw = rs.randint(-3, 4, size=(mg, ldg)).astype(float)
    ctx = _lib.Context()
    dA, dV, dG = (torch.tensor(x, device="cuda") for x in (A, V, Gw))
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_gram2(ctx.handle, dA.data_ptr(), dV.data_ptr(), ldv, rows, mg, nslices, dG.data_ptr(), ldg))
    ctx.synchronize()
    got = dG.cpu().numpy()
    assert np.array_equal(got[:, mg:], Gw[:, mg:])
    want = Gw[:, :mg] + A[:, :mg].T.dot(V[:, :mg])
    low = np.tril(np.ones((mg // 64, mg // 64))).repeat(64, 0).repeat(64, 1) > 0
    assert np.array_equal(got[:, :mg][low], want[low]) and np.array_equal(got[:, :mg][~low], Gw[:, :mg][~low])


@pytest.mark.parametrize("rows,mg,nslices", [(5, 64, 2), (130, 128, 7), (70, 192, 3)])
def test_two_operand_gram_with_equal_operands_is_the_one_operand_gram(rows, mg, nslices):
    """gpt_dev_sparse_gram2(A = V) and gpt_dev_sparse_gram(V) onto copies of one G, on data that is not integer: the same bits in all of
    G.  The two share their tiles, slices, lane maps and the layout of the partial tiles, so every sum is taken in the same order."""
    import torch
    from gptools_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(1000 * rows + mg)
    ldv = mg + 64
    V, G = rs.standard_normal((rows, ldv)), rs.standard_normal((mg, mg))
    ctx = _lib.Context()
    dV, dG1, dG2 = torch.tensor(V, device="cuda"), torch.tensor(G, device="cuda"), torch.tensor(G, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.gpt_dev_sparse_gram(ctx.handle, dV.data_ptr(), ldv, rows, mg, nslices, dG1.data_ptr(), mg))
    _lib.check(lib.gpt_dev_sparse_gram2(ctx.handle, dV.data_ptr(), dV.data_ptr(), ldv, rows, mg, nslices, dG2.data_ptr(), mg))
    ctx.synchronize()
    g1, g2 = dG1.cpu().numpy(), dG2.cpu().numpy()
    assert not np.array_equal(g1, G)
    assert np.array_equal(g1, g2)


U = 2.0 ** -53


@pytest.mark.parametrize("rows,M", [(1, 1), (63, 65), (64, 64), (65, 63), (300, 257), (300, 1), (1, 257)])
@pytest.mark.parametrize("kind", ["se", "m52*se"])
def test_rectangular_pair_pass_alone(rows, M, kind):
    """gpt_dev_sparse_grad_pairs against sum A (K_b - K_a) + 1/2 sum e (k_b - k_a)(x_i, x_i) in numpy with math.fsum, K_a and K_b from
    the library's builder (gpt_kbuild / gpt_kbuild2) at the two stencil points; lda > M.
    Bound, from the number format: the device adds L = rows M + rows products in some order, |error| <= L u sum |A_ij| |dk_ij| to first
    order; each dk_ij = k_b - k_a is exact given k_a and k_b (they agree to 1e-5), and a k may differ from the builder's by a few ulp
    where the builder takes another code path for the same pair function (its plain tiles): 8 u (|k_a| + |k_b|) per pair.  Together
    (L + 8) u sum |A_ij| (|k_a| + |k_b|)_ij, with the weights e_i / 2 on the diagonal part.  Not fitted to the device's figures."""
    import torch
    from gptools_amd import _lib
    lib = _lib.load()
    d = 2
    rs = np.random.RandomState(rows * 1000 + M)
    X, Z = rs.rand(rows, d), rs.rand(M, d)
    nx, nz = np.zeros((rows, d), dtype=np.int32), np.zeros((M, d), dtype=np.int32)
    nx[-(rows // 5):, 0] = 1 if rows >= 5 else 0
    nz[-(M // 8):, 1] = 1 if M >= 8 else 0
    lda = _up(M + 1, 128) + 2
    A = np.zeros((rows, lda))
    A[:, :M] = rs.randn(rows, M)
    A[:, M:] = 1e30                                         # (never read)
    e = rs.randn(rows)
    p1, p2 = [1.1, 0.4, 0.6], [0.9, 0.7, 0.9]
    theta = p1 + (p2 if kind != "se" else [])
    nh = len(theta)
    pa, pb = [], []
    for h in range(nh):
        ta, tb, _ = SG.stencil(theta, h)
        pa.append(ta)
        pb.append(tb)
    ctx = _lib.Context()

    def K(p, Xi, ni, Xj, nj):
        if kind == "se":
            return ctx.kbuild(_lib.KERNEL_SE, p, Xi, ni, Xj, nj)
        return ctx.kbuild2(_lib.KERNEL_M52, p[:3], _lib.KERNEL_SE, p[3:], Xi, ni, Xj, nj)

    def Kd(p):
        return np.array([K(p, X[i:i + 1], nx[i:i + 1], X[i:i + 1], nx[i:i + 1])[0, 0] for i in range(rows)])
    dX, dZ, dA, de = (torch.tensor(a, device="cuda") for a in (X, Z, A, e))
    dnx, dnz = torch.tensor(nx, device="cuda"), torch.tensor(nz, device="cuda")
    torch.cuda.synchronize()
    out = np.zeros(nh)
    ids = (_lib.KERNEL_SE, -1) if kind == "se" else (_lib.KERNEL_M52, _lib.KERNEL_SE)
    fa, fb = np.ascontiguousarray(pa, dtype=float), np.ascontiguousarray(pb, dtype=float)
    _lib.check(lib.gpt_dev_sparse_grad_pairs(ctx.handle, ids[0], ids[1], d, 1, nh, _lib.dptr(fa), _lib.dptr(fb), nh, 3, dX.data_ptr(),
                                             dnx.data_ptr(), rows, dZ.data_ptr(), dnz.data_ptr(), M, dA.data_ptr(), lda, de.data_ptr(),
                                             _lib.dptr(out)))
    ctx.synchronize()
    L = rows * M + rows
    for h in range(nh):
        Ka, Kb = K(pa[h], X, nx, Z, nz), K(pb[h], X, nx, Z, nz)
        ka, kb = Kd(pa[h]), Kd(pb[h])
        ref = math.fsum((A[:, :M] * (Kb - Ka)).ravel()) + math.fsum(0.5 * e * (kb - ka))
        size = math.fsum((np.abs(A[:, :M]) * (np.abs(Ka) + np.abs(Kb))).ravel()) + math.fsum(0.5 * np.abs(e) * (np.abs(ka) + np.abs(kb)))
        bound = (L + 8) * U * size
        print("%s rows %d M %d h %d: device - fsum = %.3g (bound %.3g, sum %.6g)" % (kind, rows, M, h, abs(out[h] - ref), bound, ref))
        assert abs(out[h] - ref) <= bound, (h, out[h], ref, bound)


# ---- the optimiser ----------------------------------------------------------------------------------------------------------------
def test_optimiser_with_the_sparse_gradient_reaches_the_value_routes_optimum(g):
    """The shape of tests/test_gpu_grad_diff.py's optimiser test at N = 300, M = 40: Matern-5/2, SLSQP from the same start, ftol 1e-6:
    the optimum of gradient="sparse" is not above the value route's by more than ftol, and the two are within ftol of each other.
    The number of evaluations of each route is printed.

    The value route differences the objective with scipy's central scheme (jac="3-point", relative step 6e-6).  Forward differences at
    eps = 1e-6, the dense test's choice, carry a truncation eps f'' / 2, and along the noise parameter f'' is 1e5 ... 1e6 here (the
    gradient is 3e4 at 0.05 from the optimum): an error of 0.05 ... 0.5 in that entry, at which SLSQP stops a g^2 / (2 f'') = 1e-5
    short of the optimum.  Measured with forward differences: value route -394.430841571 (113 evaluations, final gradient entry
    -1.14), gradient="sparse" -394.430867689 (28 evaluations, 21 gradients), 2.6e-5 apart, the sparse route the lower."""
    d = S.case_data("se_300")
    ftol = 1e-6
    res = {}
    for gradient in (None, "sparse"):
        gp = g.SparseGaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 0.5, 0.5], param_bounds=[(1e-2, 10.0)] * 3), d["Z"],
                                     noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 5.0)), method="vfe",
                                     X=d["X"], y=d["y"], err_y=0.02, n=np.zeros_like(d["n"]))
        kw = {"options": {"ftol": ftol}}
        if gradient is None:
            kw["jac"] = "3-point"
        best, _ = gp.optimize_hyperparameters(random_starts=0, opt_kwargs=kw, gradient=gradient)
        assert best.success, best
        res[gradient] = best
    print("value route %.12g (%d evaluations), sparse gradient %.12g (%d evaluations, %d gradients)"
          % (res[None].fun, res[None].nfev, res["sparse"].fun, res["sparse"].nfev, res["sparse"].njev))
    assert res["sparse"].fun <= res[None].fun + ftol
    assert abs(res[None].fun - res["sparse"].fun) <= ftol
