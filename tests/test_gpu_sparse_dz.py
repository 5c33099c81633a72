"""GPU suite (-m gpu): the gradient of the FITC / VFE / DTC objective with respect to the inducing inputs -- gpt_sparse_grad_z
(api_sparse_grad.inc, kgrad_dz.hip) through SparseGaussianProcess.inducing_gradient / optimize_inducing, and its pair pass alone on
raw pointers (gpt_dev_sparse_grad_dz_pairs).

Yardsticks.  (1) The kernel alone: numpy's sum_i A[i,m] K'_d[i,m] in extended precision with K'_d from the library's own builder at
the orders n_Z + e_d, the bound from the number format.  (2) Whole gradients: the host's exact dZ (tests/sparse_dz_cases.py), every
entry, within ten times the host's own discrepancy at the same input set.  (3) Families the host form has no exact blocks for: central
differences of the DEVICE value in Z, h = 1e-5 max(1, |z|), rtol 2e-5, atol 1e-4 max|fd| (tests/test_gpu_sparse_grad.py's rule).
Each figure is printed before it is asserted."""
import functools
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_grad_cases as SG
import sparse_dz_cases as SZ

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.fixture(scope="module")
def ctx():
    from gptools_amd import _lib
    return _lib.Context()


# ---- (1) the kernel alone against the builder -------------------------------------------------------------------------------------------
ROWS = [1, 3, 63, 64, 65, 257]
MS = [1, 63, 64, 65, 129]
#: family -> the num_dim it is run at
FAMILIES = {"se": (1, 2, 3), "m52": (1, 2, 3), "rq": (1, 2, 3), "se*periodic": (1, 2, 3), "se+m52": (1, 2, 3), "gibbs_tanh": (1,)}
#: c of the bound (rows + c) u sum_i |A[i,m] K'_d[i,m]|: what a pair value of kgrad_dz_kernel may differ from the builder's by, in units
#: of u |K'|, because the two instantiations of one pair function contract and schedule on their own.  Measured on the MI355X by
#: test_pair_values_against_the_builder (rows = 1, A = 1: the output IS the pair value), the worst per family over M, num_dim and the
#: orders of the cases below: 0 for every family -- the pair values are the builder's bit for bit (the library is compiled without
#: contraction, and both kernels call the same pair function).  A margin of 4 on a measurement of 0 would demand equal bits of every
#: later compiler; the constant is the margin applied to ONE unit, the smallest figure the measurement could have shown
C_PAIR = {"se": 4.0, "m52": 4.0, "rq": 4.0, "se*periodic": 4.0, "se+m52": 4.0, "gibbs_tanh": 4.0}


def _up(x, m):
    return (x + m - 1) // m * m


def family_terms(family, D):
    """The calls of a family: [(kernel_id, kernel_id2, parameters, parameters of the first factor)] -- two for the sum."""
    from gptools_amd import _lib
    ls = [0.4, 0.6, 0.9][:D]
    se = [1.1] + ls
    m52 = [0.7] + [1.3 * v for v in ls]
    if family == "se":
        return [(_lib.KERNEL_SE, -1, se, len(se))]
    if family == "m52":
        return [(_lib.KERNEL_M52, -1, m52, len(m52))]
    if family == "rq":
        return [(_lib.KERNEL_RQ, -1, [1.0, 1.7] + ls, D + 2)]
    if family == "se*periodic":
        return [(_lib.KERNEL_SE, _lib.KERNEL_PERIODIC, se + [0.9] + [1.5 * v for v in ls] + [0.8, 1.1, 0.7][:D], len(se))]
    if family == "se+m52":
        return [(_lib.KERNEL_SE, -1, se, len(se)), (_lib.KERNEL_M52, -1, m52, len(m52))]
    assert family == "gibbs_tanh" and D == 1
    return [(_lib.KERNEL_GIBBS_TANH, -1, [1.1, 0.3, 0.6, 0.2, 0.5], 5)]


def pair_inputs(family, D, rows, M, square):
    """Seeded points with derivative orders: some rows of X of order 1 in coordinate 0; for rq orders among Z as well (the last
    coordinate); square: X := Z (the Z-Z pass)."""
    rs = np.random.RandomState(10000 * D + 100 * rows + M)
    Z = rs.rand(M, D)
    nz = np.zeros((M, D), dtype=np.int32)
    if family == "rq" and M >= 8:
        nz[-(M // 8):, D - 1] = 1
    if square:
        return Z, nz, Z, nz
    X = rs.rand(rows, D)
    nx = np.zeros((rows, D), dtype=np.int32)
    if rows >= 5:
        nx[-(rows // 5):, 0] = 1
    return X, nx, Z, nz


def builder(ctx, term, X, nx, Z, nz):
    kid, kid2, p, n1 = term
    if kid2 < 0:
        return ctx.kbuild(kid, p, X, nx, Z, nz)
    return ctx.kbuild2(kid, p[:n1], kid2, p[n1:], X, nx, Z, nz)


def dz_pairs(ctx, term, D, X, nx, Z, nz, A, lda, skip_diag):
    """gpt_dev_sparse_grad_dz_pairs on fresh device copies -> (M, D)."""
    import torch
    from gptools_amd import _lib
    kid, kid2, p, n1 = term
    rows, M = len(X), len(Z)
    dX, dZ, dA = (torch.tensor(np.ascontiguousarray(a, dtype=float), device="cuda") for a in (X, Z, A))
    dnx, dnz = torch.tensor(np.ascontiguousarray(nx), device="cuda"), torch.tensor(np.ascontiguousarray(nz), device="cuda")
    torch.cuda.synchronize()
    out = np.full((M, D), np.nan)
    fp = np.ascontiguousarray(p, dtype=float)
    _lib.check(_lib.load().gpt_dev_sparse_grad_dz_pairs(ctx.handle, kid, kid2, D, int(max(nx.sum(1).max(), nz.sum(1).max() + 1)), _lib.dptr(fp),
                                                        len(fp), n1, dX.data_ptr(), dnx.data_ptr(), rows, dZ.data_ptr(), dnz.data_ptr(), M,
                                                        dA.data_ptr(), lda, int(skip_diag), _lib.dptr(out)))
    ctx.synchronize()
    return out


def raised_blocks(ctx, term, D, X, nx, Z, nz):
    """K'_d (rows x M) per dimension from the device builder at the orders n_Z + e_d."""
    out = []
    for dim in range(D):
        up = nz.copy()
        up[:, dim] += 1
        out.append(builder(ctx, term, X, nx, Z, up))
    return out


FAMILY_D = [(f, D) for f, dims in FAMILIES.items() for D in dims]


@pytest.mark.parametrize("family,D", FAMILY_D)
def test_pair_values_against_the_builder(ctx, family, D):
    """rows = 1 and A = 1: the output is the pair value itself.  The figure c of C_PAIR, printed per case of M; held to the constant."""
    worst = 0.0
    for M in MS:
        X, nx, Z, nz = pair_inputs(family, D, 1, M, False)
        lda = _up(M + 1, 128) + 2
        A = np.ones((1, lda))
        for term in family_terms(family, D):
            got = dz_pairs(ctx, term, D, X, nx, Z, nz, A, lda, 0)
            ref = np.stack([k[0] for k in raised_blocks(ctx, term, D, X, nx, Z, nz)], axis=1)
            assert np.all(np.isfinite(got)) and np.abs(ref).max() > 0.0
            c = (np.abs(got - ref) / (U * np.maximum(np.abs(ref), 1e-300))).max()
            worst = max(worst, c)
    print("%s D %d: pair values differ from the builder's by c = %.3g units of u |K'| (C_PAIR %.3g)" % (family, D, worst, C_PAIR[family]))
    assert C_PAIR[family] <= 100.0
    assert worst <= C_PAIR[family], (family, D, worst)


def check_pass(ctx, family, D, rows, M, square, skip_diag):
    X, nx, Z, nz = pair_inputs(family, D, rows, M, square)
    rows = len(X)
    rs = np.random.RandomState(rows + 7 * M)
    lda = _up(M + 1, 128) + 2
    A = np.full((rows, lda), 1e30)                           # (the columns [M, lda) are never read)
    A[:, :M] = rs.randn(rows, M)
    worst = 0.0
    for term in family_terms(family, D):                     # (a sum is two calls: each call is held to the bound on its own)
        got = dz_pairs(ctx, term, D, X, nx, Z, nz, A, lda, skip_diag)
        ref, size = np.zeros((M, D), dtype=LD), np.zeros((M, D), dtype=LD)
        for dim, K in enumerate(raised_blocks(ctx, term, D, X, nx, Z, nz)):
            P = A[:, :M].astype(LD) * K.astype(LD)
            if skip_diag:
                P = P * (1 - np.eye(rows, M, dtype=LD))
            ref[:, dim] = P.sum(0)
            size[:, dim] = np.abs(P).sum(0)
        # the device's recursive sum of `rows` products, and c for the pair values
        bound = (rows + C_PAIR[family]) * U * size
        err = np.abs(got.astype(LD) - ref)
        worst = max(worst, float((err / np.maximum(bound, LD(1e-300))).max()))
        assert np.all(np.isfinite(got)), (family, D, rows, M)
        assert np.all(err <= bound), (family, D, rows, M, square, skip_diag, worst)
    return worst


@pytest.mark.parametrize("family,D", FAMILY_D)
def test_pair_pass_alone(ctx, family, D):
    """gpt_dev_sparse_grad_dz_pairs over rows x M: waves without rows, the row-tile and the column-tile edges, lda > M, signed random A.
    Tolerance per entry (rows + c) u sum_i |A[i,m] K'_d[i,m]|: the standard bound of a recursive sum of `rows` terms plus c = C_PAIR;
    the two calls of the sum se + m52 are each held to it on their own."""
    worst = 0.0
    for rows in ROWS:
        for M in MS:
            worst = max(worst, check_pass(ctx, family, D, rows, M, False, 0))
    print("%s D %d: %d shapes, worst |device - numpy| = %.3g of the bound" % (family, D, len(ROWS) * len(MS), worst))


@pytest.mark.parametrize("family,D", [("se", 2), ("rq", 1), ("se*periodic", 3), ("m52", 2), ("gibbs_tanh", 1)])
def test_pair_pass_with_and_without_the_diagonal(ctx, family, D):
    """X := Z: skip_diag drops exactly the pairs i == m, and without it they are in the sum."""
    for M in MS:
        on, off = check_pass(ctx, family, D, M, M, True, 1), check_pass(ctx, family, D, M, M, True, 0)
        print("%s D %d M %d: skip_diag on %.3g / off %.3g of the bound" % (family, D, M, on, off))
    # ... and the flag is about the INDICES: with X another set of points than Z and A the identity, the pairs i == m are all there is
    X, nx, Z, nz = pair_inputs("rq", 1, 65, 65, False)
    term = family_terms("rq", 1)[0]
    A = np.zeros((65, 128))
    A[:, :65] = np.eye(65)
    a, b = dz_pairs(ctx, term, 1, X, nx, Z, nz, A, 128, 1), dz_pairs(ctx, term, 1, X, nx, Z, nz, A, 128, 0)
    kd = np.diag(raised_blocks(ctx, term, 1, X, nx, Z, nz)[0])
    assert not a.any() and np.all(kd != 0.0) and np.all(np.abs(b[:, 0] - kd) <= C_PAIR["rq"] * U * np.abs(kd))


# ---- (2) inducing_gradient against the host's exact dZ -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_dz(name, method):
    """The host's exact dZ of a case: computed once, shared, never modified."""
    from oracle import oracle as O
    O.build()
    _, _, adj, up = SZ.setup(O, name, method)
    dz = SZ.exact_dz(adj, up)
    dz.setflags(write=False)
    return dz


def noise(g, d, free=True):
    return g.DiagonalNoiseKernel(num_dim=d, initial_noise=S.NOISE, noise_bound=(0.0, 5.0), fixed_noise=not free)


def kernel_of(g, terms, d):
    cls = {"se": g.SquaredExponentialKernel, "m52": g.Matern52Kernel, "rq": g.RationalQuadraticKernel}

    def one(name, p):
        return cls[name](num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
    out = None
    for t in terms:
        k = one(t[0], t[1]) * one(t[2], t[3]) if len(t) == 4 else one(t[0], t[1])
        out = k if out is None else out + k
    return out


def case_gp(g, name, method, chunk):
    c, d = S.CASES[name], S.case_data(name)
    return g.SparseGaussianProcess(kernel_of(g, c["terms"], c["d"]), d["Z"], noise_k=noise(g, c["d"]), n_Z=d["nZ"], method=method,
                                   jitter=S.JITTER, chunk_rows=chunk, X=d["X"], y=d["y"], err_y=d["err_y"], n=d["n"])


def dz_error(got, name, method):
    ref = host_dz(name, method)
    assert got.shape == ref.shape
    return np.abs(got - ref).max() / np.abs(ref).max()


CASE_PARAMS = [(name, m, ch) for name, chunks in SZ.CASES.items() for m in S.CASES[name]["methods"] for ch in chunks]


@pytest.mark.parametrize("name,method,chunk", CASE_PARAMS)
def test_inducing_gradient_against_the_exact_host_gradient(g, name, method, chunk):
    """Every entry of dZ within ten times the host's own discrepancy at the input set, relative to max|dZ|; hyperparameters and
    K_up_to_date as they were."""
    gp = case_gp(g, name, method, chunk)
    theta = np.array(gp.free_params[:], dtype=float)
    dz = gp.inducing_gradient()
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    err = dz_error(dz, name, method)
    print("%s %s chunk %s: device - exact = %.3g of max|dZ| = %.5g (bound %.3g)" % (name, method, chunk, err, np.abs(host_dz(name, method)).max(),
                                                                                     SZ.bound(name)))
    assert err <= SZ.bound(name), (err, SZ.bound(name))


# ---- (3) against central differences of the device value in Z -----------------------------------------------------------------------------
def data_1d(N=300, M=24, nder=30):
    X, n, y = S.inputs(N, 1, nder=nder)
    Z = np.random.RandomState(97).rand(M, 1)
    return X, n, y, Z


def check_against_fd_in_z(make, label, nsample=6):
    gp = make()
    dz = gp.inducing_gradient()
    assert gp._fit_mode == "sparse" and np.all(np.isfinite(dz))
    Z0 = gp.Z.copy()
    theta = np.array(gp.free_params[:], dtype=float)
    flat = np.argsort(-np.abs(dz).ravel())
    pick = list(flat[:2]) + list(np.random.RandomState(11).permutation(flat[2:])[:nsample - 2])
    fd, got = [], []
    for i in pick:
        m, dim = np.unravel_index(int(i), dz.shape)
        h = 1e-5 * max(1.0, abs(Z0[m, dim]))
        val = []
        for sign in (1.0, -1.0):
            Zq = Z0.copy()
            Zq[m, dim] += sign * h
            gp.set_inducing(Zq, gp.n_Z)
            val.append(-gp.update_hyperparameters(theta))
        fd.append((val[0] - val[1]) / ((Z0[m, dim] + h) - (Z0[m, dim] - h)))
        got.append(dz[m, dim])
    fd, got = np.array(fd), np.array(got)
    print("%s: %d coordinates, max|fd| = %.4g, max|dZ - fd| / max|fd| = %.3g" % (label, len(pick), np.abs(fd).max(),
                                                                                 np.abs(got - fd).max() / np.abs(fd).max()))
    np.testing.assert_allclose(got, fd, rtol=2e-5, atol=1e-4 * np.abs(fd).max(), err_msg=label)
    return gp


def test_fd_matern52_without_orders_among_z(g):
    check_against_fd_in_z(lambda: case_gp(g, "m52_m520", "fitc", None), "m52_m520 fitc")


def test_fd_periodic(g):
    X, n, y, Z = data_1d(nder=0)
    check_against_fd_in_z(lambda: g.SparseGaussianProcess(
        g.PeriodicKernel(num_dim=1, initial_params=[1.0, 0.9, 0.8], param_bounds=[(1e-2, 10.0)] * 3), Z, noise_k=noise(g, 1), method="fitc",
        X=X, y=y, err_y=0.05, n=n), "periodic")


def test_fd_se_times_matern52(g):
    d = S.case_data("se_300")
    k = kernel_of(g, [("se", [1.0, 1.5, 0.8], "m52", [0.7, 0.9, 1.3])], 2)
    check_against_fd_in_z(lambda: g.SparseGaussianProcess(k, d["Z"], noise_k=noise(g, 2), method="vfe", chunk_rows=128, X=d["X"], y=d["y"],
                                                          err_y=d["err_y"], n=d["n"]), "se * m52 vfe")


def test_fd_gibbs_tanh(g):
    X, n, y, Z = data_1d()
    check_against_fd_in_z(lambda: g.SparseGaussianProcess(
        g.GibbsKernel1dTanh(initial_params=[1.1, 0.3, 0.6, 0.2, 0.5], param_bounds=[(-10.0, 10.0)] * 5), Z, noise_k=noise(g, 1), method="vfe",
        X=X, y=y, err_y=0.05, n=n), "gibbs tanh")


def test_fd_with_a_mean_function(g):
    d = S.case_data("se_300")
    check_against_fd_in_z(lambda: g.SparseGaussianProcess(
        g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3), d["Z"], noise_k=noise(g, 2),
        mu=g.LinearMeanFunction(num_dim=2, initial_params=[0.2, -0.1, 0.05]), method="fitc", X=d["X"], y=d["y"], err_y=d["err_y"],
        n=np.zeros_like(d["n"])), "linear mean fitc")


# ---- (4) chunking and determinism ----------------------------------------------------------------------------------------------------
def stencil_of(theta, rel=6e-6):
    pa, pb, dn = [], [], []
    for h in range(len(theta)):
        ta, tb, den = SG.stencil(theta, h, rel)
        pa.append(ta)
        pb.append(tb)
        dn.append(den)
    return [0] * len(theta), pa, pb, dn


@pytest.mark.parametrize("method", SG.METHODS)
def test_five_chunks_against_the_default_chunk(g, method):
    """se_300 in chunks of 64 rows (five, the last one 44 rows) and in one chunk: each within the bound of (2)."""
    a, b = case_gp(g, "se_300", method, 64).inducing_gradient(), case_gp(g, "se_300", method, None).inducing_gradient()
    ea, eb = dz_error(a, "se_300", method), dz_error(b, "se_300", method)
    print("%s: chunk 64 %.3g, default %.3g of max|dZ| (bound %.3g); the two differ by %.3g" % (
        method, ea, eb, SZ.bound("se_300"), np.abs(a - b).max() / np.abs(b).max()))
    assert ea <= SZ.bound("se_300") and eb <= SZ.bound("se_300")


@pytest.mark.parametrize("method", SG.METHODS)
def test_equal_bits_and_everything_else_left_alone(g, method):
    """gpt_fit, gpt_sparse_fit, gpt_sparse_grad_diff and two gpt_sparse_grad_z on ONE context: the two calls give equal bits, out and
    alpha_out are gpt_sparse_grad_diff's bit for bit, nh = 0 gives the noise entry and the same dZ, and no bit of c, of a sparse
    prediction or of the dense factor's predictions changes."""
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
    out0, alpha0 = ctx.sparse_grad_diff(tix, pa, pb, dn, d["y"], d["err_y"], want_alpha=True)
    out1, alpha1, dz1 = ctx.sparse_grad_z(tix, pa, pb, dn, d["y"], d["err_y"], want_alpha=True)
    out2, alpha2, dz2 = ctx.sparse_grad_z(tix, pa, pb, dn, d["y"], d["err_y"], want_alpha=True)
    assert np.array_equal(dz1, dz2) and np.array_equal(out1, out2) and np.array_equal(alpha1, alpha2)
    assert np.array_equal(out1, out0) and np.array_equal(alpha1, alpha0) and np.all(np.isfinite(out1))
    assert np.array_equal(ctx.sparse_grad_diff(tix, pa, pb, dn, d["y"], d["err_y"])[0], out0)
    err = dz_error(dz1, "se_300", method)
    print("%s: dZ device - exact = %.3g of max|dZ| (bound %.3g)" % (method, err, SZ.bound("se_300")))
    assert err <= SZ.bound("se_300")
    # nh = 0: the noise entry alone, and dZ -- the same pair passes in the same order, so the same bits
    outn, none, dzn = ctx.sparse_grad_z([], [], [], [], d["y"], d["err_y"])
    assert none is None and outn.shape == (1,) and outn[0] == out1[3] and np.array_equal(dzn, dz1)
    assert np.array_equal(ctx.sparse_get_c(), c0)
    for a, b in zip(sp_before, ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(a, b)
    for a, b in zip(dense_before, ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_one_call_of_sparse_gradient_with_inducing(g):
    gp = case_gp(g, "se_m63", "vfe", 64)
    grad, dz = gp.sparse_gradient(inducing=True)
    assert np.array_equal(grad, gp.sparse_gradient()) and np.array_equal(dz, gp.inducing_gradient())


# ---- (5) refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library(g):
    """Each before any launch, with the library's message; the fit itself is accepted in every case."""
    from gptools_amd import _lib
    gp = case_gp(g, "m52_m300", "fitc", 256)                      # derivative rows among Z: fine for the fit and its gradient ...
    assert np.all(np.isfinite(gp.sparse_gradient()))
    with pytest.raises(ValueError, match="Matern52Kernel only supports 0th and 1st order derivatives"):
        gp.inducing_gradient()                                    # ... the raised orders are 2
    X, n, y, Z = data_1d()
    nZ = np.zeros((len(Z), 1), dtype=int)
    nZ[-3:, 0] = 1
    gp = g.SparseGaussianProcess(g.GibbsKernel1dTanh(initial_params=[1.1, 0.3, 0.6, 0.2, 0.5], param_bounds=[(-10.0, 10.0)] * 5), Z, n_Z=nZ,
                                 noise_k=noise(g, 1), method="vfe", X=X, y=y, err_y=0.05, n=n)
    assert np.isfinite(gp.update_hyperparameters(np.array(gp.free_params[:], dtype=float)))
    with pytest.raises(NotImplementedError, match=r"Derivatives greater than \[1, 1\] are not supported!"):
        gp.inducing_gradient()
    # RationalQuadratic: orders 8 among Z meet 8 + 8 = 16 in the fit, 8 + 9 in this pass
    nZ = np.zeros((len(Z), 1), dtype=int)
    nZ[-1, 0] = 8
    ctx = _lib.Context()
    ctx.set_data(X, np.zeros_like(n))
    ctx.sparse_set_inducing(Z, nZ)
    ctx._sparse_nparams = [3]
    with pytest.raises(_lib.GPTBackendError, match=r"gpt_sparse_grad_z needs a sparse fit .*\(code %d\)" % _lib.GPT_E_STATE):
        ctx.sparse_grad_z([], [], [], [], y, np.full(len(y), 0.05))
    ctx.sparse_fit(1, [(_lib.KERNEL_RQ, [1.0, 1.7, 3.0])], 0.01, y, np.full(len(y), 0.05), 1e-6)
    assert np.all(np.isfinite(ctx.sparse_grad_diff([], [], [], [], y, np.full(len(y), 0.05))[0]))
    with pytest.raises(ValueError, match="derivative orders of a pair sum to 18"):
        ctx.sparse_grad_z([], [], [], [], y, np.full(len(y), 0.05))
    ctx.set_T(np.eye(len(y)))
    with pytest.raises(NotImplementedError, match=r"gpt_sparse_grad_z is not available with a linear transform set"):
        ctx.sparse_grad_z([], [], [], [], y, np.full(len(y), 0.05))


# ---- (6) optimize_inducing ----------------------------------------------------------------------------------------------------------------
def test_optimize_inducing(g):
    """N = 300, D = 1, M = 10, SE, vfe, Z started at random points of the box.  The objective rises, Z stays in the box, the
    hyperparameters are untouched; scipy with central differences of the device value (the step of (3)) from the same start ends
    within ftol of the same objective; joint=True from that optimum ends no lower.

    ftol = 1e-9 is L-BFGS-B's, relative to |f| = 343: the two runs are held to ftol |f| = 3.4e-7 of each other.  What the yardstick
    itself can reach: a central difference of the device value carries cond(K_uu + jitter I) u |f| / 2 h = 1e7 * 1.1e-16 * 343 / 2e-5
    = 2e-2 per coordinate, and a descent along a gradient that wrong stops about M dg^2 / (2 f'') = 10 * 4e-4 / (2 * 5e3) = 4e-7 short
    (f'' from max|dZ| = 500 over a length scale of 0.1).  Measured on the MI355X: 343.484415029 in 27 evaluations against 343.484415342
    in 39, 3.1e-7 apart.  (A looser ftol does not serve: at 1e-8 the central-difference run stops after 28 evaluations at
    343.484397476, 1.8e-5 short of the same 343.484415029 -- the stopping rule bounds the last step's gain, not the distance left.)"""
    import scipy.optimize
    X, n, y = S.inputs(300, 1, nder=0)
    lo, hi = X.min(), X.max()
    Z0 = lo + (hi - lo) * np.random.RandomState(3).rand(10, 1)
    ftol = 1e-9

    def make():
        return g.SparseGaussianProcess(g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(1e-2, 10.0)] * 2), Z0,
                                       noise_k=g.DiagonalNoiseKernel(num_dim=1, initial_noise=0.1, noise_bound=(1e-3, 5.0)), method="vfe",
                                       X=X, y=y, err_y=0.02, n=n)
    gp = make()
    theta = np.array(gp.free_params[:], dtype=float)
    start = -gp.update_hyperparameters(theta)
    res = gp.optimize_inducing(opt_kwargs={"options": {"ftol": ftol, "gtol": 1e-8}})
    end = -gp.update_hyperparameters(theta)
    assert end == -res.fun and end > start and res.success, res
    assert np.all(gp.Z >= lo) and np.all(gp.Z <= hi) and np.array_equal(gp.Z.ravel(), res.x)
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and np.array_equal(gp.n_Z, np.zeros((10, 1), dtype=int))
    # the same method on central differences of the value
    ref = make()

    def value(z):
        ref.set_inducing(np.array(z, dtype=float).reshape(10, 1), ref.n_Z)
        return ref.update_hyperparameters(theta)

    def fd(z):
        out = np.zeros(len(z))
        for i in range(len(z)):
            h = 1e-5 * max(1.0, abs(z[i]))
            zp, zm = np.array(z, dtype=float), np.array(z, dtype=float)
            zp[i], zm[i] = min(z[i] + h, hi), max(z[i] - h, lo)
            out[i] = (value(zp) - value(zm)) / (zp[i] - zm[i])
        return out
    res_fd = scipy.optimize.minimize(value, Z0.ravel(), method="L-BFGS-B", jac=fd, bounds=[(lo, hi)] * 10, options={"ftol": ftol, "gtol": 1e-8})
    print("start %.10g, optimize_inducing %.12g (%d evaluations), central differences %.12g (%d evaluations)"
          % (start, -res.fun, res.nfev, -res_fd.fun, res_fd.nfev))
    assert abs(res.fun - res_fd.fun) <= ftol * max(abs(res.fun), abs(res_fd.fun), 1.0)
    # joint: from the optimum over Z, hyperparameters and Z together
    res_j = gp.optimize_inducing(joint=True, opt_kwargs={"options": {"ftol": ftol, "gtol": 1e-8}})
    print("joint from there: %.12g (%d evaluations), hyperparameters %s" % (-res_j.fun, res_j.nfev, gp.free_params[:]))
    assert res_j.fun <= res.fun and np.all(gp.Z >= lo) and np.all(gp.Z <= hi)
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), res_j.x[:3]) and np.array_equal(gp.Z.ravel(), res_j.x[3:])
    assert -gp.update_hyperparameters(np.array(gp.free_params[:], dtype=float)) == -res_j.fun
