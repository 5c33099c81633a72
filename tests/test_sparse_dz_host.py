"""Host suite (no GPU) of the inducing-input gradient: the yardstick of tests/test_gpu_sparse_dz.py and what needs no device.

test_host_form_against_the_dense_route is the measurement behind sparse_dz_cases.DZ_ERR; test_against_central_differences holds the
host's form against central differences in Z of the dense N(r; 0, Q_ff + Lambda) log-density, the definition of the objective; the
plumbing tests run SparseGaussianProcess against a context that records its calls and answers with a quadratic objective."""
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_grad_cases as SG
import sparse_dz_cases as SZ
from test_sparse_grad_host import small_case, FD_ERR


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.mark.parametrize("name", sorted(SZ.CASES))
def test_host_form_against_the_dense_route(oracle, name):
    """The adjoint form contracted with the oracle's blocks at the raised orders against the dense route, coordinate by coordinate at
    the sample (the two largest entries among it): the figure DZ_ERR records, printed in the form the table holds it."""
    d = S.case_data(name)
    worst = 0.0
    for method in S.CASES[name]["methods"]:
        b, s, adj, up = SZ.setup(oracle, name, method)
        dz = SZ.exact_dz(adj, up)
        assert np.all(np.isfinite(dz)) and np.abs(dz).max() > 0.0
        pick = SZ.sample(dz)
        top = np.sort(np.abs(dz).ravel())[::-1][:2]
        assert len(pick) >= min(SZ.SAMPLE, dz.size) and all(abs(dz[pick[q]]) == top[q] for q in range(min(2, dz.size)))
        for m, dim in pick:
            err = abs(dz[m, dim] - SZ.dense_entry(b, d["y"], s, method, up, m, dim)) / np.abs(dz).max()
            worst = max(worst, err)
    print('    "%s": %.3g,' % (name, worst))
    # both routes carry cond(K_uu + jitter I) u = 1e8 * 1e-16 = 1e-8 of their largest intermediate (ROUTES_TOL of
    # tests/test_sparse_grad_host.py, the same two routes): the table may hold nothing larger than that estimate with its margin of ten
    assert SZ.DZ_ERR[name] <= 1e-7
    assert worst <= SZ.bound(name), (worst, SZ.bound(name))      # the host holds the bound the device is held to


# ---- central differences of the definition, in extended precision ------------------------------------------------------------------
# The dense log-density in double precision carries a rounding of cond(K_uu + jitter I) u |ll| = 1e-8 absolute here, and d ll / d Z is
# differenced over 2 h = 2e-5: measured with sparse_cases.dense, h = 1e-3 ... 1e-6: 2.7e-4, 2.7e-6 (the truncation, h^2), then 1.1e-6
# and 8.5e-6 (the rounding, 1 / h) of max|dZ| = 566 -- no step brings that reference under the 1e-7 this comparison is held to.  The
# reference is therefore the SAME density -- the SE covariance with the case's first-order rows, (K_uu + jitter I)^-1 K_uf, Cholesky of
# Q_ff + Lambda -- restated in numpy.longdouble from the formulas alone (u = 5e-20 where long double is the x87 format; no LAPACK): its
# rounding is 2000 times smaller and h = 1e-5 leaves the truncation, 2.7e-8.
LD = np.longdouble


def se_block_ld(theta, Xi, ni, Xj, nj):
    """SE covariance [sigma_f, l_1 .. l_D] between points whose derivative orders are 0, or 1 in coordinate 0."""
    assert ni[:, 1:].max() == 0 and nj[:, 1:].max() == 0 and ni.max() <= 1 and nj.max() <= 1
    sig, l = LD(theta[0]), np.array(theta[1:], dtype=LD)
    tau = Xi.astype(LD)[:, None, :] - Xj.astype(LD)[None, :, :]
    k = sig * sig * np.exp(-((tau / l) ** 2).sum(-1) / LD(2))
    t0 = tau[..., 0] / (l[0] * l[0])
    a, b = (ni[:, 0] == 1)[:, None], (nj[:, 0] == 1)[None, :]
    return k * np.where(a & b, 1 / (l[0] * l[0]) - t0 * t0, np.where(a, -t0, np.where(b, t0, LD(1))))


def chol_ld(A):
    L = np.zeros_like(A)
    for j in range(len(A)):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def lower_solve_ld(L, B):
    Y = np.zeros_like(B)
    for i in range(len(L)):
        Y[i] = (B[i] - L[i, :i].dot(Y[:i])) / L[i, i]
    return Y


def dense_ll_ld(theta, X, n, Z, nZ, y, s, method, jitter=S.JITTER):
    """log N(y; 0, Q_ff + Lambda) (- the trace term, vfe) of sparse_cases.dense in extended precision."""
    M = len(Z)
    Lu = chol_ld(se_block_ld(theta, Z, nZ, Z, nZ) + LD(jitter) * np.eye(M, dtype=LD))
    V = lower_solve_ld(Lu, se_block_ld(theta, Z, nZ, X, n))
    kd = np.array([se_block_ld(theta, X[i:i + 1], n[i:i + 1], X[i:i + 1], n[i:i + 1])[0, 0] for i in range(len(X))])
    kmq = kd - (V * V).sum(0)
    s = s.astype(LD)
    lam = kmq + s if method == "fitc" else s
    Ls = chol_ld(V.T.dot(V) + np.diag(lam))
    w = lower_solve_ld(Ls, y.astype(LD)[:, None])[:, 0]
    ll = -(2 * np.log(np.diag(Ls)).sum() + w.dot(w) + len(y) * np.log(2 * LD(np.pi))) / 2
    return ll - ((kmq / s).sum() / 2 if method == "vfe" else 0)


@pytest.mark.parametrize("method", SG.METHODS)
def test_against_central_differences(oracle, method):
    """d ll / d Z of the small case of tests/test_sparse_grad_host.py, every coordinate, against central differences in Z of the dense
    log-density (extended precision, see above) with h = 1e-5 max(1, |z|); the tolerance is that file's for its own central-difference
    test.  The extended-precision density is first held to sparse_cases.dense at Z itself."""
    X, n, y, Z, nZ, err = small_case()
    terms = [("se", list(S.SE2))]
    s = S.NOISE ** 2.0 + err ** 2.0
    b = dict(Kuu=S.gram(oracle, terms, Z, nZ, Z, nZ), Kuf=S.gram(oracle, terms, Z, nZ, X, n), kd=S.kdiag(oracle, terms, X, n),
             Kus=np.zeros((len(Z), 1)), Kss=np.zeros((1, 1)))
    ll0 = S.dense(b, y, s, method)["ll"]
    assert abs(float(dense_ll_ld(S.SE2, X, n, Z, nZ, y, s, method)) - ll0) <= 1e-8 * abs(ll0)      # cond u = 1e-9 of it
    adj = SG.adjoints(b, y, s, method)
    up = []
    for dim in range(2):
        e = nZ.copy()
        e[:, dim] += 1
        up.append((S.gram(oracle, terms, Z, e, X, n), S.gram(oracle, terms, Z, e, Z, nZ)))
    got = SZ.exact_dz(adj, up)
    fd = np.zeros_like(got)
    for m in range(Z.shape[0]):
        for dim in range(2):
            h = 1e-5 * max(1.0, abs(Z[m, dim]))
            Zp, Zm = Z.copy(), Z.copy()
            Zp[m, dim] += h
            Zm[m, dim] -= h
            fd[m, dim] = float((dense_ll_ld(S.SE2, X, n, Zp, nZ, y, s, method) - dense_ll_ld(S.SE2, X, n, Zm, nZ, y, s, method))
                               / LD(Zp[m, dim] - Zm[m, dim]))
    rel = np.abs(got - fd).max() / np.abs(fd).max()
    print('"%s": %.3g   (max|dZ| %.5g)' % (method, rel, np.abs(fd).max()))
    assert rel <= 10.0 * FD_ERR[method], (method, rel)


# ---- the Python layer against a context that records -------------------------------------------------------------------------------
class _Recorder(object):
    """Stands in for the library's context.  The 'objective' is -|Z - target|^2 - |p - P0|^2 over the kernel's parameters p: the
    gradient entries come back through the stencil (exact for a quadratic), dZ = -2 (Z - target)."""
    _warp_key = None
    P0 = np.array([1.4, 0.3, 0.9])

    def __init__(self, target, fail_at=None):
        self.calls, self.target, self.fail_at, self.grads = [], np.asarray(target, dtype=float), fail_at, 0

    def set_data(self, X, n):
        self.calls.append("set_data")

    def set_warp(self, layers):
        pass

    def sparse_set_inducing(self, Z, nZ=None):
        self.calls.append("sparse_set_inducing")
        self.Z = np.array(Z, dtype=float)

    def _value(self, p):
        return -((self.Z - self.target) ** 2).sum() - ((np.asarray(p, dtype=float) - self.P0) ** 2).sum()

    def sparse_fit(self, method, terms, noise_var, y, err_y, jitter, chunk_rows=0):
        self.calls.append("sparse_fit")
        self.p = np.array(terms[0][1], dtype=float)
        return self._value(self.p), np.zeros(5)

    def sparse_grad_z(self, term_idx, params_a, params_b, denom, y, err_y, want_alpha=False):
        self.calls.append("sparse_grad_z")
        self.grads += 1
        if self.fail_at is not None and self.grads >= self.fail_at:
            raise RuntimeError("the recorder was told to fail here")
        out = np.array([(self._value(b) - self._value(a)) / dn for a, b, dn in zip(params_a, params_b, denom)] + [0.0])
        return out, None, -2.0 * (self.Z - self.target)


def recorded_gp(g, target, fail_at=None):
    d = S.case_data("se_300")
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3)
    gp = g.SparseGaussianProcess(k, d["Z"][:5], noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=S.NOISE, noise_bound=(0.0, 5.0)),
                                 method="vfe", X=d["X"], y=d["y"], err_y=0.02, n=d["n"])
    gp._ctx_obj = _Recorder(target, fail_at)
    return gp, d


def test_new_names(g):
    for name in ("inducing_gradient", "optimize_inducing"):
        assert callable(getattr(g.SparseGaussianProcess, name))
    assert hasattr(g._lib.Context, "sparse_grad_z")
    assert "gpt_sparse_grad_z" in g._lib.SIGNATURES and "gpt_dev_sparse_grad_dz_pairs" in g._lib.SIGNATURES


def test_set_inducing_after_an_upload_sends_the_inducing_inputs_alone(g):
    gp, d = recorded_gp(g, np.zeros((5, 2)))
    gp.compute_K_L_alpha_ll()
    assert gp._ctx.calls == ["set_data", "sparse_set_inducing", "sparse_fit"]
    gp.set_inducing(d["Z"][5:10])
    assert not gp.K_up_to_date
    gp.compute_K_L_alpha_ll()
    assert gp._ctx.calls[3:] == ["sparse_set_inducing", "sparse_fit"] and np.array_equal(gp._ctx.Z, d["Z"][5:10])
    gp.compute_K_L_alpha_ll()                                    # nothing changed: nothing sent
    assert len(gp._ctx.calls) == 5
    gp.add_data(d["X"][:3], d["y"][:3], err_y=0.02)              # new data: both go again, the data first
    gp.compute_K_L_alpha_ll()
    assert gp._ctx.calls[5:] == ["set_data", "sparse_set_inducing", "sparse_fit"]


def test_inducing_gradient_and_the_one_call_of_sparse_gradient(g):
    gp, d = recorded_gp(g, np.full((5, 2), 0.25))
    theta = np.array(gp.free_params[:], dtype=float)
    dZ = gp.inducing_gradient()
    assert dZ.shape == (5, 2) and np.array_equal(dZ, -2.0 * (d["Z"][:5] - 0.25))
    assert np.array_equal(np.array(gp.free_params[:], dtype=float), theta) and gp.K_up_to_date
    before = gp._ctx.calls.count("sparse_grad_z")
    grad, dZ2 = gp.sparse_gradient(inducing=True)
    assert gp._ctx.calls.count("sparse_grad_z") == before + 1 and np.array_equal(dZ2, dZ)
    np.testing.assert_allclose(grad[:3], -2.0 * (np.array(S.SE2) - _Recorder.P0), rtol=1e-9)
    gp._ctx.target = np.full((5, 2), np.nan)
    with pytest.raises(FloatingPointError):
        gp.inducing_gradient()


@pytest.mark.parametrize("joint", [False, True])
def test_optimize_inducing_packs_unpacks_and_boxes(g, joint):
    """Z alone, then [theta, vec(Z)]: the optimum of the recorder's quadratic is the target inside the box and the box's edge outside;
    the hyperparameters move to P0 with joint=True and stay with joint=False."""
    target = np.array([[0.2, 0.3], [0.5, 0.6], [0.7, 0.1], [-3.0, 0.4], [0.9, 7.0]])
    gp, d = recorded_gp(g, target)
    theta0, nZ0 = np.array(gp.free_params[:], dtype=float), gp.n_Z.copy()
    res = gp.optimize_inducing(joint=joint)
    lo, hi = d["X"].min(0), d["X"].max(0)
    want = np.clip(target, lo, hi)
    assert res.x.shape == ((4 if joint else 0) + 10,)
    np.testing.assert_allclose(gp.Z, want, atol=1e-5)
    assert np.all(gp.Z >= lo) and np.all(gp.Z <= hi) and np.array_equal(gp.Z, res.x[-10:].reshape(5, 2))
    assert gp.Z[3, 0] == lo[0] and gp.Z[4, 1] == hi[1] and np.array_equal(gp.n_Z, nZ0)
    theta = np.array(gp.free_params[:], dtype=float)
    if joint:
        np.testing.assert_allclose(theta[:3], _Recorder.P0, atol=1e-5)
        assert np.array_equal(theta, res.x[:4]) and theta[3] == theta0[3]      # (the recorder's objective ignores the noise)
    else:
        assert np.array_equal(theta, theta0)
    assert gp.K_up_to_date and np.array_equal(gp._ctx.Z, gp.Z) and np.array_equal(gp._ctx.p, theta[:3])
    assert gp._ctx.calls.count("set_data") == 1                  # every step sent Z alone


def test_optimize_inducing_boxes_given_by_the_caller_and_refusals(g):
    target = np.full((5, 2), 0.5)
    gp, d = recorded_gp(g, target)
    gp.optimize_inducing(bounds=[(0.0, 0.4), (0.6, 1.0)])
    np.testing.assert_allclose(gp.Z, np.tile([0.4, 0.6], (5, 1)), atol=1e-12)
    box = np.zeros((5, 2, 2))
    box[..., 1] = 1.0
    box[2, 1] = (0.1, 0.2)
    gp.optimize_inducing(bounds=box)
    want = target.copy()
    want[2, 1] = 0.2
    np.testing.assert_allclose(gp.Z, want, atol=1e-5)
    for bad in (np.zeros((3, 2)), [(1.0, 0.0), (0.0, 1.0)]):
        with pytest.raises(ValueError):
            gp.optimize_inducing(bounds=bad)
    with pytest.raises(ValueError):
        gp.optimize_inducing(opt_kwargs={"jac": True})


@pytest.mark.parametrize("joint", [False, True])
def test_optimize_inducing_restores_state_after_an_exception(g, joint):
    gp, d = recorded_gp(g, np.full((5, 2), 0.5), fail_at=3)
    theta0 = np.array(gp.free_params[:], dtype=float)
    with pytest.raises(RuntimeError):
        gp.optimize_inducing(joint=joint)
    assert gp._ctx.grads == 3
    assert np.array_equal(gp.Z, d["Z"][:5]) and np.array_equal(np.array(gp.free_params[:], dtype=float), theta0)
    assert not gp.K_up_to_date
