"""GPU suite: input-warped kernels on the device route (gpt_set_warp: warp_points_kernel + the WARP builder) -- pair lists, Gram
matrices, ll, alpha and predictions against the reference (tests/golden/g16_warp.npz) and against the host class
(Python-kernel route); identities that need no fixture; context state and refusals; the batched fit with per-element warps
(gpt_set_warp_batch) bit for bit against single warped fits; ll_batch / compute_ll_matrix / the MAP.

Largest deviations from the fixture measured on MI355X (the bounds below are at most 10x these, and never more than 10x the
unwarped tests' for the same quantity): pairs 1.5e-12 relative (SE with orders in several dimensions; M52 3.4e-13, RQ 2.6e-13,
sum 6.1e-13, product 7.1e-14); ll 1.7e-13 relative; as a fraction of the largest reference entry: alpha 2.1e-12, mean 3.6e-12,
cov 7.1e-13, std 1.6e-12; the compute_ll_matrix grid 5.8e-14 relative."""
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, assert_close, assert_close_nan

sys.path.insert(0, GOLDEN)
import gen_g16_warp as G16      # noqa: E402

pytestmark = pytest.mark.gpu

# tests/test_gpu_parity.py's tolerances for the same inner kernel: 1e-11 ... 1e-12 for pairs
PAIR_TOL = {"se": dict(rtol=1e-11), "m52": dict(rtol=1e-11), "rq": dict(rtol=1e-11, atol_scale=1e-13),
            "sum": dict(rtol=1e-11), "prod": dict(rtol=1e-11, atol_scale=1e-13)}


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def _scaled(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def _fit(golden, D):
    G = golden("g16_warp")
    return G, {k[len("fit_d%d__" % D):]: v for k, v in G.items() if k.startswith("fit_d%d__" % D)}


def _host_twin(g, k):
    """The same kernel object behind a subclass that overrides __call__: a Python kernel, evaluated by the host class."""
    class HostWarped(g.WarpedKernel):
        def __call__(self, *a, **kw):
            return g.WarpedKernel.__call__(self, *a, **kw)
    return HostWarped(k.k, k.w)


@pytest.mark.parametrize("D", G16.DIMS)
@pytest.mark.parametrize("warp", G16.WARPS)
@pytest.mark.parametrize("inner", G16.INNERS)
def test_device_pairs_match_reference_and_host_class(g, golden, inner, warp, D):
    G = golden("g16_warp")
    p = {k: G["pairs_%s_%s_d%d__%s" % (inner, warp, D, k)] for k in ("xi", "xj", "ni", "nj", "k")}
    ni, nj = p["ni"].astype(int), p["nj"].astype(int)
    k = G16.make_kernel(g, inner, warp, D)
    gp = g.GaussianProcess(k, X=p["xi"], y=np.zeros(len(p["xi"])), n=ni)
    assert gp._device_model() is not None
    K = gp.compute_Kij(p["xi"], p["xj"], ni, nj)                       # gpt_kbuild on the warped model
    assert gp._ctx._warp_key is not None
    nz = p["k"] != 0
    print("pairs %s %s %d: %.3g" % (inner, warp, D, np.max(np.abs(np.diagonal(K) - p["k"])[nz] / np.abs(p["k"][nz]))))
    assert_close(np.diagonal(K), p["k"], msg="device vs reference", **PAIR_TOL[inner])
    host = k(p["xi"], p["xj"], ni, nj)                                # the host class around the device pair list
    assert_close(np.diagonal(K), host, msg="device vs host class", **PAIR_TOL[inner])
    Ks = gp.compute_Kij(p["xi"], None, ni, None)
    M = len(ni)
    Kh = k(np.repeat(p["xi"], M, axis=0), np.tile(p["xi"], (M, 1)), np.repeat(ni, M, axis=0), np.tile(ni, (M, 1))).reshape(M, M)
    assert_close(Ks, Kh, msg="symmetric Gram vs host class", **PAIR_TOL[inner])


@pytest.mark.parametrize("D", G16.DIMS)
def test_edges_nan_for_nan(g, golden, D):
    G = golden("g16_warp")
    xi, xj, want = G["edge_d%d__xi" % D], G["edge_d%d__xj" % D], G["edge_d%d__k" % D]
    z = np.zeros((12, D), dtype=int)
    gp = g.GaussianProcess(G16.make_kernel(g, "se", "beta", D), X=xi, y=np.zeros(12))
    got = np.diagonal(gp.compute_Kij(xi, xj, z, z))
    assert np.isnan(want).sum() == 3
    assert_close_nan(got, want, rtol=1e-11)


@pytest.mark.parametrize("D", G16.DIMS)
@pytest.mark.parametrize("case", G16.FIT_CASES)
def test_fit_and_predict_match_reference_and_host_route(g, golden, case, D):
    G, d = _fit(golden, D)
    key = "fit_%s_d%d__" % (case, D)
    gp = G16.make_fit_gp(g, case, D, d)
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    _, Xs = G16.fit_points(case, d, D)
    print(key, "K %.3g ll %.3g alpha %.3g" % (_scaled(gp.K, G[key + "K"]), abs(gp.ll - G[key + "ll"]) / abs(G[key + "ll"]),
                                              _scaled(gp.alpha.ravel(), G[key + "alpha"])))
    assert_close(gp.K, G[key + "K"], rtol=1e-11, atol_scale=1e-13, msg="K")
    assert abs(gp.ll - G[key + "ll"]) <= 1.5e-12 * abs(G[key + "ll"])
    assert _scaled(gp.alpha.ravel(), G[key + "alpha"]) <= 2e-11
    mean, cov = gp.predict(Xs, n=d["ns"], return_std=False, return_cov=True)
    m0, s0 = gp.predict(Xs, n=0)
    print(key, "mean %.3g cov %.3g std0 %.3g" % (_scaled(mean, G[key + "mean"]), _scaled(cov, G[key + "cov"]),
                                                 _scaled(s0, G[key + "std0"])))
    assert _scaled(mean, G[key + "mean"]) <= 3e-11 and _scaled(m0, G[key + "mean0"]) <= 3e-11
    assert _scaled(cov, G[key + "cov"]) <= 7e-12
    assert _scaled(s0, G[key + "std0"]) <= 1.6e-11
    if case == "noise":
        _, sn = gp.predict(Xs, n=0, noise=True)
        assert _scaled(sn, G[key + "std0_noise"]) <= 1.6e-11
    # the same model through the host class (Python-kernel route: pair list on the host, gpt_fit_matrix)
    gh = G16.make_fit_gp(g, case, D, d)
    gh.k = _host_twin(g, gh.k)
    assert gh._device_model() is None
    gh.compute_K_L_alpha_ll()
    assert gh._fit_mode == "matrix"
    assert abs(gh.ll - gp.ll) <= 1e-9 * abs(gp.ll)
    mh, ch = gh.predict(Xs, n=d["ns"], return_std=False, return_cov=True)
    np.testing.assert_allclose(mh, mean, rtol=0, atol=1e-9 * max(1.0, np.max(np.abs(mean))))
    np.testing.assert_allclose(ch, cov, rtol=0, atol=2e-10 * max(1.0, np.max(np.abs(cov))))


def _raw_fit(ctx, terms, layers, X, n, y, err, noise_var=0.09, diag_add=1e-9, N=None):
    ctx.set_data(X, n)
    ctx.set_warp(layers)
    ll, ld = ctx.fit_terms(terms, noise_var, y, err, diag_add)
    N = len(y)
    return ll, ld, ctx.get_alpha(N), ctx.get_L(N)


def _identity_data(D, N=700):
    rs = np.random.RandomState(77 + D)
    X = rs.uniform(0.05, 0.95, (N, D))
    n = np.zeros((N, D), dtype=int)
    for r, d in zip(range(N - 150, N), rs.randint(0, D, 150)):
        n[r, d] = 1
    return X, n, rs.randn(N), rs.uniform(0.05, 0.2, N)


# Identities, measured on MI355X (largest over D = 1, 2, 3; alpha and L as a fraction of their largest entry), bounds 10x:
# beta(1, 1) layer against no layer: ll 1.3e-14, alpha 3.1e-13, L 2.1e-14; linear layer against the rescaled SE: ll 9e-16,
# alpha 3.1e-14, L 7.6e-15 (D = 3; exactly 0 for D = 1, 2, where b - a is a power of two)
B11_LL, B11_ALPHA, B11_L = 1.3e-13, 3.1e-12, 2.1e-13
LIN_LL, LIN_ALPHA, LIN_L = 9e-15, 3.1e-13, 7.6e-14


@pytest.mark.parametrize("D", [1, 2, 3])
def test_identity_layers(g, D):
    from gptools_amd import _lib
    X, n, y, err = _identity_data(D)
    p = np.array([1.2] + [0.3, 0.45, 0.6][:D])
    terms = [(_lib.KERNEL_SE, p), (_lib.KERNEL_M52, p * 0.9)]
    ctx = _lib.Context(0)
    base = _raw_fit(ctx, terms, None, X, n, y, err)
    # linear layer with a = 0, b = 1: w = x and w' = 1 exactly -> the same bits, derivative rows included
    unit = _raw_fit(ctx, terms, [(_lib.WARP_LINEAR, np.tile([0.0, 1.0], D))], X, n, y, err)
    assert ctx._warp_key is not None
    assert unit[0] == base[0] and unit[1] == base[1]
    assert np.array_equal(unit[2], base[2]) and np.array_equal(unit[3], base[3])
    # beta layer with alpha = beta = 1: w = x, w' = 1 to rounding
    b11 = _raw_fit(ctx, terms, [(_lib.WARP_BETA, np.ones(2 * D))], X, n, y, err)
    print("identity D %d beta(1,1): ll %.3g alpha %.3g L %.3g" % (D, abs(b11[0] - base[0]) / abs(base[0]), _scaled(b11[2], base[2]),
                                                                  _scaled(b11[3], base[3])))
    assert abs(b11[0] - base[0]) <= B11_LL * abs(base[0])
    assert _scaled(b11[2], base[2]) <= B11_ALPHA and _scaled(b11[3], base[3]) <= B11_L
    # a linear layer (a, b) around SE = the unwarped SE with length scales l (b - a): slope factor, and its place in front of the
    # diagonal epilogue (noise_var, err_y and diag_add all non-zero)
    a, b = np.array([-1.0, 2.0, 0.5][:D]), np.array([3.0, 2.5, 10.0][:D])
    Xr = a + X * (b - a)
    lin = _raw_fit(ctx, [(_lib.KERNEL_SE, p)], [(_lib.WARP_LINEAR, np.column_stack((a, b)).ravel())], Xr, n, y, err)
    wide = _raw_fit(ctx, [(_lib.KERNEL_SE, np.concatenate(([p[0]], p[1:] * (b - a))))], None, Xr, n, y, err)
    print("identity D %d linear vs rescaled SE: ll %.3g alpha %.3g L %.3g" % (D, abs(lin[0] - wide[0]) / abs(wide[0]),
                                                                              _scaled(lin[2], wide[2]), _scaled(lin[3], wide[3])))
    assert abs(lin[0] - wide[0]) <= LIN_LL * abs(wide[0])
    assert _scaled(lin[2], wide[2]) <= LIN_ALPHA and _scaled(lin[3], wide[3]) <= LIN_L
    # state: clearing the layers, and new data, give the unwarped bits again
    again = _raw_fit(ctx, terms, None, X, n, y, err)
    assert again[0] == base[0] and np.array_equal(again[3], base[3])
    ctx.set_data(X, n)
    ctx.set_warp([(_lib.WARP_BETA, np.full(2 * D, 1.7))])
    ctx.set_data(X, n)                                        # drops the layers
    ll, _ = ctx.fit_terms(terms, 0.09, y, err, 1e-9)
    assert ll == base[0]


def test_state_and_refusals(g):
    from gptools_amd import _lib
    X, n, y, err = _identity_data(2, N=300)
    p = np.array([1.2, 0.3, 0.45])
    ctx = _lib.Context(0)
    ctx.set_option("debug_poison", 1)
    layers = [(_lib.WARP_LINEAR, [-0.5, 1.5, 0.0, 1.0]), (_lib.WARP_BETA, [0.7, 1.8, 2.0, 0.6])]
    ll, _, alpha, L = _raw_fit(ctx, [(_lib.KERNEL_SE, p)], layers, X, n, y, err)
    assert np.isfinite(ll) and np.isfinite(alpha).all() and np.isfinite(L).all()      # nothing of dXw / dS left unwritten
    mean, std, _ = ctx.predict(X[:37], n[:37], 1)
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    with pytest.raises(NotImplementedError, match="warp"):
        ctx.ll_grad([0], [0])
    with pytest.raises(NotImplementedError, match="warp"):
        ctx.fit_batch_terms([[(_lib.KERNEL_SE, p)]] * 2, np.zeros(2), np.tile(y, (2, 1)), err, 1e-9)
    with pytest.raises(NotImplementedError, match="warp"):
        ctx.predict_batch(X[:5], n[:5], np.ones(2, dtype=np.int32))
    # a batch with its own warps: the element count must match; the batch it leaves resident is not predicted from
    lb = [[(t, np.asarray(q) * (1.0 + 0.01 * b)) for t, q in layers] for b in range(2)]
    ctx.set_warp_batch(lb + lb[:1])
    with pytest.raises(ValueError, match="elements"):
        ctx.fit_batch_terms([[(_lib.KERNEL_SE, p)]] * 2, np.full(2, 0.09), np.tile(y, (2, 1)), err, 1e-9)
    ctx.set_warp(None)
    ctx.set_warp_batch(lb)
    llb, _, info = ctx.fit_batch_terms([[(_lib.KERNEL_SE, p)]] * 2, np.full(2, 0.09), np.tile(y, (2, 1)), err, 1e-9)
    assert (info == 0).all() and np.isfinite(llb).all()                 # (debug_poison on: nothing of the batch's points left unwritten)
    with pytest.raises(NotImplementedError, match="warps"):
        ctx.predict_batch(X[:5], n[:5], np.ones(2, dtype=np.int32))
    llu, _, info = ctx.fit_batch_terms([[(_lib.KERNEL_SE, p)]] * 2, np.full(2, 0.09), np.tile(y, (2, 1)), err, 1e-9)   # consumed: unwarped
    assert (info == 0).all() and llu[0] == llu[1] and llu[0] != llb[0]
    ctx.set_warp(layers)
    ctx.fit_terms([(_lib.KERNEL_SE, p)], 0.09, y, err, 1e-9)
    # order 2 in X*: refused before anything is launched; order 2 in the data: gpt_set_warp refuses
    n2 = n[:5].copy()
    n2[0, 0] = 2
    with pytest.raises(ValueError, match="greater than one"):
        ctx.predict(X[:5], n2, 0)
    with pytest.raises(ValueError, match="greater than one"):
        ctx.kbuild(_lib.KERNEL_SE, p, X[:5], n2)
    nn = n.copy()
    nn[3, 1] = 2
    ctx.set_data(X, nn)
    with pytest.raises(ValueError, match="greater than one"):
        ctx.set_warp(layers)
    ll2, _ = ctx.fit_terms([(_lib.KERNEL_SE, p)], 0.09, y, err, 1e-9)                # no layers were set: an unwarped fit
    assert np.isfinite(ll2)
    with pytest.raises(ValueError):
        ctx.set_warp([(3, [0.0, 1.0, 0.0, 1.0])])
    with pytest.raises(ValueError):
        ctx.set_warp([(_lib.WARP_LINEAR, [0.0, 1.0])])


@pytest.mark.parametrize("with_T", [False, True])
@pytest.mark.parametrize("model", ["one", "sum"])
@pytest.mark.parametrize("N", [200, 1000])
def test_batch_elements_carry_the_single_warped_fits_bits(g, N, model, with_T):
    """gpt_set_warp_batch + gpt_fit_batch_terms: element b = gpt_set_warp(b's layers) + gpt_fit_terms(b's parameters), bit for bit,
    with derivative rows, 1-term and sum models, with and without T; every element has other warp and kernel parameters."""
    from gptools_amd import _lib
    rs = np.random.RandomState(N + 7 * with_T + (3 if model == "sum" else 0))
    D, B = 2, 5
    a, b = np.array([-1.0, 2.0]), np.array([3.0, 2.5])
    X = a + rs.uniform(0.02, 0.98, (N, D)) * (b - a)
    n = np.zeros((N, D), dtype=int)
    for r, d in zip(range(N - N // 4, N), rs.randint(0, D, N // 4)):
        n[r, d] = 1
    Ny = N // 2 if with_T else N
    T = rs.uniform(0.0, 1.0, (Ny, N)) / N if with_T else None
    Y, err, nv = rs.randn(B, Ny), rs.uniform(0.05, 0.2, Ny), rs.uniform(0.01, 0.1, B)
    layers_list, terms_list = [], []
    for e in range(B):
        layers_list.append([(_lib.WARP_LINEAR, np.column_stack((a, b)).ravel()), (_lib.WARP_BETA, rs.uniform(0.5, 2.5, 2 * D))])
        terms = [(_lib.KERNEL_SE, np.array([1.0, 0.3, 0.4]) * rs.uniform(0.8, 1.2, 3))]
        if model == "sum":
            terms.append((_lib.KERNEL_M52, np.array([0.7, 0.5, 0.6]) * rs.uniform(0.8, 1.2, 3)))
        terms_list.append(terms)
    ctx = _lib.Context(0)
    ctx.set_data(X, n)
    if with_T:
        ctx.set_T(T)
    ctx.set_warp_batch(layers_list)
    ll, ld, info = ctx.fit_batch_terms(terms_list, nv, Y, err, 1e-9)
    assert (info == 0).all()
    for e in range(B):
        ctx.set_warp(layers_list[e])
        ll1, ld1 = ctx.fit_terms(terms_list[e], nv[e], Y[e], err, 1e-9)
        assert ll[e] == ll1 and ld[e] == ld1, (e, ll[e] - ll1, ld[e] - ld1)
    assert len(set(ll.tolist())) == B


def test_gp_routes_for_a_warped_model(g, golden):
    G, d = _fit(golden, 2)
    fixed = np.array([False] * 3 + [True] * 8)               # (hyperparameter derivatives exist for the inner kernel's parameters only)
    gp = G16.make_fit_gp(g, "se_lin_beta", 2, d, fixed=fixed)
    gp.partitioned = True
    assert not gp._partitioned_possible()
    gp.partitioned = False
    # analytic gradient: the general branch (host dK through the host class), never gpt_ll_grad
    gp.use_hyper_deriv = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gp.compute_K_L_alpha_ll()
    free = np.array(gp.free_params[:], dtype=float)
    gp.use_hyper_deriv = False
    for i in range(3):                                       # the inner kernel's parameters
        h = 1e-6 * free[i]
        up, dn = free.copy(), free.copy()
        up[i] += h
        dn[i] -= h
        fd = (gp.ll_batch([up])[0] - gp.ll_batch([dn])[0]) / (2 * h)
        assert abs(gp.ll_deriv[i] - fd) <= 1e-4 * max(1.0, abs(fd)), (i, gp.ll_deriv[i], fd)
    # predict_MCMC / compute_from_MCMC: the row-by-row loop
    gp = G16.make_fit_gp(g, "se_lin_beta", 2, d)
    free = np.array(gp.free_params[:], dtype=float)
    trace = np.tile(free, (3, 1)) * np.array([[1.0], [1.05], [0.95]])
    _, Xs = G16.fit_points("se_lin_beta", d, 2)
    out = gp.compute_from_MCMC(Xs, n=0, flat_trace=trace)
    gp.update_hyperparameters(trace[1])
    m1, s1 = gp.predict(Xs, n=0)
    np.testing.assert_allclose(out["mean"][1], m1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["std"][1], s1, rtol=0, atol=1e-12)
    # draw_sample runs on what predict left on the device
    u = np.random.RandomState(3).randn(len(Xs), 2)
    s = gp.draw_sample(Xs, rand_vars=u)
    assert s.shape == (len(Xs), 2) and np.isfinite(s).all()


def test_ll_batch_and_grid(g, golden):
    G, d = _fit(golden, 2)
    gp = G16.make_fit_gp(g, "se_lin_beta", 2, d, fixed=G["grid__fixed"])
    ll, pv = gp.compute_ll_matrix([(0.5, 2.5), (0.6, 3.0)], [4, 3])
    np.testing.assert_array_equal(pv[0], G["grid__p0"])
    print("grid: %.3g" % np.max(np.abs(ll - G["grid__ll"]) / np.abs(G["grid__ll"])))
    np.testing.assert_allclose(ll, G["grid__ll"], rtol=5e-13)
    # ll_batch takes the batched fit with per-element warps; every element carries the bits of the single warped fit
    for case, N in (("se_lin_beta", 200), ("sum_lin_beta", 1000)):
        rs = np.random.RandomState(N)
        D = 2
        dd = dict(U=rs.uniform(0.02, 0.98, (N, D)), y=rs.randn(N), n=np.zeros((N, D), dtype=int))
        dd["Us"] = dd["U"][:2]
        dd["n"][-N // 4:, 0] = 1
        gp = G16.make_fit_gp(g, case, D, dd)
        free = np.array(gp.free_params[:], dtype=float)
        plist = [free * (1.0 + 0.05 * rs.rand(len(free))) for _ in range(6)]
        calls, orig = [], gp._ctx.set_warp_batch
        gp._ctx.set_warp_batch = lambda ll_: (calls.append(len(ll_)), orig(ll_))[1]
        batch = gp.ll_batch(plist)
        assert calls == [6]                                  # the one-launch-sequence route with per-element warps
        single = np.array([-gp.update_hyperparameters(p) for p in plist])
        assert np.array_equal(batch, single), (case, batch - single)


def test_map_matches_host_route(g, golden):
    G, d = _fit(golden, 1)
    res = []
    for host in (False, True):
        lls = []
        for start in ([1.0, 0.3, 1.0, 1.0], [0.7, 0.5, 1.5, 0.8]):
            gp = G16.make_fit_gp(g, "se_beta", 1, d)
            gp.k.k.param_bounds = [(0.1, 10.0), (0.05, 5.0)]
            if host:
                gp.k = _host_twin(g, gp.k)
            gp.update_hyperparameters(np.array(start))
            r, _ = gp.optimize_hyperparameters(method="SLSQP", random_starts=0, num_proc=0)
            lls.append(-float(r.fun))
        res.append(max(lls))
    print("MAP ll device %.12g host %.12g" % tuple(res))
    assert abs(res[0] - res[1]) <= 1e-6 * abs(res[1])
