"""PeriodicKernel on the host, no GPU: the kernel's per-dimension chain (gptools_amd/csrc/periodic.hpp) compiled for the CPU against
the mpmath fixture tests/golden/g21_periodic.npz (gen_g21_periodic.py), its exact periodicity, the class surface, the masked
encoding, and what GaussianProcess._device_model() makes of models that hold the kernel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gptools_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gptools_amd", "csrc")

#: Largest deviation of the test aid from the fixture, as a fraction of the entry's scale (sigma_f^2 times the product over the
#: dimensions of the largest magnitude the derivative of that order takes over one period): measured 1.22e-14, at combined order 14
#: with |tau| near four periods (1.3e-15 at order 0; the D = 16 set 1.3e-16).  Asserted with a factor 4; the GPU suite allows the
#: device ten times this constant.  Beyond 1e-13 the arithmetic would be wrong.
HOST_DEV = 1.22e-14


def load_aid():
    subprocess.run(["make", "-C", CSRC, "periodic_host"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(CSRC, "build", "libperiodic_host.so"))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    L.gpt_host_periodic_pairs.restype = ctypes.c_int
    L.gpt_host_periodic_pairs.argtypes = [ctypes.c_int, dp, dp, dp, ip, ip, ctypes.c_int64, dp]

    def pairs(params, Xi, Xj, ni, nj):
        """The kernel [sigma_f, l .., p ..] at the M pairs (rows of Xi, Xj with orders ni, nj), by the host build of periodic.hpp."""
        Xi, Xj = np.ascontiguousarray(np.atleast_2d(Xi), dtype=float), np.ascontiguousarray(np.atleast_2d(Xj), dtype=float)
        ni, nj = np.ascontiguousarray(np.atleast_2d(ni), dtype=np.int32), np.ascontiguousarray(np.atleast_2d(nj), dtype=np.int32)
        params = np.ascontiguousarray(params, dtype=float)
        M, D = Xi.shape
        assert Xj.shape == (M, D) and ni.shape == (M, D) and nj.shape == (M, D) and len(params) == 2 * D + 1
        out = np.empty(M)
        rc = L.gpt_host_periodic_pairs(D, params.ctypes.data_as(dp), Xi.ctypes.data_as(dp), Xj.ctypes.data_as(dp),
                                       ni.ctypes.data_as(ip), nj.ctypes.data_as(ip), M, out.ctypes.data_as(dp))
        assert rc == 0
        return out
    return pairs


_SCALES = {}


def order_scale(l, p, n):
    """The fixture's yardstick for one dimension: the largest magnitude the n-th derivative of exp(-2 sin^2(pi tau / p) / l^2)
    takes over a period (1 for n = 0 or l = inf), on the generator's grid of 4096 points."""
    if n == 0 or np.isinf(l):
        return 1.0
    key = (float(l), float(p), int(n))
    if key not in _SCALES:
        from math import comb
        a, w = 1.0 / (l * l), 2.0 * np.pi / p
        th = np.linspace(0.0, 2.0 * np.pi, 4096, endpoint=False)
        G = [None] + [a * w ** k * np.cos(th + 0.5 * np.pi * k) for k in range(1, n + 1)]
        P = [np.ones_like(th)]
        for m in range(n):
            P.append(sum(comb(m, k) * G[k + 1] * P[m - k] for k in range(m + 1)))
        _SCALES[key] = float(np.abs(np.exp(a * (np.cos(th) - 1.0)) * P[n]).max())
    return _SCALES[key]


def pair_scales(params, ni, nj):
    """sigma_f^2 times the product of order_scale over the dimensions, for every row of combined orders ni + nj."""
    params = np.asarray(params, dtype=float)
    n = np.atleast_2d(ni) + np.atleast_2d(nj)
    D = n.shape[1]
    out = np.full(len(n), params[0] ** 2)
    for d in range(D):
        for v in np.unique(n[:, d]):
            out[n[:, d] == v] *= order_scale(params[1 + d], params[1 + D + d], int(v))
    return out


@pytest.fixture(scope="module")
def aid():
    return load_aid()


@pytest.fixture(scope="module")
def g():
    import gptools_amd
    return gptools_amd


def fixture_cases(G):
    for c in range(int(G["ncases"])):
        yield c, int(G["c%d_D" % c]), {k: G["c%d_%s" % (c, k)] for k in ("params", "Xi", "Xj", "ni", "nj", "k", "scale")}


# ---- the chain against mpmath ---------------------------------------------------------------------------------------------------
def test_aid_against_the_mpmath_fixture(aid, golden):
    G = golden("g21_periodic")
    seen, worst = set(), 0.0
    for c, D, f in fixture_cases(G):
        got = aid(f["params"], f["Xi"], f["Xj"], f["ni"], f["nj"])
        dev = np.abs(got - f["k"]) / f["scale"]
        print("case %d, D = %d, %d pairs: worst scaled deviation %.3g" % (c, D, len(got), dev.max()))
        worst = max(worst, dev.max())
        seen.add(D)
        assert (f["ni"] + f["nj"]).max() <= 16
        # a dimension with l = inf: exactly 1.0 without an order, exactly 0.0 with one
        masked = np.isinf(f["params"][1:1 + D])
        if masked.any():
            hit = ((f["ni"] + f["nj"])[:, masked] > 0).any(axis=1)
            assert hit.any() and (~hit).any()
            assert np.all(got[hit] == 0.0) and np.all(f["k"][hit] == 0.0)
    assert seen == {1, 2, 3, 16}
    assert HOST_DEV < 1e-13 / 4
    assert worst <= 4 * HOST_DEV, worst


def test_fixture_holds_what_it_should(golden):
    G = golden("g21_periodic")
    orders, zero_tau, whole, far, both = set(), 0, 0, 0, 0
    for c, D, f in fixture_cases(G):
        n = f["ni"] + f["nj"]
        orders |= set(int(v) for v in n.ravel())
        tau = f["Xi"] - f["Xj"]
        t = tau / f["params"][1 + D:]
        zero_tau += int((tau == 0).all(axis=1).sum())
        whole += int(((t == np.rint(t)) & (tau != 0)).all(axis=1).sum())
        far += int((np.abs(t) > 2).any(axis=1).sum())
        both += int(((f["ni"] > 0) & (f["nj"] > 0)).any(axis=1).sum())
        assert np.all(f["scale"] > 0) and np.all(np.abs(f["k"]) <= f["scale"] * (1 + 1e-9))
        # the yardstick the GPU suite forms for its own pairs is the fixture's
        np.testing.assert_allclose(pair_scales(f["params"], f["ni"], f["nj"]), f["scale"], rtol=1e-12)
    assert orders == set(range(17)) and zero_tau >= 8 and whole >= 16 and far >= 50 and both >= 50
    assert os.path.getsize(os.path.join(HERE, "golden", "g21_periodic.npz")) < 100 * 1024


# ---- periodic to the bit -----------------------------------------------------------------------------------------------------
def test_exact_periodicity_with_a_power_of_two_period(aid):
    """p a power of two: tau / p is exact, so tau and tau + 5 p reduce to the same t and give the same bits, at every order.
    (tau on a grid of 2^-20, so that tau + 5 p is exact too.)"""
    rs = np.random.RandomState(5)
    for D, ps in ((1, [0.5]), (2, [2.0, 0.25]), (3, [4.0, 0.125, 1.0])):
        params = np.concatenate(([1.3], rs.uniform(0.3, 2.0, D), ps))
        M = 400
        Xj = np.round(rs.uniform(-1, 1, (M, D)) * 2 ** 20) / 2 ** 20
        Xi = Xj + np.round(rs.uniform(-3, 3, (M, D)) * 2 ** 20) / 2 ** 20
        ni, nj = rs.randint(0, 9, (M, D)), rs.randint(0, 9, (M, D))
        ni[:50], nj[:50] = 0, 0
        a = aid(params, Xi, Xj, ni, nj)
        b = aid(params, Xi + 5 * np.asarray(ps), Xj, ni, nj)
        c = aid(params, Xi, Xj + 5 * np.asarray(ps), ni, nj)
        assert np.array_equal(a, b) and np.array_equal(a, c)
        assert np.all(np.isfinite(a)) and np.ptp(a) > 0


# ---- the class -------------------------------------------------------------------------------------------------------------
def test_class_surface(g):
    k = g.PeriodicKernel(num_dim=3, initial_params=[1.1, 0.5, 0.6, 0.7, 2.0, 3.0, 4.0], param_bounds=[(0.0, 10.0)] * 7)
    assert g.PeriodicKernel is g.kernel.PeriodicKernel and type(k)._gpt_kernel_id == _lib.KERNEL_PERIODIC == 14
    assert k.num_dim == 3 and k.num_params == 7
    assert list(k.param_names) == [r"\sigma_f", "l_1", "l_2", "l_3", "p_1", "p_2", "p_3"]
    assert list(k.param_bounds[:]) == [(0.0, 10.0)] * 7
    np.testing.assert_array_equal(k._native_params(), [1.1, 0.5, 0.6, 0.7, 2.0, 3.0, 4.0])
    assert k._native_params().dtype == float
    k1 = g.PeriodicKernel(initial_params=[1.0, 0.5, 2.0], param_bounds=[(0.0, 10.0)] * 3)
    assert k1.num_dim == 1 and list(k1.param_names) == [r"\sigma_f", "l_1", "p_1"]
    # the refusal of the RationalQuadratic / Matern kernels, before any context is touched
    z = np.zeros((1, 1))
    with pytest.raises(NotImplementedError, match="Hyperparameter derivatives have not been implemented!"):
        k1(z, z, z.astype(int), z.astype(int), hyper_deriv=1)
    assert type(k1).__call__ is g.Kernel.__call__


def test_masked_encoding(g):
    base = g.PeriodicKernel(num_dim=2, initial_params=[1.2, 0.5, 0.6, 2.0, 3.0], param_bounds=[(0.0, 10.0)] * 5)
    mk = g.MaskedKernel(base, total_dim=4, mask=[3, 1])
    kid, p = mk._native_term()
    assert kid == _lib.KERNEL_PERIODIC
    np.testing.assert_array_equal(p, [1.2, np.inf, 0.6, np.inf, 0.5, 1.0, 3.0, 1.0, 2.0])
    assert mk._native_factor()[0] == kid
    z = np.zeros((1, 4))
    with pytest.raises(NotImplementedError):
        mk(z, z, z.astype(int), z.astype(int), hyper_deriv=0)


def test_header_and_binding_carry_the_constant():
    with open(os.path.join(HERE, "..", "include", "gpt_hip.h")) as fh:
        text = fh.read()
    assert "#define GPT_KERNEL_PERIODIC 14" in text and "#define GPT_PERIODIC_MAXORD 16" in text
    assert _lib.KERNEL_PERIODIC == 14 and _lib.PERIODIC_MAXORD == 16


# ---- device-model resolution ---------------------------------------------------------------------------------------------------
class _Recorder(object):
    """Stands in for ``_lib.Context``: records the fits it is asked for."""

    def __init__(self, log):
        self.log, self._warp_key = log, None

    def set_data(self, X, n):
        self._warp_key = None

    def set_warp(self, layers):
        self._warp_key = tuple((int(t), tuple(float(v) for v in p)) for t, p in (layers or [])) or None
        self.log.append(("set_warp", self._warp_key))

    def set_option(self, key, value):
        pass

    def _fit(self, terms):
        self.log.append(("fit", tuple(tuple(int(e) if i % 2 == 0 else tuple(float(v) for v in e) for i, e in enumerate(t)) for t in terms)))
        return 1.0, 0.0

    def fit(self, kernel_id, params, noise_var, y, err_y, diag_add):
        return self._fit([(kernel_id, params)])

    def fit_sum(self, kernel_ids, params_list, noise_var, y, err_y, diag_add):
        return self._fit(list(zip(kernel_ids, params_list)))

    def fit_terms(self, terms, noise_var, y, err_y, diag_add):
        return self._fit(terms)

    def fit_matrix(self, K_tot, y):
        self.log.append(("fit_matrix",))
        return 1.0, 0.0


def _models(g):
    B = [(0.0, 10.0)]
    per = lambda: g.PeriodicKernel(num_dim=1, initial_params=[1.1, 0.7, 2.0], param_bounds=B * 3)
    se = lambda: g.SquaredExponentialKernel(num_dim=1, initial_params=[0.9, 1.5], param_bounds=B * 2)
    P, S = (_lib.KERNEL_PERIODIC, (1.1, 0.7, 2.0)), (_lib.KERNEL_SE, (0.9, 1.5))
    warped = g.LinearWarpedKernel(per(), [-1.0], [3.0])
    return {"periodic": (per(), (P,), None), "se + periodic": (se() + per(), (S, P), None),
            "se * periodic": (se() * per(), (S + P,), None), "periodic * periodic": (per() * per(), (P + P,), None),
            "linear-warped periodic": (warped, (P,), ((_lib.WARP_LINEAR, (-1.0, 3.0)),))}


@pytest.mark.parametrize("name", ["periodic", "se + periodic", "se * periodic", "periodic * periodic", "linear-warped periodic"])
def test_device_model_resolves_to_native_terms(g, monkeypatch, name):
    k, terms, layers = _models(g)[name]
    X = np.linspace(0.0, 1.0, 12)
    gp = g.GaussianProcess(k, X=X, y=np.sin(X), err_y=0.1)
    model = gp._device_model()
    assert model is not None
    got = tuple(tuple(int(e) if i % 2 == 0 else tuple(float(v) for v in e) for i, e in enumerate(t)) for t in model[0])
    assert got == terms
    assert tuple((int(t), tuple(float(v) for v in p)) for t, p in model[1]) == (layers or ())
    log = []
    monkeypatch.setattr(_lib, "Context", lambda device=0: _Recorder(log))
    gp.compute_K_L_alpha_ll()
    assert gp._fit_mode == "kernel"
    assert [e for e in log if e[0] == "fit"] == [("fit", terms)] and ("fit_matrix",) not in log
    if layers:
        assert ("set_warp", layers) in log


def test_periodic_times_gibbs_stays_on_the_host_route(g):
    B = [(0.0, 10.0)]
    per = g.PeriodicKernel(num_dim=1, initial_params=[1.1, 0.7, 2.0], param_bounds=B * 3)
    gib = g.GibbsKernel1dTanh(initial_params=[1.0, 0.5, 1.0, 0.3, 0.5], param_bounds=B * 5)
    X = np.linspace(0.0, 1.0, 12)
    for k in (per * gib, gib * per):
        assert k._native_factors() is None
        assert g.GaussianProcess(k, X=X, y=np.sin(X), err_y=0.1)._device_model() is None
    # ... and beside a Gibbs TERM the model is native
    assert g.GaussianProcess(per + gib, X=X, y=np.sin(X), err_y=0.1)._device_model() is not None
