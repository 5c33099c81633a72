"""MaskedKernel on the host (no GPU): construction, the hyperparameters reaching the base kernel, pickling, the routing decisions
(which models the HIP library evaluates itself and how they are encoded), the reference's steps of the host route on a
Python-defined base, and the fixture's own consistency against the CPU oracle."""
import os
import pickle
import sys

import numpy as np
import pytest

import gptools_amd as g
from gptools_amd import _lib
from gptools_amd.kernel.masked import unit_factor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_g19_masked as G19      # noqa: E402

INF = np.inf
B2 = [(1e-3, 20.0)] * 2


def se1(p=(1.2, 0.6), **kw):
    return g.SquaredExponentialKernel(num_dim=1, initial_params=list(p), param_bounds=B2, **kw)


class PyKernel(g.Kernel):
    """A Python-defined 1-D kernel whose value shows what it was called with."""

    def __init__(self):
        super(PyKernel, self).__init__(num_dim=1, num_params=1, initial_params=[2.0], param_bounds=[(0.0, 10.0)])

    def __call__(self, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False):
        v = self.params[0] * (Xi[:, 0] + 10.0 * Xj[:, 0] + 100.0 * ni[:, 0] + 1000.0 * nj[:, 0])
        return v + (1e6 if symmetric else 0.0) + (1e7 * (hyper_deriv + 1) if hyper_deriv is not None else 0.0)


class OwnCallSE(g.SquaredExponentialKernel):
    def __call__(self, *a, **kw):
        return super(OwnCallSE, self).__call__(*a, **kw)


class OwnCallMasked(g.MaskedKernel):
    def __call__(self, *a, **kw):
        return super(OwnCallMasked, self).__call__(*a, **kw)


# ---- construction ------------------------------------------------------------------------------------------------------------
def test_exported_and_defaults():
    assert g.MaskedKernel is g.kernel.MaskedKernel
    k = g.MaskedKernel(se1())
    assert isinstance(k, g.Kernel)
    assert k.num_dim == 2 and k.mask == [0] and k.maskC == [1]
    assert list(k.scale) == [1.0, 1.0]
    assert k.num_params == 2


def test_constructor_errors():
    with pytest.raises(ValueError, match="Length of mask"):
        g.MaskedKernel(se1(), total_dim=3, mask=[0, 1])
    with pytest.raises(ValueError, match="Length of scale"):
        g.MaskedKernel(se1(), total_dim=2, mask=[0], scale=[1.0])
    with pytest.raises(ValueError):                       # an index range(total_dim) does not hold (the reference's list.remove)
        g.MaskedKernel(se1(), total_dim=2, mask=[2])
    se2 = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=[(1e-3, 20.0)] * 3)
    with pytest.raises(ValueError):                       # ... or holds no more
        g.MaskedKernel(se2, total_dim=3, mask=[1, 1])


def test_mask_complement():
    se2 = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=[(1e-3, 20.0)] * 3)
    k = g.MaskedKernel(se2, total_dim=5, mask=[3, 0])
    assert k.mask == [3, 0] and k.maskC == [1, 2, 4] and k.num_dim == 5


# ---- the hyperparameters are the base's -------------------------------------------------------------------------------------
def test_hyperparameters_reach_the_base():
    base = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.2, 0.6], fixed_params=[False, True],
                                      param_bounds=[(0.1, 5.0), (0.2, 3.0)], enforce_bounds=True)
    base.param_names = np.asarray(["s", "l"])
    k = g.MaskedKernel(base, total_dim=3, mask=[2])
    assert np.array_equal(k.params, [1.2, 0.6]) and k.params is base.params
    assert list(k.param_names) == ["s", "l"] and list(k.fixed_params) == [False, True]
    assert list(k.free_params) == [1.2] and list(k.free_param_names) == ["s"] and k.num_free_params == 1
    assert [tuple(b) for b in k.param_bounds] == [(0.1, 5.0), (0.2, 3.0)] and [tuple(b) for b in k.free_param_bounds] == [(0.1, 5.0)]
    assert k.hyperprior is base.hyperprior and k.enforce_bounds is True
    k.set_hyperparams([9.0])                              # clamped by the base's box
    assert base.params[0] == 5.0
    k.params = [0.7, 0.9]
    assert np.array_equal(base.params, [0.7, 0.9])
    k.fixed_params = [True, False]
    assert list(base.fixed_params) == [True, False] and list(k.free_params) == [0.9]
    k.free_params = [1.5]
    assert base.params[1] == 1.5
    k.param_bounds = [(0.0, 1.0), (0.0, 2.0)]
    assert [tuple(b) for b in base.param_bounds] == [(0.0, 1.0), (0.0, 2.0)]
    k.enforce_bounds = False
    assert base.enforce_bounds is False
    base.params[0] = 0.3
    assert k.params[0] == 0.3
    assert k.hyperprior(k.params) == base.hyperprior(base.params)


def test_in_a_gaussian_process_parameter_vector():
    k = G19.make_kernel(g, "b")
    gp = g.GaussianProcess(k)
    assert len(gp.free_params) == 7
    gp.k.set_hyperparams(np.arange(1.0, 8.0))
    assert np.array_equal(k.k1.base.params, [1, 2, 3, 4, 5]) and np.array_equal(k.k2.base.params, [6, 7])


def test_pickle_round_trip():
    k = g.MaskedKernel(se1(), total_dim=3, mask=[1], scale=[2.0, 0.5])
    k2 = pickle.loads(pickle.dumps(k))
    assert type(k2) is g.MaskedKernel and k2.num_dim == 3 and k2.mask == [1] and k2.maskC == [0, 2]
    assert np.array_equal(k2.scale, [2.0, 0.5]) and np.array_equal(k2.params, k.params)
    assert k2._native_factor() is None                    # (a given scale stays the host route)
    k3 = pickle.loads(pickle.dumps(G19.make_kernel(g, "a")))
    assert k3._native_factors() is not None
    k3.k1.params[0] = 4.0
    assert k3.k1.base.params[0] == 4.0


def test_num_dim_rules_in_sums_and_products():
    m = g.MaskedKernel(se1(), total_dim=2, mask=[0])
    se2 = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=[(1e-3, 20.0)] * 3)
    assert (m + se2).num_dim == 2 and (m * se2).num_dim == 2 and (se2 * m).num_params == 5
    with pytest.raises(ValueError):
        m + se1()
    with pytest.raises(ValueError):
        m * g.MaskedKernel(se1(), total_dim=3, mask=[0])


# ---- routing -----------------------------------------------------------------------------------------------------------------
def _terms(k):
    return g.GaussianProcess(k)._native_terms()


def _same(t, u):
    assert len(t) == len(u)
    for a, b in zip(t, u):
        if isinstance(b, (int, np.integer)):
            assert a == b
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b, dtype=float))


def test_on_dim_ids():
    assert _lib.kernel_on_dim(_lib.KERNEL_GIBBS_TANH, 0) == 7 + 256 and _lib.kernel_on_dim(_lib.KERNEL_GIBBS_BSPLINE, 2) == 12 + 768
    assert _lib.GIBBS_ON_DIM_MAX_D == 3
    kid, p = unit_factor(3)
    assert kid == _lib.KERNEL_SE and np.array_equal(p, [1.0, INF, INF, INF])


def test_routing_of_the_fixture_models():
    TANH0, CUBIC1 = _lib.kernel_on_dim(_lib.KERNEL_GIBBS_TANH, 0), _lib.kernel_on_dim(_lib.KERNEL_GIBBS_CUBIC, 1)
    t = _terms(G19.make_kernel(g, "a"))
    assert len(t) == 1
    _same(t[0], (_lib.KERNEL_SE, [1.2, 0.6, INF], _lib.KERNEL_M52, [1.0, INF, 0.9]))
    _same(G19.make_kernel(g, "a")._native_factors(), t[0])
    t = _terms(G19.make_kernel(g, "b"))
    assert len(t) == 1
    _same(t[0], (TANH0, G19.TANH_P, _lib.KERNEL_SE, [1.0, INF, 0.8]))
    t = _terms(G19.make_kernel(g, "c"))
    assert len(t) == 2
    _same(t[0], (_lib.KERNEL_SE, [1.0, 0.7, INF, 0.9]))
    _same(t[1], (_lib.KERNEL_RQ, [0.6, 1.5, INF, 0.8, INF]))
    t = _terms(G19.make_kernel(g, "d"))
    assert len(t) == 1
    _same(t[0], (CUBIC1, G19.CUBIC_P, _lib.KERNEL_SE, [1.0, 0.8, INF, 1.1]))
    ke = G19.make_kernel(g, "e")
    assert _terms(ke) is None and ke._native_factors() is None and not g.GaussianProcess(ke)._fast_fit_possible()


def test_routing_mask_order_and_lone_gibbs():
    se2 = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.3, 0.4], param_bounds=[(1e-3, 20.0)] * 3)
    _same(g.MaskedKernel(se2, total_dim=4, mask=[3, 1])._native_factor(), (_lib.KERNEL_SE, [1.0, INF, 0.4, INF, 0.3]))
    mat = G19.masked(g, "matern", [1.0, 1.5, 0.8], 2, [1])
    _same(mat._native_factor(), (_lib.KERNEL_MATERN, [1.0, 1.5, INF, 0.8]))
    lone = G19.masked(g, "tanh", G19.TANH_P, 3, [2])
    t = _terms(lone)
    _same(t[0], (_lib.kernel_on_dim(_lib.KERNEL_GIBBS_TANH, 2), G19.TANH_P, _lib.KERNEL_SE, [1.0, INF, INF, INF]))
    # a sum of up to 8 terms, masked ones among them; the ninth sends the model to the host
    k = lone
    for _ in range(7):
        k = k + G19.masked(g, "se", [1.0, 0.5], 3, [0])
    assert len(_terms(k)) == 8
    assert _terms(k + G19.masked(g, "se", [1.0, 0.5], 3, [0])) is None
    # under linear warp layers the masked model peels off like any native one
    gp = g.GaussianProcess(g.LinearWarpedKernel(G19.make_kernel(g, "a"), [0.0, 0.0], [2.0, 2.0]))
    terms, layers = gp._device_model()
    assert len(terms) == 1 and len(terms[0]) == 4 and len(layers) == 1


def test_host_route_cases():
    se = se1
    host = [
        g.MaskedKernel(se(), total_dim=2, mask=[0], scale=[1.0, 1.0]),                   # a scale, even of ones
        g.MaskedKernel(se() + se(), total_dim=2, mask=[0]),                               # base: a sum
        g.MaskedKernel(se() * se(), total_dim=2, mask=[0]),                               # ... a product
        g.MaskedKernel(g.LinearWarpedKernel(se(), [0.0], [2.0]), total_dim=2, mask=[0]),  # ... a warped kernel
        g.MaskedKernel(PyKernel(), total_dim=2, mask=[0]),                                # ... a Python-defined kernel
        g.MaskedKernel(OwnCallSE(num_dim=1, initial_params=[1.0, 1.0], param_bounds=B2), total_dim=2, mask=[0]),
        g.MaskedKernel(g.MaskedKernel(g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 1.0], param_bounds=B2),
                                      total_dim=2, mask=[1]), total_dim=3, mask=[0, 2]),  # nested masks
        G19.masked(g, "tanh", G19.TANH_P, 4, [1]),                                        # Gibbs beyond 3 dimensions
        OwnCallMasked(se(), total_dim=2, mask=[0]),                                       # a subclass with its own __call__
    ]
    for k in host:
        assert k._native_factor() is None and k._native_term() is None, type(k.base).__name__
        assert _terms(k) is None
        other = g.MaskedKernel(se(), total_dim=k.num_dim, mask=[0])
        assert (k * other)._native_factors() is None and _terms(k + other) is None
    # a forwarded attribute never makes a kernel native
    assert g.MaskedKernel._gpt_kernel_id is None


def test_hyper_deriv_and_partitioned_decisions():
    gp = g.GaussianProcess(G19.make_kernel(g, "c"))
    assert gp._has_masked() and not g.GaussianProcess(se1())._has_masked()
    assert g.GaussianProcess(g.LinearWarpedKernel(G19.make_kernel(g, "a"), [0.0, 0.0], [2.0, 2.0]))._has_masked()
    gp1 = g.GaussianProcess(G19.masked(g, "se", [1.0, 0.5], 2, [0]))
    gp1.partitioned = True
    d = G19.model_data("a")
    gp1.add_data(d["X"], d["y"], err_y=0.05)
    assert not gp1._partitioned_possible()
    k = G19.masked(g, "se", [0.9, 0.7, 1.1], 3, [0, 2])
    assert [k._device_hyper_deriv(h) for h in range(3)] == [0, 1, 3]
    rq = G19.masked(g, "rq", [1.1, 0.6, 0.9, 0.5], 3, [2, 1])
    assert [rq._device_hyper_deriv(h) for h in range(4)] == [0, 1, 4, 3]


# ---- the host route's steps --------------------------------------------------------------------------------------------------
def test_host_call_on_a_python_base():
    k = g.MaskedKernel(PyKernel(), total_dim=3, mask=[1], scale=[2.0, 3.0])
    Xi = np.array([[9.0, 1.0, 9.0], [9.0, 2.0, 9.0], [9.0, 3.0, 9.0], [9.0, 4.0, 9.0]])
    Xj = np.array([[8.0, 0.5, 8.0], [8.0, 0.25, 8.0], [8.0, 0.125, 8.0], [8.0, 1.0, 8.0]])
    ni = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 2, 0]])
    nj = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 1]])
    v = k(Xi, Xj, ni, nj)
    # base sees Xi * 2 and Xj * 3 and the masked column's orders; scale ** order multiplies in; an outside order: exactly 0
    assert v[0] == 2.0 * (2.0 + 10.0 * 1.5)
    assert v[1] == 2.0 * (4.0 + 10.0 * 0.75 + 100.0 + 1000.0) * 2.0 * 3.0
    assert v[2] == 0.0 and v[3] == 0.0
    assert k(Xi[:1], Xj[:1], ni[:1], nj[:1], symmetric=True)[0] == v[0] + 1e6
    assert k(Xi[:1], Xj[:1], ni[:1], nj[:1], hyper_deriv=0)[0] == v[0] + 1e7


# ---- the fixture against the CPU oracle --------------------------------------------------------------------------------------
def test_fixture_value_corners_against_the_oracle(golden, oracle):
    """The stored corners' value-only block (the first 20 of the corner's 60 training rows carry no derivative) as elementwise
    products / sums of the oracle's matrices on the sliced columns: guards the generator."""
    G = golden("g19_masked")
    O = oracle
    nv = G19.CORNER - G19.N_DERIV
    lo = G19.N_TRAIN - G19.CORNER

    def block(kind, p, cols, scale=1.0):
        Xc = X[:, cols] * scale
        return O.kbuild(kind, p, Xc, np.zeros(Xc.shape, dtype=int))
    for m in ("a", "c", "e"):
        X = G["model_%s__X" % m][lo:lo + nv]
        assert not G["model_%s__n" % m][lo:lo + nv].any()
        if m == "a":
            K = block("se", [1.2, 0.6], [0]) * block("m52", [1.0, 0.9], [1])
        elif m == "e":
            K = block("se", [1.2, 0.6], [0], 2.0) * block("m52", [1.0, 0.9], [1])
        else:
            K = block("se", [1.0, 0.7, 0.9], [0, 2]) + block("rq", [0.6, 1.5, 0.8], [1])
        np.testing.assert_allclose(G["model_%s__K" % m][:nv, :nv], K, rtol=1e-12, atol=1e-14, err_msg=m)
    # every stored pair with an order outside the mask is exactly zero, and nothing stored is non-finite
    for case, (kind, p, D, mask, scale) in G19.PAIR_CASES.items():
        ni, nj, kv = G["pairs_%s__ni" % case], G["pairs_%s__nj" % case], G["pairs_%s__k" % case]
        outC = [d for d in range(D) if d not in mask]
        outside = (ni[:, outC] != 0).any(axis=1) | (nj[:, outC] != 0).any(axis=1)
        assert outside.sum() >= 60 and np.all(kv[outside] == 0.0) and np.isfinite(kv).all(), case
        assert (~outside & (kv != 0.0)).sum() >= 60, case
