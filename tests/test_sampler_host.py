"""CPU suite: the ensemble sampler (gptools_amd/sampler.py), the library's stepping loop compiled for the host
(csrc/ensemble.hpp through test_aids/ensemble_host.cpp), summarize_sampler, and what sample_hyperparameter_posterior decides
without a device (arguments, the library route's eligibility, the no-GPU failure)."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MU = np.array([2.0, -0.3])
SIGMA = np.array([[1.0, 0.045], [0.045, 0.0025]])
SIGMA_INV = np.linalg.inv(SIGMA)
STD = np.sqrt(np.diag(SIGMA))


def gauss(P):
    d = np.atleast_2d(P) - MU
    return -0.5 * np.einsum("ki,ij,kj->k", d, SIGMA_INV, d)


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


# ---- 1. a Gaussian target -------------------------------------------------------------------------------------------------------
# Bounds from a numpy restatement of the sampler over seeds 0 to 19: worst |mean - mu| / sigma 0.072, worst |std / sigma - 1|
# 0.030, acceptance 0.70 to 0.72; asserted at about three times the worst case.
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gaussian_target_moments(g, seed):
    rs = np.random.RandomState(seed)
    s = g.EnsembleSampler(64, 2, gauss, random_state=rs)
    pos0 = MU + rs.randn(64, 2) * (3.0, 0.2)
    s.run_mcmc(pos0, 600)
    flat = s.chain[:, 200:, :].reshape(-1, 2)
    dev_mean = np.abs(flat.mean(0) - MU) / STD
    dev_std = np.abs(flat.std(0) / STD - 1.0)
    acc = s.acceptance_fraction.mean()
    print("seed %d: |mean - mu| / sigma %s, |std / sigma - 1| %s, acceptance %.3f" % (seed, dev_mean, dev_std, acc))
    assert (dev_mean <= 0.2).all() and (dev_std <= 0.1).all()
    assert 0.5 < acc < 0.9
    assert s.route == "host"


# ---- 2. continuation ------------------------------------------------------------------------------------------------------------
def test_runs_continue_the_chain(g):
    pos0 = MU + np.random.RandomState(5).randn(16, 2) * (1.0, 0.1)
    one = g.EnsembleSampler(16, 2, gauss, random_state=7)
    one.run_mcmc(pos0, 40)
    two = g.EnsembleSampler(16, 2, gauss, random_state=7)
    pos, lnp = two.run_mcmc(pos0, 15)
    np.testing.assert_array_equal(pos, two.chain[:, -1, :])
    two.run_mcmc(pos, 25, lnprob0=lnp)
    np.testing.assert_array_equal(one.chain, two.chain)
    np.testing.assert_array_equal(one.lnprobability, two.lnprobability)
    np.testing.assert_array_equal(one.acceptance_fraction, two.acceptance_fraction)
    three = g.EnsembleSampler(16, 2, gauss, random_state=7)          # ... and without the stored log-probabilities
    three.run_mcmc(three.run_mcmc(pos0, 15)[0], 25)
    np.testing.assert_array_equal(one.chain, three.chain)


# ---- 3. arguments and edges -----------------------------------------------------------------------------------------------------
def test_shapes_attributes_and_reset(g):
    s = g.EnsembleSampler(8, 2, gauss, a=2.5, random_state=np.random.RandomState(3))
    assert s.chain.shape == (8, 0, 2) and s.chain.size == 0 and s.lnprobability.shape == (8, 0)
    assert s.flatchain.shape == (0, 2) and s.acceptance_fraction.shape == (8,)
    assert (s.a, s.dim, s.k) == (2.5, 2, 8) and isinstance(s.random_state, np.random.RandomState)
    pos0 = MU + np.random.RandomState(1).randn(8, 2) * 0.05
    pos, lnp = s.run_mcmc(pos0, 7)
    assert s.chain.shape == (8, 7, 2) and s.lnprobability.shape == (8, 7)
    assert s.flatchain.shape == (56, 2) and s.flatlnprobability.shape == (56,)
    np.testing.assert_array_equal(pos, s.chain[:, -1, :])
    np.testing.assert_array_equal(lnp, s.lnprobability[:, -1])
    np.testing.assert_array_equal(s.lnprobability, gauss(s.flatchain).reshape(8, 7))
    assert ((s.acceptance_fraction >= 0) & (s.acceptance_fraction <= 1)).all()
    s.run_mcmc(pos, 0)
    assert s.chain.shape == (8, 7, 2)
    s.reset()
    assert s.chain.size == 0 and s.chain.shape == (8, 0, 2) and (s.acceptance_fraction == 0).all()
    assert isinstance(g.EnsembleSampler(8, 2, gauss).random_state, np.random.RandomState)


def test_bad_ensembles_and_initial_nan_raise(g):
    with pytest.raises(ValueError):
        g.EnsembleSampler(7, 2, gauss)
    with pytest.raises(ValueError):
        g.EnsembleSampler(4, 3, gauss)
    s = g.EnsembleSampler(8, 2, lambda P: np.where(P[:, 0] > 0, gauss(P), np.nan), random_state=0)
    pos0 = MU + np.random.RandomState(1).randn(8, 2) * 0.05
    pos0[3, 0] = -1.0
    with pytest.raises(ValueError, match="NaN"):
        s.run_mcmc(pos0, 3)
    with pytest.raises(ValueError):
        s.run_mcmc(pos0[:6], 3)


@pytest.mark.parametrize("bad", [np.nan, -np.inf])
def test_excluded_half_plane_is_never_entered(g, bad):
    # the target is `bad` left of x = 1.8, which cuts through the bulk of the Gaussian; one walker starts there (at -inf)
    calls = []

    def f(P):
        calls.append(len(P))
        return np.where(P[:, 0] >= 1.8, gauss(P), bad)
    s = g.EnsembleSampler(16, 2, f, random_state=4)
    pos0 = MU + np.abs(np.random.RandomState(2).randn(16, 2)) * (0.5, 0.02)
    lnp0 = gauss(pos0)
    pos0[5, 0], lnp0[5] = 1.0, -np.inf
    s.run_mcmc(pos0, 60, lnprob0=lnp0)
    moved = np.ones(16, dtype=bool)
    moved[5] = False
    assert (s.chain[moved][:, :, 0] >= 1.8).all() and np.isfinite(s.lnprobability[moved]).all()
    assert not np.isnan(s.lnprobability).any()
    assert set(calls) == {8}                                     # half an ensemble per call, nothing else
    # the walker outside leaves as soon as a proposal of its lands inside, and stays at its start until then
    inside = s.chain[5, :, 0] >= 1.8
    first = np.argmax(inside) if inside.any() else 60
    assert (s.chain[5, :first, 0] == 1.0).all() and inside[first:].all()


# ---- 4. the library's loop, compiled for the host --------------------------------------------------------------------------------
LNPROB_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope="module")
def ensemble_host():
    here = os.path.join(ROOT, "gptools_amd", "csrc")
    subprocess.run(["make", "-C", here, "ensemble_host"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(here, "build", "libensemble_host.so"))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    L.gpt_host_ensemble_run.restype = ctypes.c_int
    L.gpt_host_ensemble_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp, dp, dp, ip, dp, dp, dp, dp, dp, ip,
                                        LNPROB_FN]
    return L


def _library_loop(L, fn, lo, hi, a, variates, pos0, lnp0):
    us, pj, ua = variates
    nsteps, K = us.shape
    p = pos0.shape[1]
    pos, lnp = np.array(pos0, dtype=float), np.array(lnp0, dtype=float)
    chain, lc, nacc = np.empty((nsteps, K, p)), np.empty((nsteps, K)), np.zeros(K, dtype=np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    d = lambda x: x.ctypes.data_as(dp)      # noqa: E731
    rc = L.gpt_host_ensemble_run(K, p, nsteps, a, d(lo), d(hi), d(us), pj.ctypes.data_as(ip), d(ua), d(pos), d(lnp), d(chain), d(lc),
                                 nacc.ctypes.data_as(ip), fn)
    return rc, chain, lc, nacc, pos, lnp


def test_library_loop_matches_python_loop(g, ensemble_host):
    from gptools_amd import sampler as S
    lo, hi = np.array([1.6, -0.36]), np.array([3.5, -0.2])          # cuts through the bulk on three sides
    K, nsteps, a = 16, 50, 2.0
    counts = {"outside": 0, "evaluated": 0}

    def boxed(P):                                                # the Python loop's target: the box prior, then the Gaussian
        P = np.atleast_2d(P)
        inside = ((lo <= P) & (P <= hi)).all(1)
        counts["outside"] += int((~inside).sum())
        out = np.full(len(P), -np.inf)
        if inside.any():
            out[inside] = gauss(P[inside])
        return out

    @LNPROB_FN
    def callback(count, q, out):                                 # the library loop's evaluator: in-box proposals only
        P = np.ctypeslib.as_array(q, shape=(count, 2))
        assert ((lo <= P) & (P <= hi)).all()
        counts["evaluated"] += count
        np.ctypeslib.as_array(out, shape=(count,))[:] = gauss(P)
        return 0

    rs = np.random.RandomState(11)
    pos0 = np.column_stack((rs.uniform(lo[0], hi[0], K), rs.uniform(lo[1], hi[1], K)))
    lnp0 = boxed(pos0)
    variates = S.draw_variates(np.random.RandomState(12), K, nsteps)
    assert variates[1].dtype == np.int32 and all(v.shape == (nsteps, K) for v in variates)
    counts["outside"] = 0
    chain_py, lc_py, nacc_py = S.host_steps(boxed, pos0, lnp0, a, *variates)
    rc, chain_c, lc_c, nacc_c, pos_c, lnp_c = _library_loop(ensemble_host, callback, lo, hi, a, variates, pos0, lnp0)
    assert rc == 0
    assert counts["outside"] > 20 and counts["evaluated"] == nsteps * K - counts["outside"]      # the case occurred
    np.testing.assert_array_equal(chain_c, chain_py)
    np.testing.assert_array_equal(lc_c, lc_py)
    np.testing.assert_array_equal(nacc_c, nacc_py)
    np.testing.assert_array_equal(pos_c, chain_py[-1])
    np.testing.assert_array_equal(lnp_c, lc_py[-1])
    assert 0 < nacc_py.sum() < nsteps * K
    # the sampler's own run draws the same variates from the same state
    s = g.EnsembleSampler(K, 2, boxed, a=a, random_state=np.random.RandomState(12))
    s.run_mcmc(pos0, nsteps, lnprob0=lnp0)
    np.testing.assert_array_equal(s.chain, np.transpose(chain_c, (1, 0, 2)))
    np.testing.assert_array_equal(s.lnprobability, lc_c.T)


def test_library_loop_refuses_bad_arguments_and_passes_errors_on(ensemble_host):
    from gptools_amd import sampler as S
    lo, hi = np.array([-10.0, -10.0]), np.array([10.0, 10.0])
    pos0 = MU + np.random.RandomState(1).randn(8, 2) * 0.05
    variates = S.draw_variates(np.random.RandomState(2), 8, 4)
    ok = LNPROB_FN(lambda count, q, out: 0)
    bad_partner = (variates[0], variates[1].copy(), variates[2])
    bad_partner[1][2, 3] = 4                                      # outside the half of 4
    assert _library_loop(ensemble_host, ok, lo, hi, 2.0, bad_partner, pos0, gauss(pos0))[0] == -1
    assert _library_loop(ensemble_host, ok, lo, hi, 1.0, variates, pos0, gauss(pos0))[0] == -1
    failing = LNPROB_FN(lambda count, q, out: -5)
    assert _library_loop(ensemble_host, failing, lo, hi, 2.0, variates, pos0, gauss(pos0))[0] == -5


# ---- 5. summarize_sampler -------------------------------------------------------------------------------------------------------
def _weighted_percentile(x, w, p):
    """The stated rule, directly: p_n = 100 / S_N (S_n - w_n / 2) of the sorted samples, linear in between."""
    order = np.argsort(x)
    x, w = x[order], w[order]
    pn = [100.0 / w.sum() * (w[:n + 1].sum() - w[n] / 2.0) for n in range(len(x))]
    for n in range(len(x) - 1):
        if pn[n] <= p <= pn[n + 1]:
            return x[n] + (p - pn[n]) / (pn[n + 1] - pn[n]) * (x[n + 1] - x[n])
    raise AssertionError("p outside the samples' percentiles")


def test_summarize_sampler(g):
    rs = np.random.RandomState(0)
    chain = rs.randn(6, 40, 3) * (1.0, 2.0, 0.5) + (0.0, 1.0, -2.0)

    class Sampler(object):
        pass
    s = Sampler()
    s.chain = chain
    mask = np.array([True, False, True, True, False, True])
    mean, lo, hi = g.summarize_sampler(s, burn=10, chain_mask=mask, ci=0.9)
    flat = chain[mask, 10:, :].reshape(-1, 3)
    np.testing.assert_array_equal(mean, np.mean(flat, axis=0))
    edge = 100.0 * (1.0 - 0.9) / 2.0                              # (the contract's expression: not exactly 5)
    np.testing.assert_array_equal(lo, np.percentile(flat, edge, axis=0))
    np.testing.assert_array_equal(hi, np.percentile(flat, 100.0 - edge, axis=0))
    mean3, lo3, hi3 = g.summarize_sampler(chain)                  # an array, all walkers, 95 %
    np.testing.assert_array_equal(mean3, chain.reshape(-1, 3).mean(0))
    np.testing.assert_allclose(lo3, np.percentile(chain.reshape(-1, 3), 2.5, axis=0), rtol=1e-15)
    two = chain[0]
    mean2, lo2, hi2 = g.summarize_sampler(two, burn=5)
    np.testing.assert_array_equal(mean2, two[5:].mean(0))
    np.testing.assert_allclose(np.array([lo2, hi2]), np.percentile(two[5:], [2.5, 97.5], axis=0), rtol=1e-15)
    w = rs.rand(6, 40) + 0.1
    meanw, low, hiw = g.summarize_sampler(chain, weights=w, burn=10, chain_mask=mask, ci=0.8)
    wf = w[mask, 10:].ravel()
    np.testing.assert_allclose(meanw, wf.dot(flat) / wf.sum(), rtol=1e-14)
    for i in range(3):
        edge = 100.0 * (1.0 - 0.8) / 2.0
        np.testing.assert_allclose(low[i], _weighted_percentile(flat[:, i], wf, edge), rtol=1e-12)
        np.testing.assert_allclose(hiw[i], _weighted_percentile(flat[:, i], wf, 100.0 - edge), rtol=1e-12)
    with pytest.raises(ValueError):
        g.summarize_sampler(rs.randn(2, 3, 10, 2))


# ---- 6. the library route's eligibility, arguments --------------------------------------------------------------------------------
def _se(g, d=1, **kw):
    return g.SquaredExponentialKernel(num_dim=d, initial_params=[1.0] + [0.3] * d, param_bounds=[(0.1, 10.0)] * (d + 1), **kw)


def _gp(g, k, d=1, n_obs=12, **kw):
    rs = np.random.RandomState(0)
    X = rs.rand(n_obs, d)
    kw.setdefault("noise_k", g.DiagonalNoiseKernel(d, initial_noise=0.1, noise_bound=(1e-3, 1.0)))
    return g.GaussianProcess(k, X=X, y=rs.randn(n_obs), err_y=0.05, **kw)


def test_library_route_eligibility(g):
    assert _gp(g, _se(g))._library_stepping_refusal() is None
    rq = g.RationalQuadraticKernel(num_dim=1, initial_params=[1.0, 2.0, 0.5], param_bounds=[(0.1, 10.0)] * 3)
    rs = np.random.RandomState(1)
    withT = g.GaussianProcess(rq + _se(g), X=rs.rand(12, 1), y=rs.randn(5), err_y=0.1, T=rs.rand(5, 12))
    assert withT._library_stepping_refusal() is None
    refusal, plan = withT._library_stepping()
    assert refusal is None and list(plan["free_idx"]) == [0, 1, 2, 3, 4] and plan["lo"].shape == (5,)
    assert plan["log_prior"] == withT.hyperprior(withT.params)
    refusal, plan = _gp(g, _se(g))._library_stepping()
    assert list(plan["free_idx"]) == [0, 1, 2]                   # the noise sigma: the length of the kernel's parameters

    mean = g.ConstantMeanFunction(initial_params=[0.0], param_bounds=[(-1.0, 1.0)])
    assert "mean function" in _gp(g, _se(g), mu=mean)._library_stepping_refusal()
    warped = g.BetaWarpedKernel(_se(g))
    assert "warp" in _gp(g, warped)._library_stepping_refusal()
    masked = g.MaskedKernel(_se(g), total_dim=2, mask=[0]) * g.MaskedKernel(_se(g), total_dim=2, mask=[1])
    assert "MaskedKernel" in _gp(g, masked, d=2)._library_stepping_refusal()
    normal = _se(g)
    normal.hyperprior = g.NormalJointPrior([1.0, 0.3], [0.2, 0.1])
    assert "NormalJointPrior" in _gp(g, normal)._library_stepping_refusal()

    class Mine(g.SquaredExponentialKernel):
        def __call__(self, *a, **kw):
            return g.SquaredExponentialKernel.__call__(self, *a, **kw)
    mine = Mine(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.1, 10.0)] * 2)
    assert "Python-defined" in _gp(g, mine)._library_stepping_refusal()

    for gp in (_gp(g, _se(g), mu=mean), _gp(g, warped), _gp(g, mine)):
        with pytest.raises(ValueError) as err:
            gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=2, stepping="library")
        assert gp._library_stepping_refusal() in str(err.value)
        assert gp._ctx_obj is None                               # before any device call


def test_sampling_arguments(g):
    gp = _gp(g, _se(g))
    with pytest.raises(NotImplementedError):
        gp.sample_hyperparameter_posterior(sampler_type="pt")
    with pytest.raises(NotImplementedError):
        gp.sample_hyperparameter_posterior(plot_posterior=True)
    with pytest.raises(NotImplementedError):
        gp.sample_hyperparameter_posterior(plot_chains=True)
    with pytest.raises(ValueError):
        gp.sample_hyperparameter_posterior(stepping="device")
    assert gp._ctx_obj is None
    with pytest.raises(NotImplementedError, match="flat_trace"):
        gp.predict_MCMC(np.zeros((2, 1)))


# ---- 7. no GPU: a loud failure, not a chain of -inf -------------------------------------------------------------------------------
@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
@pytest.mark.parametrize("stepping", ["auto", "host", "library"])
def test_sampling_fails_loudly_without_gpu(g, stepping):
    from gptools_amd import _lib
    gp = _gp(g, _se(g))
    before = list(gp.free_params[:])
    with pytest.raises(_lib.GPTBackendError):
        gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=3, stepping=stepping, random_state=0)
    assert list(gp.free_params[:]) == before
