"""GPU suite: GaussianProcess.sample_hyperparameter_posterior -- the library route (gpt_ensemble_run) against the host route bit
for bit, the stored log-probabilities against update_hyperparameters, the sampled posterior against quadrature on a grid, and
the sampler through predict_MCMC."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def _model_a(g):
    """SE, d = 2, N = 150 (padded order 256: two leaves, the smallest batched factorisation with an update step), the last 10 rows
    first derivatives in dimension 0, free noise."""
    rs = np.random.RandomState(21)
    N = 150
    X = rs.rand(N, 2)
    n = np.zeros((N, 2), dtype=int)
    n[N - 10:, 0] = 1
    y = np.where(n[:, 0] == 1, np.cos(3.0 * X.sum(1)) * 3.0, np.sin(3.0 * X.sum(1))) + 0.05 * rs.randn(N)
    box = [(0.1, 5.0), (0.05, 2.0), (0.05, 2.0)]
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.4, 0.5], param_bounds=box)
    nk = g.DiagonalNoiseKernel(2, initial_noise=0.05, noise_bound=(1e-3, 1.0))
    return g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.02, n=n), np.array(box + [(1e-3, 1.0)])


def _model_b(g):
    """RQ + SE, d = 1, 150 latent points seen as 60 observations through a random T, the noise fixed."""
    rs = np.random.RandomState(22)
    X = np.sort(rs.rand(150))
    T = rs.rand(60, 150) / 150.0
    y = T.dot(np.sin(6.0 * X)) + 0.01 * rs.randn(60)
    box = [(0.1, 3.0), (0.1, 5.0), (0.05, 2.0), (0.1, 3.0), (0.05, 2.0)]
    k = (g.RationalQuadraticKernel(num_dim=1, initial_params=[1.0, 2.0, 0.5], param_bounds=box[:3])
         + g.SquaredExponentialKernel(num_dim=1, initial_params=[0.5, 0.2], param_bounds=box[3:]))
    nk = g.DiagonalNoiseKernel(1, initial_noise=0.02, fixed_noise=True)
    return g.GaussianProcess(k, noise_k=nk, X=X, y=y, err_y=0.01, T=T), np.array(box)


def _outside_proposals(g, sampler, theta0, box, seed, a=2.0):
    """Proposals of the run that left the box, rebuilt from the chain and the variates of the same seed: ``(count, stayed)`` --
    how many there were, and whether every walker whose proposal left the box kept its position in that half-step."""
    from gptools_amd.sampler import draw_variates
    K, nsteps, _ = sampler.chain.shape
    h = K // 2
    us, pj, _ = draw_variates(np.random.RandomState(seed), K, nsteps)
    states = np.concatenate((theta0[None], np.transpose(sampler.chain, (1, 0, 2))))
    count, stayed = 0, True
    for s in range(nsteps):
        before, after = states[s], states[s + 1]
        for sl, S, C in ((slice(0, h), before[:h], before[h:]), (slice(h, K), before[h:], after[:h])):
            t = (a - 1.0) * us[s, sl] + 1.0
            z = t * t / a
            Cj = C[pj[s, sl]]
            q = Cj - z[:, None] * (Cj - S)
            out = ~((box[:, 0] <= q) & (q <= box[:, 1])).all(1)
            count += int(out.sum())
            stayed = stayed and np.array_equal(after[sl][out], S[out])
    return count, stayed


@pytest.fixture(scope="module")
def runs(g):
    """Both routes on both models, once: ``runs[name] = (gp, box, theta0, host sampler, library sampler)``."""
    res = {}
    for name, make, seed in (("a", _model_a, 31), ("b", _model_b, 32)):
        gp, box = make(g)
        theta0 = np.random.RandomState(seed).uniform(box[:, 0], box[:, 1], size=(16, len(box)))      # the whole prior box
        before = np.array(gp.free_params[:], dtype=float)
        host = gp.sample_hyperparameter_posterior(nwalkers=16, nsamp=30, theta0=theta0, random_state=seed, stepping="host")
        lib = gp.sample_hyperparameter_posterior(nwalkers=16, nsamp=30, theta0=theta0, random_state=seed, stepping="library")
        np.testing.assert_array_equal(np.array(gp.free_params[:], dtype=float), before)
        res[name] = (gp, box, theta0, host, lib, seed)
    return res


# ---- 8. the routes agree bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_routes_agree_bit_for_bit(g, runs, name):
    gp, box, theta0, host, lib, seed = runs[name]
    assert host.route == "host" and lib.route == "library"
    assert host.chain.shape == (16, 30, len(box)) and lib.chain.shape == host.chain.shape
    np.testing.assert_array_equal(lib.chain, host.chain)
    np.testing.assert_array_equal(lib.lnprobability, host.lnprobability)
    np.testing.assert_array_equal(lib.acceptance_fraction, host.acceptance_fraction)
    moved = (np.diff(host.chain, axis=1) != 0).any(2).sum()
    assert 0 < moved < 16 * 29 and np.isfinite(host.lnprobability[:, -1]).any()
    outside, stayed = _outside_proposals(g, host, theta0, box, seed)
    print("model %s: %d of %d proposals left the box, %d moves" % (name, outside, 16 * 30, moved))
    assert outside >= 1 and stayed                               # the case occurred, and none of them was accepted
    assert ((box[:, 0] <= host.chain) & (host.chain <= box[:, 1])).all()


# ---- 9. the stored log-probabilities are the model's -----------------------------------------------------------------------------
def _check_stored(gp, sampler, count=20, seed=0):
    rs = np.random.RandomState(seed)
    K, S, _ = sampler.chain.shape
    finite = 0
    for w, s in zip(rs.randint(K, size=count), rs.randint(S, size=count)):
        stored = sampler.lnprobability[w, s]
        assert -1.0 * gp.update_hyperparameters(sampler.chain[w, s]) == stored, (w, s, stored)
        finite += np.isfinite(stored)
    assert finite > 0


def test_stored_lnprob_is_update_hyperparameters(runs):
    gp, _, _, _, lib, _ = runs["a"]
    before = np.array(gp.free_params[:], dtype=float)
    _check_stored(gp, lib)
    gp.update_hyperparameters(before)


# ---- 10. the posterior against quadrature ----------------------------------------------------------------------------------------
def test_posterior_against_quadrature(g):
    """Bounds: |mean - mean_grid| <= 0.25 std_grid, |std / std_grid - 1| <= 0.15, no walker's acceptance below 0.05.  A numpy
    restatement on the CPU over seeds 0 to 7 gave at worst 0.099 and 0.066, acceptance 0.66 and no stuck walker; the grid moments
    move by 4e-4 sigma from 150 to 300 points, 2e-4 of the mass lies on the box's edge."""
    rs = np.random.RandomState(11)
    x = np.sort(rs.rand(40))
    K = 1.3 ** 2 * np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 0.25 ** 2) + 1e-10 * np.eye(40)
    y = np.linalg.cholesky(K).dot(rs.randn(40)) + 0.1 * rs.randn(40)
    box = np.array([(0.2, 5.0), (0.05, 2.0)])
    k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[tuple(b) for b in box])
    gp = g.GaussianProcess(k, X=x, y=y, err_y=0.1)
    ll, axes = gp.compute_ll_matrix(box, 150)
    w = np.exp(ll - ll.max())
    w /= w.sum()
    grids = np.meshgrid(*axes, indexing="ij")
    mean_grid = np.array([(w * m).sum() for m in grids])
    std_grid = np.sqrt(np.array([(w * (m - mu) ** 2).sum() for m, mu in zip(grids, mean_grid)]))
    np.random.seed(0)                                            # (the starting draw of the hyperprior)
    s = gp.sample_hyperparameter_posterior(nwalkers=64, nsamp=600, random_state=0)
    flat = s.chain[:, 200:, :].reshape(-1, 2)
    dev_mean = np.abs(flat.mean(0) - mean_grid) / std_grid
    dev_std = np.abs(flat.std(0) / std_grid - 1.0)
    print("route %s; grid mean %s std %s; sampled mean %s std %s; |dmean| / std %s, |std ratio - 1| %s; acceptance %.3f (least %.3f)"
          % (s.route, mean_grid, std_grid, flat.mean(0), flat.std(0), dev_mean, dev_std, s.acceptance_fraction.mean(),
             s.acceptance_fraction.min()))
    assert s.route == ("library" if gp.sampler_auto_route == "library" else "host")
    assert (dev_mean <= 0.25).all() and (dev_std <= 0.15).all()
    assert (s.acceptance_fraction >= 0.05).all()


# ---- 11. end to end -------------------------------------------------------------------------------------------------------------
def test_sampler_through_predict_mcmc_and_continuation(g):
    rs = np.random.RandomState(5)
    x = np.sort(rs.rand(50))
    y = np.sin(5.0 * x) + 0.1 * rs.randn(50)
    box = [(0.2, 5.0), (0.05, 2.0)]

    def make():
        k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=box)
        nk = g.DiagonalNoiseKernel(1, initial_noise=0.1, noise_bound=(0.01, 1.0))
        return g.GaussianProcess(k, noise_k=nk, X=x, y=y, err_y=0.02)
    gp = make()
    theta0 = np.random.RandomState(6).uniform([0.5, 0.1, 0.05], [2.0, 0.6, 0.3], size=(16, 3))
    p0 = [1.2, 0.25, 0.12]
    ll0 = gp.update_hyperparameters(p0)
    s = gp.sample_hyperparameter_posterior(nwalkers=16, nsamp=30, theta0=theta0, random_state=3)
    assert s.chain.shape == (16, 30, 3) and gp.K_up_to_date and -1.0 * gp.ll == ll0
    np.testing.assert_array_equal(np.array(gp.free_params[:], dtype=float), p0)
    Xs = np.linspace(0.0, 1.0, 7)
    via_sampler = gp.predict_MCMC(Xs, sampler=s, burn=10, thin=5)
    via_trace = gp.predict_MCMC(Xs, flat_trace=s.chain[:, 10::5, :].reshape(-1, 3))
    assert set(via_sampler) == set(via_trace) and "mean" in via_sampler and "std" in via_sampler
    for key in via_trace:
        np.testing.assert_array_equal(via_sampler[key], via_trace[key])
    last = np.array(s.chain[:, -1, :])
    again = gp.sample_hyperparameter_posterior(nsamp=20, sampler=s)
    assert again is s and s.chain.shape == (16, 50, 3)
    np.testing.assert_array_equal(np.array(gp.free_params[:], dtype=float), p0)
    # ... from the last position: a walker's first new state is that position or a move away from it, and the whole chain is
    # the chain of one run of 50 steps
    stay = (s.chain[:, 30, :] == last).all(1)
    assert stay.any() and not stay.all()
    whole = make().sample_hyperparameter_posterior(nwalkers=16, nsamp=50, theta0=theta0, random_state=3)
    np.testing.assert_array_equal(s.chain, whole.chain)
    np.testing.assert_array_equal(s.lnprobability, whole.lnprobability)

    class Foreign(object):                                       # any object with run_mcmc and chain: called as the reference does
        chain = np.empty((16, 0, 3))
        calls = []

        def run_mcmc(self, pos, nsteps):
            self.calls.append((np.array(pos), nsteps))
    f = Foreign()
    assert gp.sample_hyperparameter_posterior(nsamp=4, sampler=f, theta0=theta0) is f
    assert len(f.calls) == 1 and f.calls[0][1] == 4 and np.array_equal(f.calls[0][0], theta0) and f.a == 2.0


# ---- 12. a model with a mean function: the host route ---------------------------------------------------------------------------
def test_mean_function_model_takes_host_route(g):
    rs = np.random.RandomState(8)
    x = np.sort(rs.rand(60))
    y = 0.7 + np.sin(5.0 * x) + 0.1 * rs.randn(60)
    k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3], param_bounds=[(0.2, 5.0), (0.05, 2.0)])
    mu = g.ConstantMeanFunction(initial_params=[0.5], param_bounds=[(-2.0, 2.0)])
    gp = g.GaussianProcess(k, X=x, y=y, err_y=0.1, mu=mu)
    theta0 = np.random.RandomState(9).uniform([0.5, 0.1, 0.0], [2.0, 0.6, 1.0], size=(16, 3))
    s = gp.sample_hyperparameter_posterior(nwalkers=16, nsamp=20, theta0=theta0, random_state=1, stepping="auto")
    assert s.route == "host" and s.chain.shape == (16, 20, 3)
    assert (np.diff(s.chain, axis=1) != 0).any()
    _check_stored(gp, s)
    with pytest.raises(ValueError, match="mean function"):
        gp.sample_hyperparameter_posterior(nwalkers=16, nsamp=2, theta0=theta0, stepping="library")
