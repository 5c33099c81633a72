"""No GPU: the host's yardstick of the batched sparse fit and what SparseGaussianProcess.sparse_ll_batch decides before it meets a device.

test_host_routes_of_the_elements is the measurement behind sparse_batch_cases.HOST_ERR_BATCH: Woodbury against dense at every element of
every case tests/test_gpu_sparse_batch.py fits.  It prints the table, asserts every figure and every recorded constant of the fit group
<= 1e-10 and of the VFE trace term <= 1e-9 (sparse_batch_cases: why), and holds the host itself to the bound the device is held to."""
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_batch_cases as SB

PARAMS = [(name, m) for name in SB.BATCH_CASES for m in S.CASES[name]["methods"]]


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def test_elements():
    """Element 0 is the case; the others scale every kernel parameter within (0.85, 1.2), term by term from one generator."""
    for name in SB.BATCH_CASES:
        els = SB.element_terms(name)
        assert len(els) == SB.NELEM and [tuple(t) for t in S.CASES[name]["terms"]] == els[0]
        draws = np.random.RandomState(211).uniform(0.85, 1.2, size=4 * sum(len(p) for t in els[0] for p in t[1::2]))
        ratio = np.concatenate([np.asarray(p) / np.asarray(p0) for el in els[1:] for t, t0 in zip(el, els[0])
                                for p, p0 in zip(t[1::2], t0[1::2])])
        np.testing.assert_allclose(ratio, draws, rtol=1e-15, atol=0)
        assert [t[0::2] for t in els[3]] == [t[0::2] for t in els[0]]
    assert SB.element_noise() == [S.NOISE * f for f in (1.0, 0.7, 1.5, 1.0, 2.0)]


@pytest.mark.parametrize("name,method", PARAMS)
def test_host_routes_of_the_elements(oracle, name, method):
    N = S.CASES[name]["N"]
    for b in range(SB.NELEM):
        w, d = SB.host_routes(oracle, name, method, b)
        fig = SB.fit_figures(w, d)
        print('    ("%s", "%s", %d): {%s},   # cond(K_uu + jitter I) = %.1e' % (name, method, b, ", ".join('"%s": %.3g' % (k, fig[k]) for k in SB.FIT_FIGURES),
                                                                              w["cond_uu"]))
        assert np.all(w["lam"] > 0.0) and w["cond_uu"] <= 3.2e8
        for k in SB.FIT_FIGURES:
            ceiling = SB.CEILING[SB.group_of(k)]
            assert SB.HOST_ERR_BATCH[(name, method, b)][k] <= ceiling, k
            assert fig[k] <= ceiling, (k, fig[k])
            assert fig[k] <= SB.bound(name, k, N), (k, fig[k], SB.bound(name, k, N))


# ---- SparseGaussianProcess.sparse_ll_batch without a device --------------------------------------------------------------------
def make(g, **kw):
    d = S.case_data("se_300")
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, param_bounds=[(0.0, 1e3)] * 3)
    args = dict(noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=S.NOISE, noise_bound=(0.0, 5.0)), X=d["X"], y=d["y"], err_y=0.02,
                n=d["n"])
    args.update(kw)
    return g.SparseGaussianProcess(args.pop("k", k), args.pop("Z", d["Z"]), **args)


def test_vectors_the_prior_excludes_never_reach_a_device(g, monkeypatch):
    gp = make(g)
    here = np.array(gp.free_params[:], dtype=float)
    monkeypatch.setattr(type(gp), "_resident_ctx", lambda self: pytest.fail("a device was asked for"))
    out = gp.sparse_ll_batch([[-1.0, 0.4, 0.6, 0.1], [1.1, 2e3, 0.6, 0.1], [1.1, 0.4, 0.6, 7.0]])
    assert out.shape == (3,) and np.all(np.isneginf(out))
    assert np.array_equal(gp.free_params[:], here) and not gp.K_up_to_date
    assert gp.sparse_ll_batch([]).shape == (0,)


def test_element_bytes(g):
    """The layout of api_sparse_batch.inc, written out for M = 40, N = 300 (MPU = BP = LDV = 128, MG = 64, one tile)."""
    gp = make(g)
    chunk, per = gp._sparse_batch_element_bytes()
    assert chunk == 320                                  # N to 64: the default budget holds far more rows
    slices = min(1536, 75, 1024)                         # one tile: six times 256 units, at most a slice per four rows
    assert per == 8 * (320 * 128 + 128 * 128 + 9216 + 128 * 128 + 9216 + 64 * 64 + 4096 * slices + 3 * 320 + 300)
    gp = make(g, chunk_rows=128)
    chunk, per = gp._sparse_batch_element_bytes()
    assert chunk == 128 and per == 8 * (128 * 128 + 2 * (128 * 128 + 9216) + 64 * 64 + 4096 * 32 + 3 * 128 + 300)
    # M = 128: MPU = 128 < BP = 256, MG = 192 (six tiles)
    gp = make(g, Z=np.random.RandomState(1).rand(128, 2))
    chunk, per = gp._sparse_batch_element_bytes()
    assert per == 8 * (320 * 256 + 128 * 128 + 9216 + 256 * 256 + 2 * 9216 + 192 * 192 + 4096 * 75 * 6 + 3 * 320 + 300)


def test_the_refusals_beside_it_stand(g):
    gp = make(g)
    x0 = np.array(gp.free_params[:], dtype=float)
    with pytest.raises(NotImplementedError, match="sparse_ll_batch"):
        gp.ll_batch([x0])
    with pytest.raises(NotImplementedError):
        gp.ll_gradient_batch([x0])
    with pytest.raises(NotImplementedError):
        gp.optimize_hyperparameters(batch_starts=True, random_starts=2)
    with pytest.raises(ValueError):
        gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=1, stepping="library")


def test_mixed_model_shapes_go_row_by_row(g, monkeypatch):
    """Elements that are not one model shape (here: _device_terms answers another kernel id for the second vector) never reach the
    batched call: every vector goes through update_hyperparameters, in order."""
    from gptools_amd import sparse
    gp = make(g)
    seen, calls = [], [0]
    real = sparse._device_terms

    def terms(obj):
        calls[0] += 1
        t = real(obj)
        return t if calls[0] != 2 else [(t[0][0] + 1,) + tuple(t[0][1:])]
    monkeypatch.setattr(sparse, "_device_terms", terms)
    monkeypatch.setattr(type(gp), "_resident_ctx", lambda self: pytest.fail("the batched route was taken"))
    monkeypatch.setattr(type(gp), "update_hyperparameters", lambda self, p, **kw: seen.append(np.array(p)) or -float(len(seen)))
    gp.K_up_to_date = True
    vecs = [[1.1, 0.4, 0.6, 0.1], [1.0, 0.5, 0.6, 0.1], [0.9, 0.4, 0.5, 0.2]]
    out = gp.sparse_ll_batch(vecs)
    assert np.array_equal(out, [1.0, 2.0, 3.0]) and np.array_equal(np.array(seen), np.array(vecs))
    assert not gp.K_up_to_date                            # (the rows replaced the resident fit)


def test_grid_of_one_is_the_loop(g, monkeypatch):
    gp = make(g)
    gp.sparse_batch_grid = 1
    seen = []
    monkeypatch.setattr(type(gp), "sparse_ll_batch", lambda self, pl, **kw: pytest.fail("batched"))
    monkeypatch.setattr(type(gp), "update_hyperparameters", lambda self, p, **kw: seen.append(1) or 2.5)
    assert np.array_equal(gp._ll_rows([[1.1, 0.4, 0.6, 0.1]] * 3), [-2.5] * 3) and len(seen) == 3
