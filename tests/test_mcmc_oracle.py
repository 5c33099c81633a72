"""CPU suite: predictions marginalised over a hyperparameter trace (tests/golden/g14_mcmc.npz, from the reference's
compute_from_MCMC / predict_MCMC / predict(use_MCMC=True)) reproduced by composing the oracle's fit + predict per trace row
with the laws of total variance / covariance in numpy.  Pins both the fixture and the formula the GPU path implements."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, assert_close

sys.path.insert(0, GOLDEN)
import gen_g14_mcmc as G14      # noqa: E402


def _case(golden, name):
    g = golden("g14_mcmc")
    d = {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(name + "__") and k.count("__") == 1}
    res = {}
    for k, v in g.items():
        parts = k.split("__")
        if parts[0] == name and len(parts) == 3:
            res.setdefault(parts[1], {})[parts[2]] = v
    return d, res


# single-kernel cases the oracle covers: kernel name, how a trace row splits into (kernel params, noise sigma)
SINGLE = {"se1": ("se", lambda p: (p[:2], p[2])), "m52d": ("m52", lambda p: (p, 0.0)), "drop": ("se", lambda p: (p, 0.0)),
          "ot": ("se", lambda p: (p, 0.0))}


def _rows(oracle, name, d, trace, noise):
    kern, split = SINGLE[name]
    means, covs = [], []
    for p in trace:
        if np.isnan(p).any():
            continue                                          # the evaluation fails: dropped
        kp, sn = split(np.asarray(p, dtype=float))
        try:
            f = oracle.fit(kern, kp, d["X"], d["n"], d["y"], d["err_y"], noise_var=sn ** 2.0)
        except np.linalg.LinAlgError:
            continue
        m, _, c = oracle.predict(kern, kp, d["X"], d["n"], f["L"], f["alpha"], d["Xs"], d["ns"],
                                 noise_params=[sn] if noise and sn > 0 else None,
                                 noise_n=np.zeros(d["X"].shape[1], dtype=np.int32) if noise and sn > 0 else None)
        if "A" in d:
            m, c = d["A"].dot(m), d["A"].dot(c).dot(d["A"].T)
        means.append(m)
        covs.append(c)
    return np.array(means), np.array(covs)


def _marginal(means, covs, ddof):
    mean = np.mean(means, axis=0)
    cov = np.mean(covs, axis=0) + np.cov(means, rowvar=0, ddof=ddof)
    var_only = np.mean(np.array([np.diagonal(c) for c in covs]), axis=0) + np.var(means, axis=0, ddof=ddof)
    return mean, cov, np.sqrt(np.diagonal(cov)), np.sqrt(var_only)


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_g14_oracle_composition_reproduces_reference(oracle, golden, name):
    d, res = _case(golden, name)
    scale = 10.0                                             # (sigma_f^2 of the traces is at most ~2.6: absolute 1e-10 of it)
    for call, meth, kw in G14.CALLS[name]:
        r = res[call]
        noise = bool(kw.get("noise", False))
        trace = d["trace"]
        if "burn" in kw or "thin" in kw:
            trace = trace[kw.get("burn", 0)::kw.get("thin", 1)]
        means, covs = _rows(oracle, name, d, trace, noise)
        if meth == "compute_from_MCMC":
            assert r["mean"].shape[0] == len(means), call
            assert_close(means, r["mean"], rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " mean")
            assert_close(np.sqrt(np.array([np.diagonal(c) for c in covs])), r["std"], rtol=1e-10, atol_scale=1e-10 * scale,
                         msg=call + " std")
            if "cov" in r:
                assert_close(covs, r["cov"], rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " cov")
            continue
        mean, cov, std, std_var = _marginal(means, covs, kw.get("ddof", 1))
        assert_close(mean, r["mean"], rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " mean")
        if "cov" in r:
            assert_close(cov, r["cov"], rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " cov")
            assert_close(std, r["std"], rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " std")
        else:
            got = r["std"] if "std" in r else r["second"]
            assert_close(std_var, got, rtol=1e-10, atol_scale=1e-10 * scale, msg=call + " std")


def test_g14_drop_case_keeps_the_excluded_row_and_drops_the_nan_row(golden):
    d, res = _case(golden, "drop")
    assert d["trace"].shape[0] == 12
    assert np.isnan(d["trace"][3]).any() and d["trace"][7, 1] > 10.0
    assert res["cfm"]["mean"].shape[0] == 11


def test_g14_fixture_has_every_case_and_call(golden):
    g = golden("g14_mcmc")
    for name in G14.CASES:
        for call, _, _ in G14.CALLS[name]:
            assert any(k.startswith("%s__%s__" % (name, call)) for k in g), (name, call)
