"""Host suite (no GPU): the yardstick of the greedy inducing-input selection (tests/greedy_cases.py) and what the Python layer decides
without a device.

test_yardstick is the measurement behind greedy_cases.HOST_ERR / TRACE_ERR and asserts the conditions that make the device tests
meaningful: the gap condition (the pivots are decided far above the rounding of a residual), equal pivots in float64 and
longdouble, and trace_M = tr(K_ff - K_fu K_uu^-1 K_uf).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import greedy_cases as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_yardstick(oracle, name):
    c = G.CASES[name]
    K, rows, y64, yld = G.reference(oracle, name)
    M = c["M"]
    first = 0 if not G.STATIONARY[name] else 1
    gap = y64["gap"][first:].min()
    herr = G.host_figures(y64, yld)
    terr = abs(float(y64["trace"][-1]) - G.nystrom_trace(K, y64["idx"])) / y64["kmax"]
    print("%s: %d candidates of N = %d, M = %d: smallest gap %.3g of max k_ii (from step %d)" % (name, len(rows), c["N"], M, gap, first))
    print('    HOST_ERR "%s": %.3g,   TRACE_ERR "%s": %.3g   (dmax_M-1 = %.3g, trace_M = %.6g, max k_ii = %.6g)'
          % (name, herr, name, terr, float(y64["dmax"][-1]), float(y64["trace"][-1]), y64["kmax"]))
    assert len(rows) == c["N"] - c["nder"]
    assert y64["count"] == M and yld["count"] == M
    assert gap >= G.GAP_MIN, (name, gap)
    assert np.array_equal(y64["idx"], yld["idx"])
    if G.STATIONARY[name]:
        assert np.unique(np.diag(K)).size == 1                       # the complete tie of step 0: the lowest candidate
        assert y64["idx"][0] == 0 and y64["gap"][0] == 0.0
    assert np.all(np.diff(y64["trace"]) < 0.0) and np.all(y64["dmax"] > 0.0)
    # the recorded constants, and the host itself held to what the device is held to
    assert G.HOST_ERR[name] <= 1e-10 and G.TRACE_ERR[name] <= 1e-10
    assert herr <= max(10.0 * G.HOST_ERR[name], len(rows) * (M + 2) * G.U), (herr, G.HOST_ERR[name])
    assert terr <= max(10.0 * G.TRACE_ERR[name], len(rows) * M * G.U), (terr, G.TRACE_ERR[name])


def test_greedy_beats_random_subsets_on_the_host(oracle):
    """The property test 5 of the GPU suite asks of the device, first on the host: the Nystrom trace of the greedy 64 rows is at most
    half that of each seeded random subset."""
    K, rows, _, _ = G.reference(oracle, G.CLASS_CASE)
    y = G.yardstick(K, G.CLASS_M)
    assert abs(float(y["trace"][-1]) - G.nystrom_trace(K, y["idx"])) <= 1e-10 * y["kmax"]
    for seed in G.CLASS_SEEDS:
        t = G.nystrom_trace(K, G.random_subset(len(rows), G.CLASS_M, seed))
        print("seed %d: random subset %.6g, greedy %.6g, factor %.3g" % (seed, t, float(y["trace"][-1]), t / float(y["trace"][-1])))
        assert t >= 2.0 * float(y["trace"][-1]), seed


def test_yardstick_stop_rule_and_ties(oracle):
    """Every point twice: the pivots are the lower rows of their pairs, and with tol > 0 the loop stops when the 60 distinct points are
    used up (the case of the GPU suite's contract test)."""
    X, _ = G.case_points("m52_m63")
    X2 = np.concatenate([X[:60], X[:60]])
    K = G.gram(oracle, G.CASES["m52_m63"]["terms"], X2)
    y = G.yardstick(K, 60)
    assert y["count"] == 60 and np.all(y["idx"] < 60)
    y = G.yardstick(K, 90, tol=1e-9)
    print("duplicates: count %d, residual after 60 pivots %.3g" % (y["count"], float(y["trace"][-1])))
    assert y["count"] == 60


def test_python_layer_refusals_need_no_device():
    import warnings
    warnings.simplefilter("ignore")
    import gptools_amd as g
    assert callable(g.greedy_inducing) and callable(g.SparseGaussianProcess.select_inducing)

    class Mine(g.SquaredExponentialKernel):
        def __call__(self, *a, **k):
            return super(Mine, self).__call__(*a, **k)
    X = np.random.RandomState(0).rand(10, 1)
    with pytest.raises(NotImplementedError, match="not one the library evaluates itself"):
        g.greedy_inducing(Mine(num_dim=1, initial_params=[1.0, 0.3]), X, 3)
    k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.0, 0.3])
    sgp = g.SparseGaussianProcess(k, X[:2])
    with pytest.raises(g.GPArgumentError):
        sgp.select_inducing(3)
