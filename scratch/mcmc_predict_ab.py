"""Prediction marginalised over a hyperparameter trace: the batched route (gpt_fit_batch_terms + gpt_predict_batch) against the
loop route (update_hyperparameters + predict per row, forced by batch_grid_max_n = 0), in one process, by wall clock.

    python scratch/mcmc_predict_ab.py                  # the table of DESIGN.md section 9: N x M x S, std-only and cov
    python scratch/mcmc_predict_ab.py --one N M S      # one marginal prediction (cov), batched route -- for rocprofv3
"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import gptools_amd as g      # noqa: E402


def make(N, M, S, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-3.0, 3.0, (N, 2))
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]) + 0.02 * rs.randn(N)
    gp = g.GaussianProcess(g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 1.0, 1.0],
                                                      param_bounds=[(1e-3, 10.0)] * 3))
    gp.add_data(X, y, err_y=0.05)
    Xs = rs.uniform(-3.0, 3.0, (M, 2))
    trace = np.column_stack([rs.uniform(0.8, 1.4, S), rs.uniform(0.9, 1.5, S), rs.uniform(0.9, 1.5, S)])
    return gp, Xs, trace


def timed(fn, reps):
    fn()                                                    # warm-up: allocations, first launches
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        N, M, S = (int(v) for v in sys.argv[2:5])
        gp, Xs, trace = make(N, M, S)
        gp.predict_MCMC(Xs, flat_trace=trace, return_cov=True)
        gp.predict_MCMC(Xs, flat_trace=trace, return_cov=True)
        return
    print("%6s %6s %5s %5s %12s %12s %8s" % ("N", "M", "S", "what", "batched_ms", "loop_ms", "ratio"))
    for N in (256, 1024, 4096):
        for M in (64, 1024):
            for S in (64, 256):
                gp, Xs, trace = make(N, M, S)
                for what, kw in (("std", dict(return_std=True)), ("cov", dict(return_cov=True))):
                    gp.batch_grid_max_n = 4096
                    tb = timed(lambda: gp.predict_MCMC(Xs, flat_trace=trace, **kw), 2)
                    gp.batch_grid_max_n = 0
                    tl = timed(lambda: gp.predict_MCMC(Xs, flat_trace=trace, **kw), 1)
                    print("%6d %6d %5d %5s %12.2f %12.2f %8.2f" % (N, M, S, what, 1e3 * tb, 1e3 * tl, tl / tb), flush=True)
                gp._ctx.release_batch_scratch()


if __name__ == "__main__":
    main()
