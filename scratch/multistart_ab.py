"""Multi-start MAP: the starts in lockstep (optimize_hyperparameters(batch_starts=True): one ll_gradient_batch per round) against
the starts one after another (one fit and one ll_gradient per evaluation), gradient="device" both, the same seeded starts, in one
process, by wall clock.  Matern-5/2, d = 2, free noise, SLSQP.

    python scratch/multistart_ab.py                  # the table of DESIGN.md section 14: N x R, and one batched gradient of 32 points
"""
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, ".")
import gptools_amd as g      # noqa: E402


def make(N, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-3.0, 3.0, (N, 2))
    y = np.sin(X[:, 0]) * np.cos(0.5 * X[:, 1]) + 0.05 * rs.randn(N)
    gp = g.GaussianProcess(g.Matern52Kernel(num_dim=2, initial_params=[1.0, 1.0, 1.0], param_bounds=[(0.05, 10.0)] * 3),
                           noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=0.1, noise_bound=(1e-3, 2.0)))
    gp.add_data(X, y, err_y=0.01)
    return gp


def optimise(gp, R, lockstep, seed=77):
    np.random.seed(seed)
    t0 = time.perf_counter()
    best, done = gp.optimize_hyperparameters(random_starts=R, gradient="device", batch_starts=lockstep,
                                             opt_kwargs={"options": {"ftol": 1e-6}})
    return time.perf_counter() - t0, best, done


def timed(fn, reps):
    fn()                                                    # warm-up: allocations, first launches
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    warnings.simplefilter("ignore")
    print("%6s %4s %14s %14s %8s %16s %16s" % ("N", "R", "lockstep_ms", "sequential_ms", "ratio", "best_lockstep", "best_sequential"))
    for N in (256, 1024, 4096):
        gp = make(N)
        optimise(gp, 2, True)                               # warm-up of both routes: scratch, first launches
        optimise(gp, 2, False)
        for R in (8, 32):
            tb, bb, db = optimise(gp, R, True)
            ts, bs, ds = optimise(gp, R, False)
            print("%6d %4d %14.1f %14.1f %8.2f %16.9g %16.9g   starts completed %d / %d" % (N, R, 1e3 * tb, 1e3 * ts, ts / tb, bb.fun, bs.fun, db, ds),
                  flush=True)
        # one round of 32 points: the batched value + gradient against 32 x (update_hyperparameters + ll_gradient), and the host's
        # share of the batched call (the 32 stencils)
        rs = np.random.RandomState(5)
        theta = np.array(gp.free_params[:], dtype=float)
        pts = [theta * (1.0 + 0.2 * rs.uniform(-1.0, 1.0, len(theta))) for _ in range(32)]

        def loop():
            for p in pts:
                gp.update_hyperparameters(p)
                gp.ll_gradient()

        def stencils():
            for p in pts:
                gp._assign_free(p)
                gp._ll_gradient_stencil(6e-6)
        t_alone = timed(lambda: gp.ll_gradient_batch(pts), 2)       # (a scratch above 2 GiB goes back to the device after the call)
        gp._hold_batch_scratch = True                               # ... and as a lockstep optimisation calls it: the scratch is held
        t_batch = timed(lambda: gp.ll_gradient_batch(pts), 3)
        few = ["%d: %.2f" % (nb, 1e3 * timed(lambda: gp.ll_gradient_batch(pts[:nb]), 3)) for nb in (1, 2, 8)]     # the rounds of a run's end
        gp._hold_batch_scratch = False
        t_loop = timed(loop, 2)
        t_host = timed(stencils, 3)
        print("%6d   32 points: ll_gradient_batch %.2f ms (of which the host's 32 stencils %.2f ms; %.2f ms when it returns its scratch), "
              "32 x (update + ll_gradient) %.2f ms, ratio %.2f" % (N, 1e3 * t_batch, 1e3 * t_host, 1e3 * t_alone, 1e3 * t_loop, t_loop / t_batch),
              flush=True)
        print("%6s   ll_gradient_batch of fewer points [ms]: %s; one update + ll_gradient %.2f" % ("", ", ".join(few), 1e3 * t_loop / 32), flush=True)
        gp._ctx.release_batch_scratch()


if __name__ == "__main__":
    main()
