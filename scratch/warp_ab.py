"""Cost of an input warp: the builder and the whole fit, 2-D squared-exponential kernel, warped (linear +
beta layer) against unwarped on the same points, alternated in one process; warp_points_kernel on its own; and what the device
route buys over the host class.  Medians over REPS repeats after a warm-up.  Usage: python scratch/warp_ab.py [quick]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import gptools_amd as g                     # noqa: E402
from gptools_amd import _lib                # noqa: E402

REPS = 15
quick = len(sys.argv) > 1


def med(f, reps=REPS, warm=3):
    for _ in range(warm):
        f()
    return float(np.median([f() for _ in range(reps)]))


def builder_and_fit():
    rs = np.random.RandomState(0)
    for N in ((4096,) if quick else (4096, 8192, 16384)):
        for deriv in (False, True):
            X = rs.uniform(0.02, 0.98, (N, 2)) * 4.0 - 1.0
            n = np.zeros((N, 2), dtype=int)
            if deriv:
                n[-N // 4:, 0] = 1
            y, err = rs.randn(N), np.full(N, 0.1)
            p = np.array([1.0, 0.3, 0.3])
            ctx = _lib.Context(0)
            ctx.set_option("timing", 1)
            ctx.set_data(X, n)
            layers = [(_lib.WARP_LINEAR, [-1.0, 3.0, -1.0, 3.0]), (_lib.WARP_BETA, [0.8, 1.7, 1.4, 0.9])]
            res = {"plain": [], "warp": []}
            for it in range(REPS + 3):
                for tag in ("plain", "warp"):
                    ctx.set_warp(layers if tag == "warp" else None)
                    ctx.fit(_lib.KERNEL_SE, p if tag == "warp" else p * [1, 4, 4], 0.01, y, err, 1e-10)
                    t = ctx.last_timings()
                    if it >= 3:
                        res[tag].append((t["kbuild"], t["total"]))
            a, b = np.median(res["plain"], axis=0), np.median(res["warp"], axis=0)
            print("N %5d %s  build %.4f -> %.4f ms (x%.3f)   fit %.4f -> %.4f ms (x%.4f)"
                  % (N, "n=1 last quarter" if deriv else "value rows      ", a[0], b[0], b[0] / a[0], a[1], b[1], b[1] / a[1]))


def warp_points_alone():
    rs = np.random.RandomState(1)
    N, D = 16384, 3
    ctx = _lib.Context(0)
    ctx.set_data(rs.uniform(0.02, 0.98, (N, D)), np.zeros((N, D), dtype=int))
    k = [0]

    def one():
        k[0] += 1
        lay = [(_lib.WARP_BETA, np.full(2 * D, 1.0 + 1e-3 * k[0]))]
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.set_warp(lay)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3
    print("gpt_set_warp (warp_points_kernel + launch, host wall) N %d D %d: %.4f ms" % (N, D, med(one)))


def data(rs, N):
    X = rs.uniform(0.02, 0.98, (N, 2))
    n = np.zeros((N, 2), dtype=int)
    n[-N // 4:, 0] = 1
    return X, n, rs.randn(N)


def user_gain():
    rs = np.random.RandomState(2)
    for N in ((512,) if quick else (1024, 4096)):
        X, n, y = data(rs, N)

        def make(host, X=X, n=n, y=y):
            k = g.BetaWarpedKernel(g.SquaredExponentialKernel(num_dim=2, initial_params=[1.0, 0.3, 0.3], param_bounds=[(1e-3, 1e3)] * 3),
                                   initial_params=[0.8, 1.7, 1.4, 0.9], param_bounds=[(1e-2, 1e2)] * 4)
            if host:
                class HostWarped(g.WarpedKernel):
                    def __call__(self, *a, **kw):
                        return g.WarpedKernel.__call__(self, *a, **kw)
                k = HostWarped(k.k, k.w)
            return g.GaussianProcess(k, X=X, y=y, err_y=0.1, n=n)
        out = []
        for host in (False, True):
            gp = make(host)
            free = np.array(gp.free_params[:], dtype=float)
            c = [0]

            def one():
                c[0] += 1
                t0 = time.perf_counter()
                gp.update_hyperparameters(free * (1.0 + 1e-4 * c[0]))
                return (time.perf_counter() - t0) * 1e3
            out.append(med(one, reps=3 if host else REPS, warm=1 if host else 2))
        print("update_hyperparameters N %d: device route %.3f ms, host class route %.1f ms (x%.0f)" % (N, out[0], out[1], out[1] / out[0]))
    N = 1024
    gp = make(False, *data(rs, N))
    assert len(gp.y) == N
    free = np.array(gp.free_params[:], dtype=float)
    plist = [free * (1.0 + 1e-3 * i) for i in range(64)]

    def batch():
        t0 = time.perf_counter()
        gp.ll_batch(plist)
        return (time.perf_counter() - t0) * 1e3

    def singles():
        t0 = time.perf_counter()
        for p in plist:
            gp.update_hyperparameters(p)
        return (time.perf_counter() - t0) * 1e3
    print("64 parameter rows at N %d: ll_batch %.2f ms, 64 single evaluations %.2f ms" % (N, med(batch, 7, 2), med(singles, 7, 2)))


builder_and_fit()
warp_points_alone()
user_gain()
