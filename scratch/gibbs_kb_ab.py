"""Gibbs-tanh against the 1-D squared-exponential kernel on the same points:
  (1) the fused builder alone (gpt_dev_kbuild, lower triangle + fused diagonal), HIP events on the context's stream, value-only
      rows and rows with the last quarter at n = 1, N in {4096, 8192, 16384};
  (2) gpt_fit at N = 8192 (value rows and last quarter n = 1), the context's per-phase events ("timing" option, total).
Warm-up first; then the two kernels alternate, REPS times each, in one process; min / median / max over the repeats.
python scratch/gibbs_kb_ab.py [reps] > profiles/gibbs_kb_ab.txt"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/scratch/", 1)[0])
from gptools_amd import _lib      # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
KERNELS = (("se", _lib.KERNEL_SE, np.array([1.0, 0.3])),
           ("gibbs", _lib.KERNEL_GIBBS_TANH, np.array([1.0, 0.5, 0.1, 0.05, 0.5])))
lib = _lib.load()
ctx = _lib.Context(0)
st = torch.cuda.ExternalStream(int(ctx.stream))


def stats(v):
    v = np.asarray(v)
    return "min %.4f  med %.4f  max %.4f ms" % (v.min(), np.median(v), v.max())


def points(N, deriv):
    rs = np.random.RandomState(N)
    X = np.sort(rs.rand(N))[:, None]
    n = np.zeros((N, 1), dtype=np.int32)
    if deriv == "quarter":
        n[3 * N // 4:] = 1
    return X, n


print("# (1) builder alone: lower triangle, fused diagonal, D = 1; %d alternating repeats after 3 warm-up calls" % REPS)
for N in (4096, 8192, 16384):
    for deriv in ("none", "quarter"):
        X, n = points(N, deriv)
        err = 0.05 * np.ones(N)
        with torch.cuda.stream(st):
            dX = torch.from_numpy(X).cuda()
            dn = torch.from_numpy(n).cuda()
            de = torch.from_numpy(err).cuda()
            dK = torch.empty((N, N), dtype=torch.float64, device="cuda")
            times = {k[0]: [] for k in KERNELS}

            def run(kid, params):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                _lib.check(lib.gpt_dev_kbuild(ctx.handle, kid, _lib.dptr(params), len(params), dX.data_ptr(), dn.data_ptr(), N,
                                              dX.data_ptr(), dn.data_ptr(), N, 1, -1, 1, None, 1, 0, 0, de.data_ptr(), 0.0,
                                              2.2e-14, dK.data_ptr(), N))
                e1.record(st)
                st.synchronize()
                return e0.elapsed_time(e1)
            for _ in range(3):
                for name, kid, params in KERNELS:
                    run(kid, params)
            for _ in range(REPS):
                for name, kid, params in KERNELS:
                    times[name].append(run(kid, params))
        ratio = np.median(times["gibbs"]) / np.median(times["se"])
        for name in times:
            print("N=%5d deriv=%-7s %-5s %s" % (N, deriv, name, stats(times[name])))
        print("N=%5d deriv=%-7s gibbs / se (medians) = %.3f" % (N, deriv, ratio))
        del dK
        torch.cuda.empty_cache()

print("# (2) gpt_fit, N = 8192, D = 1: total of the context's events (upload of y, build, factorisation, tail)")
ctx.set_option("timing", 1)
for deriv in ("none", "quarter"):
    N = 8192
    X, n = points(N, deriv)
    rs = np.random.RandomState(1)
    y = np.sin(6.0 * X[:, 0]) + 0.05 * rs.randn(N)
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    times = {k[0]: [] for k in KERNELS}
    kb = {k[0]: [] for k in KERNELS}
    for rep in range(3 + REPS):
        for name, kid, params in KERNELS:
            ctx.fit(kid, params, 0.0, y, err, 2.2e-14)
            t = ctx.last_timings()
            if rep >= 3:
                times[name].append(t["total"])
                kb[name].append(t["kbuild"])
    for name in times:
        print("fit N=8192 deriv=%-7s %-5s total %s | build med %.4f ms" % (deriv, name, stats(times[name]), np.median(kb[name])))
    print("fit N=8192 deriv=%-7s gibbs / se (median totals) = %.4f" % (deriv, np.median(times["gibbs"]) / np.median(times["se"])))
ctx.close()
