"""The input sets and the host's yardstick of the sparse-GP tests (tests/test_sparse_host.py, tests/test_gpu_sparse.py).

Not a test module.  Everything here is numpy / LAPACK on covariance blocks from the CPU oracle's builder: the dense
N(0, Q_ff + Lambda) log-density and predictive on one side, the Woodbury form (the formulas of DESIGN.md section 18) on the other.
The two are the host's two routes to every compared figure; their discrepancy at a case's inputs, measured on the CPU, is that
case's entry of HOST_ERR, and a device figure is held to ten times it (the ten covers the device's other summation order), as in
tests/test_gpu_loo.py.  As there (three_figures: the largest of the three; HOST_CLOSED_ERR: the largest over the sizes), the figure
that bounds is the largest of a GROUP at one input set: ll and the four sums it is made of ("fit"), the VFE trace term ("trace":
k_i - q_i cancels and 1 / s_i = 100 amplifies it, a scale of its own), the predictions ("pred"), each over the methods that input
set is fitted with.  One figure of one method is one draw of a rounding error whose scale is cond(K_uu + jitter I) u: vfe and dtc
at the SAME matrices measure 9.2e-14 and 1.9e-14 in ll, c.c 5.3e-14 ... 5.5e-13 across the cases; the largest of a group
estimates the scale, a single draw does not.  The dense route forms (K_uu + jitter I)^-1 K_uf by LU, not from the Woodbury route's
Cholesky factor (see dense()).

Where the two routes are nearly ONE piece of arithmetic the discrepancy says nothing about a device that evaluates exp, log and
the reciprocal square root itself and adds in another order: sum log Lambda_i and r^T Lambda^-1 r for vfe / dtc (Lambda_i = s_i on
either route; they differ only as numpy's pairwise sum differs from the exactly rounded math.fsum: ~1e-16), and every figure of the
M = 1 case (cond = 1: 2e-16 ... 8e-15).  No bound is therefore taken below FLOOR(N) = 2 N u, u = 2^-53: the worst-case forward error
gamma_N = N u of ONE inner product of length N relative to the sum of its terms' sizes, doubled because every figure passes through
two such stages (the Gram over the N rows, then the factorisation and solves).  It is a statement about the number format, not about
the code under test: 1.4e-14 at N = 64, 6.7e-14 at N = 300, 2.4e-13 at N = 1100 -- below ten times the host's discrepancy wherever
the two routes are independent.
"""
import math

import numpy as np
import scipy.linalg

FIGURES = ("ll", "sum_log_lambda", "sum_log_diag_LB", "r_lambda_r", "c_c", "trace", "mean", "std", "cov", "mean_noise", "std_noise",
           "cov_noise")


def floor(N):
    return 2.0 * N * 2.0 ** -53


def inputs(N, d, nder=60, seed=31):
    """The inputs of tests/test_gpu_loo.py: seeded, any size."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, d)
    n = np.zeros((N, d), dtype=int)
    if nder:
        n[-nder:, 0] = 1
    y = np.sin(3 * X.sum(1)) + 0.05 * rs.randn(N)
    return X, n, y


SE2 = [1.1, 0.4, 0.6]
NOISE = 0.1

#: name -> model (terms: (oracle kernel, params) or (kernel 1, params 1, kernel 2, params 2) for a product), d, N, derivative rows,
#: M, order-1 inducing rows, methods, chunk_rows (None: the default), heteroscedastic err_y, optionally nstar (test points: NSTAR)
CASES = {
    "se_300": dict(terms=[("se", SE2)], d=2, N=300, nder=60, M=40, zder=0, methods=("fitc", "vfe", "dtc"), chunks=(None, 128), het=False),
    "sum_prod_1100": dict(terms=[("se", SE2), ("m52", [0.7, 0.9, 1.3], "se", [1.0, 1.5, 0.8])], d=2, N=1100, nder=60, M=70, zder=0,
                          methods=("fitc",), chunks=(256,), het=True),
    "rq_257": dict(terms=[("rq", [1.0, 1.7, 0.4])], d=1, N=257, nder=0, M=33, zder=4, methods=("vfe",), chunks=(64,), het=False),
    "se3_130": dict(terms=[("se", [1.1, 0.4, 0.6, 0.9])], d=3, N=130, nder=0, M=129, zder=0, methods=("fitc",), chunks=(64,), het=False),
    "se1_64": dict(terms=[("se", [1.1, 0.35])], d=1, N=64, nder=0, M=1, zder=0, methods=("fitc",), chunks=(None,), het=False),
    # M at the edges of the padded orders (MPU = M to 128, BP = LDV = M + 1 to 128, MG = M + 1 to 64) and past the 256-thread stride of
    # the row kernels: 63 / 127 put the r~ column in the last column of the last Gram tile (127: BP = MPU), 64 / 128 give the
    # augmented row a tile / a 128-block of its own (128: MPU < BP), 257 / 300 / 520 run the two-wide loop of sparse_lambda_kernel
    # without / with a remainder pass / with a remainder pass that starts past 512.  sum_m257 is fitted with two methods because one
    # method is one draw (module docstring).  With vfe alone the two routes measured 3.5e-13 apart in ll on one CPU and 7.2e-12
    # apart on another (same numpy, another BLAS code path; ll = -611 stands behind r^T Lambda^-1 r - c.c = 15778 - 13826, and the
    # dense route's c.c moved).  Against the Woodbury sums in numpy.longdouble: Woodbury 1.6e-12 on both CPUs, dense 1.9e-12 on
    # the first and 5.6e-12 on the second, the device 1.3e-12.  fitc at the same matrices measures 5.0e-12, the scale of that error
    "se_m63": dict(terms=[("se", SE2)], d=2, N=130, nder=20, M=63, zder=0, methods=("fitc", "vfe"), chunks=(64,), het=False),
    "se_m64": dict(terms=[("se", SE2)], d=2, N=130, nder=20, M=64, zder=0, methods=("fitc",), chunks=(64,), het=False),
    "se_m127": dict(terms=[("se", [1.1, 0.2, 0.3])], d=2, N=200, nder=20, M=127, zder=0, methods=("fitc", "vfe"), chunks=(64,), het=True,
                    nstar=150),
    "se_m128": dict(terms=[("se", [1.1, 0.2, 0.3])], d=2, N=200, nder=20, M=128, zder=0, methods=("fitc", "dtc"), chunks=(64,), het=True),
    "m52_m300": dict(terms=[("m52", [1.0, 0.3, 0.4])], d=2, N=700, nder=60, M=300, zder=4, methods=("fitc", "vfe"), chunks=(256,), het=True),
    "sum_m257": dict(terms=[("se", [1.1, 0.2, 0.25]), ("m52", [0.7, 0.9, 1.3], "se", [1.0, 1.5, 0.8])], d=2, N=400, nder=40, M=257, zder=0,
                     methods=("fitc", "vfe"), chunks=(128,), het=True),
    "m52_m520": dict(terms=[("m52", [1.0, 0.8, 0.8, 0.8])], d=3, N=900, nder=60, M=520, zder=0, methods=("fitc", "vfe"), chunks=(None,),
                     het=False),
}
JITTER = 1e-6
NSTAR, NSTAR_DER = 50, 4


def case_data(name):
    """X, n, y, err_y, Z, n_Z, Xs, ns of a case: seeded."""
    c = CASES[name]
    X, n, y = inputs(c["N"], c["d"], nder=c["nder"])
    rs = np.random.RandomState(97)
    Z = rs.rand(c["M"], c["d"])
    nZ = np.zeros((c["M"], c["d"]), dtype=int)
    if c["zder"]:
        nZ[-c["zder"]:, 0] = 1
    nstar = c.get("nstar", NSTAR)
    Xs = rs.rand(nstar, c["d"])
    ns = np.zeros((nstar, c["d"]), dtype=int)
    ns[-NSTAR_DER:, 0] = 1
    err_y = 0.02 + 0.05 * rs.rand(c["N"]) if c["het"] else np.full(c["N"], 0.02)
    return dict(X=X, n=n, y=y, err_y=err_y, Z=Z, nZ=nZ, Xs=Xs, ns=ns)


# ---- covariance blocks from the CPU oracle ---------------------------------------------------------------------------------------
def _leibniz_product(O, k1, p1, k2, p2, Xi, ni, Xj, nj):
    """K of the product k1 * k2 for points whose derivative orders are 0, or 1 in ONE coordinate: the general Leibniz rule over which
    factor takes each point's derivative (a point of order 0 has one split, counted once)."""
    ni, nj = np.asarray(ni), np.asarray(nj)
    assert ni.sum(1).max() <= 1 and nj.sum(1).max() <= 1
    out = np.zeros((len(Xi), len(Xj)))
    for a in (0, 1):                     # a = 1: the first factor takes the row point's derivative
        wi = np.where(ni.sum(1) > 0, 1.0, 1.0 - a)
        for b in (0, 1):
            wj = np.where(nj.sum(1) > 0, 1.0, 1.0 - b)
            T = O.kbuild(k1, p1, Xi, ni * a, Xj, nj * b) * O.kbuild(k2, p2, Xi, ni * (1 - a), Xj, nj * (1 - b))
            out += wi[:, None] * T * wj[None, :]
    return out


def gram(O, terms, Xi, ni, Xj, nj):
    out = 0.0
    for t in terms:
        out = out + (_leibniz_product(O, t[0], t[1], t[2], t[3], Xi, ni, Xj, nj) if len(t) == 4 else O.kbuild(t[0], t[1], Xi, ni, Xj, nj))
    return out


def kdiag(O, terms, X, n):
    """k(x_i, x_i), point by point (never the N x N matrix)."""
    return np.array([gram(O, terms, X[i:i + 1], n[i:i + 1], X[i:i + 1], n[i:i + 1])[0, 0] for i in range(len(X))])


def blocks(O, name):
    c, d = CASES[name], case_data(name)
    t = c["terms"]
    return dict(Kuu=gram(O, t, d["Z"], d["nZ"], d["Z"], d["nZ"]), Kuf=gram(O, t, d["Z"], d["nZ"], d["X"], d["n"]),
                kd=kdiag(O, t, d["X"], d["n"]), Kus=gram(O, t, d["Z"], d["nZ"], d["Xs"], d["ns"]),
                Kss=gram(O, t, d["Xs"], d["ns"], d["Xs"], d["ns"]))


def noise_block(ns, noise_n, sigma):
    """The DiagonalNoiseKernel term of k(X*, X*): sigma^2 on the diagonal where a row's orders equal noise_n."""
    hit = np.all(np.asarray(ns) == np.asarray(noise_n)[None, :], axis=1)
    return np.diag(np.where(hit, sigma ** 2.0, 0.0))


# ---- the two host routes ------------------------------------------------------------------------------------------------------------
def woodbury(b, r, s, method, jitter=JITTER):
    M = b["Kuu"].shape[0]
    Lu = scipy.linalg.cholesky(b["Kuu"] + jitter * np.eye(M), lower=True)
    V = scipy.linalg.solve_triangular(Lu, b["Kuf"], lower=True)
    kmq = b["kd"] - (V ** 2).sum(0)
    lam = kmq + s if method == "fitc" else s.copy()
    B = np.eye(M) + (V / lam).dot(V.T)
    LB = scipy.linalg.cholesky(B, lower=True)
    c = scipy.linalg.solve_triangular(LB, V.dot(r / lam), lower=True)
    parts = np.array([np.log(lam).sum(), np.log(np.diag(LB)).sum(), r.dot(r / lam), c.dot(c),
                      (kmq / s).sum() if method == "vfe" else 0.0])
    ll = -0.5 * (parts[0] + 2.0 * parts[1] + parts[2] - parts[3] + len(r) * math.log(2.0 * math.pi)) - 0.5 * parts[4]
    v = scipy.linalg.solve_triangular(Lu, b["Kus"], lower=True)
    w = scipy.linalg.solve_triangular(LB, v, lower=True)
    return dict(ll=ll, parts=parts, mean=w.T.dot(c), cov=b["Kss"] - v.T.dot(v) + w.T.dot(w), lam=lam,
                cond_uu=np.linalg.cond(b["Kuu"] + jitter * np.eye(M)), cond_B=np.linalg.cond(B))


def dense(b, r, s, method, jitter=JITTER):
    M, N = b["Kuf"].shape
    # (K_uu + jitter I)^-1 K_uf by LU with partial pivoting, NOT by the Cholesky factor the Woodbury route takes: with the same
    # LAPACK factor on both routes their difference would leave out the one error cond(K_uu + jitter I) amplifies, that of L_u
    # itself, which a device that factors K_uu in its own order does not share with either
    KiKuf = np.linalg.solve(b["Kuu"] + jitter * np.eye(M), b["Kuf"])
    Qff = b["Kuf"].T.dot(KiKuf)
    kmq = b["kd"] - np.diag(Qff)
    lam = kmq + s if method == "fitc" else s.copy()
    S = Qff + np.diag(lam)
    cS = scipy.linalg.cho_factor(S, lower=True)
    logdet = 2.0 * np.log(np.diag(cS[0])).sum()
    quad = r.dot(scipy.linalg.cho_solve(cS, r))
    trace = (kmq / s).sum() if method == "vfe" else 0.0
    ll = -0.5 * (logdet + quad + N * math.log(2.0 * math.pi)) - 0.5 * trace
    # the five sums by the dense route: the determinant lemma log det S = sum log Lambda + log det B, and the quadratic form
    # r^T S^-1 r = r^T Lambda^-1 r - c.c; the two plain sums with the exactly rounded math.fsum
    p0 = math.fsum(np.log(lam))
    p2 = math.fsum(r * r / lam)
    parts = np.array([p0, 0.5 * (logdet - p0), p2, p2 - quad, trace])
    Qsf = b["Kus"].T.dot(KiKuf)
    return dict(ll=ll, parts=parts, mean=Qsf.dot(scipy.linalg.cho_solve(cS, r)),
                cov=b["Kss"] - Qsf.dot(scipy.linalg.cho_solve(cS, Qsf.T)))


def figures(got, ref, y):
    """The compared figures of (ll, parts, mean, std, cov) tuples ``got`` against ``ref``, each relative to its natural scale:
    ll to |ll|, a part to its own size, means to max|y|, standard deviations to their largest, covariance entries to the largest
    diagonal entry."""
    out = {"ll": abs(got["ll"] - ref["ll"]) / abs(ref["ll"])}
    for i, name in enumerate(FIGURES[1:6]):
        out[name] = abs(got["parts"][i] - ref["parts"][i]) / abs(ref["parts"][i]) if ref["parts"][i] != 0.0 else abs(got["parts"][i])
    for suffix in ("", "_noise"):
        if "mean" + suffix not in got:
            continue
        out["mean" + suffix] = np.abs(got["mean" + suffix] - ref["mean" + suffix]).max() / np.abs(y).max()
        out["std" + suffix] = np.abs(got["std" + suffix] - ref["std" + suffix]).max() / ref["std" + suffix].max()
        out["cov" + suffix] = np.abs(got["cov" + suffix] - ref["cov" + suffix]).max() / np.diag(ref["cov" + suffix]).max()
    return out


def host_routes(O, name, method):
    """(woodbury, dense) of a case, each with mean / std / cov without and with the noise term (noise orders: all zero)."""
    c, d = CASES[name], case_data(name)
    b = blocks(O, name)
    s = NOISE ** 2.0 + d["err_y"] ** 2.0
    nb = noise_block(d["ns"], np.zeros(c["d"], dtype=int), NOISE)
    out = []
    for route in (woodbury, dense):
        res = route(b, d["y"], s, method)
        res["std"] = np.sqrt(np.diag(res["cov"]))
        res["mean_noise"], res["cov_noise"] = res["mean"], res["cov"] + nb
        res["std_noise"] = np.sqrt(np.diag(res["cov_noise"]))
        out.append(res)
    return out[0], out[1]


GROUPS = {"fit": ("ll", "sum_log_lambda", "sum_log_diag_LB", "r_lambda_r", "c_c"), "trace": ("trace",),
          "pred": ("mean", "std", "cov", "mean_noise", "std_noise", "cov_noise")}


def host_err(name, figure):
    """The host's discrepancy that bounds ``figure`` at the input set ``name``: the largest over the figures of its group and over
    the methods the input set is fitted with (module docstring)."""
    group = [g for g in GROUPS.values() if figure in g][0]
    return max(HOST_ERR[(name, m)][f] for m in CASES[name]["methods"] for f in group)


def bound(name, method, figure, N):
    """What a device figure may differ from the host's by: ten times the host's own discrepancy, never below the floor of the module
    docstring."""
    return max(10.0 * host_err(name, figure), floor(N))


#: the host's discrepancy Woodbury - dense per case, method and figure, measured on the CPU by tests/test_sparse_host.py (which prints
#: this table and asserts every entry <= 1e-10); cond(K_uu + jitter I) and cond(B) beside each
HOST_ERR = {
    ("se_300", "fitc"): {   # cond(K_uu + jitter I) = 2.8e+07, cond(B) = 2.2e+04
        "ll": 4.86e-13, "sum_log_lambda": 7.22e-14, "sum_log_diag_LB": 1.56e-13, "r_lambda_r": 2.01e-13, "c_c": 5.28e-14, "trace": 0, "mean": 1.31e-11, "std": 1e-11, "cov": 1.83e-11, "mean_noise": 1.31e-11, "std_noise": 4.96e-12, "cov_noise": 4.5e-12},
    ("se_300", "vfe"): {   # cond(K_uu + jitter I) = 2.8e+07, cond(B) = 2.5e+04
        "ll": 9.2e-14, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 4.31e-14, "r_lambda_r": 4.01e-16, "c_c": 9.88e-15, "trace": 1.4e-11, "mean": 1.25e-11, "std": 9.87e-12, "cov": 1.82e-11, "mean_noise": 1.25e-11, "std_noise": 4.82e-12, "cov_noise": 4.32e-12},
    ("se_300", "dtc"): {   # cond(K_uu + jitter I) = 2.8e+07, cond(B) = 2.5e+04
        "ll": 1.88e-14, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 4.31e-14, "r_lambda_r": 4.01e-16, "c_c": 9.88e-15, "trace": 0, "mean": 1.25e-11, "std": 9.87e-12, "cov": 1.82e-11, "mean_noise": 1.25e-11, "std_noise": 4.82e-12, "cov_noise": 4.32e-12},
    ("sum_prod_1100", "fitc"): {   # cond(K_uu + jitter I) = 7.2e+07, cond(B) = 9.2e+04
        "ll": 3.45e-12, "sum_log_lambda": 1.28e-14, "sum_log_diag_LB": 1.45e-13, "r_lambda_r": 1.21e-13, "c_c": 5.45e-13, "trace": 0, "mean": 7.83e-11, "std": 2.51e-12, "cov": 1.73e-12, "mean_noise": 7.83e-11, "std_noise": 2.51e-12, "cov_noise": 1.73e-12},
    ("rq_257", "vfe"): {   # cond(K_uu + jitter I) = 2.4e+07, cond(B) = 1.8e+04
        "ll": 8.58e-15, "sum_log_lambda": 1.94e-16, "sum_log_diag_LB": 1.28e-14, "r_lambda_r": 0, "c_c": 1.47e-15, "trace": 8.13e-11, "mean": 3.36e-13, "std": 8.52e-12, "cov": 1.7e-11, "mean_noise": 3.36e-13, "std_noise": 8.52e-12, "cov_noise": 1.7e-11},
    ("se3_130", "fitc"): {   # cond(K_uu + jitter I) = 8.3e+07, cond(B) = 8.2e+03
        "ll": 9.4e-14, "sum_log_lambda": 1.17e-14, "sum_log_diag_LB": 3.02e-14, "r_lambda_r": 5.38e-14, "c_c": 5.28e-14, "trace": 0, "mean": 5.71e-13, "std": 2.31e-13, "cov": 1.89e-13, "mean_noise": 5.71e-13, "std_noise": 1.95e-13, "cov_noise": 1.89e-13},
    ("se1_64", "fitc"): {   # cond(K_uu + jitter I) = 1.0e+00, cond(B) = 1.0e+00
        "ll": 1.42e-15, "sum_log_lambda": 2.1e-15, "sum_log_diag_LB": 2.7e-15, "r_lambda_r": 1.25e-14, "c_c": 1.48e-14, "trace": 0, "mean": 7.14e-15, "std": 4.19e-16, "cov": 1.83e-16, "mean_noise": 7.14e-15, "std_noise": 3.83e-16, "cov_noise": 1.83e-16},
    ("se_m63", "fitc"): {   # cond(K_uu + jitter I) = 4.4e+07, cond(B) = 1.1e+04
        "ll": 7.89e-14, "sum_log_lambda": 5.02e-14, "sum_log_diag_LB": 7.25e-14, "r_lambda_r": 2.66e-13, "c_c": 3.33e-13, "trace": 0, "mean": 1.09e-11, "std": 3.99e-12, "cov": 7.69e-12, "mean_noise": 1.09e-11, "std_noise": 3.99e-12, "cov_noise": 7.69e-12},
    ("se_m63", "vfe"): {   # cond(K_uu + jitter I) = 4.4e+07, cond(B) = 1.1e+04
        "ll": 6.73e-14, "sum_log_lambda": 0, "sum_log_diag_LB": 1.46e-13, "r_lambda_r": 1.51e-16, "c_c": 1.84e-15, "trace": 1.21e-11, "mean": 8.85e-12, "std": 5.27e-12, "cov": 9.92e-12, "mean_noise": 8.85e-12, "std_noise": 5.27e-12, "cov_noise": 9.92e-12},
    ("se_m64", "fitc"): {   # cond(K_uu + jitter I) = 4.5e+07, cond(B) = 1.1e+04
        "ll": 3.53e-13, "sum_log_lambda": 7.4e-14, "sum_log_diag_LB": 1.39e-13, "r_lambda_r": 2.23e-13, "c_c": 2.07e-13, "trace": 0, "mean": 1.11e-11, "std": 3.18e-12, "cov": 6.12e-12, "mean_noise": 1.11e-11, "std_noise": 3.18e-12, "cov_noise": 6.12e-12},
    ("se_m127", "fitc"): {   # cond(K_uu + jitter I) = 4.1e+07, cond(B) = 1.6e+04
        "ll": 6.07e-13, "sum_log_lambda": 2.02e-13, "sum_log_diag_LB": 5.36e-13, "r_lambda_r": 1.02e-13, "c_c": 1.24e-13, "trace": 0, "mean": 9.09e-12, "std": 6.96e-13, "cov": 1.62e-12, "mean_noise": 9.09e-12, "std_noise": 6.96e-13, "cov_noise": 1.62e-12},
    ("se_m127", "vfe"): {   # cond(K_uu + jitter I) = 4.1e+07, cond(B) = 1.7e+04
        "ll": 1.58e-11, "sum_log_lambda": 0, "sum_log_diag_LB": 5.81e-15, "r_lambda_r": 1.16e-16, "c_c": 4.76e-14, "trace": 7.29e-11, "mean": 6.43e-12, "std": 2.96e-12, "cov": 5.92e-12, "mean_noise": 6.43e-12, "std_noise": 2.96e-12, "cov_noise": 5.92e-12},
    ("se_m128", "fitc"): {   # cond(K_uu + jitter I) = 4.1e+07, cond(B) = 1.6e+04
        "ll": 1.2e-12, "sum_log_lambda": 1.12e-13, "sum_log_diag_LB": 8.85e-14, "r_lambda_r": 2.96e-13, "c_c": 3.58e-13, "trace": 0, "mean": 8.13e-12, "std": 5.22e-12, "cov": 2.97e-12, "mean_noise": 8.13e-12, "std_noise": 5.22e-12, "cov_noise": 2.97e-12},
    ("se_m128", "dtc"): {   # cond(K_uu + jitter I) = 4.1e+07, cond(B) = 1.7e+04
        "ll": 2.45e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 1.58e-13, "r_lambda_r": 1.16e-16, "c_c": 9.2e-14, "trace": 0, "mean": 5.88e-12, "std": 4.51e-12, "cov": 2.79e-12, "mean_noise": 5.88e-12, "std_noise": 4.51e-12, "cov_noise": 2.79e-12},
    ("m52_m300", "fitc"): {   # cond(K_uu + jitter I) = 9.6e+07, cond(B) = 2.0e+04
        "ll": 5.14e-13, "sum_log_lambda": 1.29e-14, "sum_log_diag_LB": 2.41e-13, "r_lambda_r": 4.98e-14, "c_c": 3.8e-14, "trace": 0, "mean": 2.82e-11, "std": 1.25e-12, "cov": 2.36e-12, "mean_noise": 2.82e-11, "std_noise": 1.25e-12, "cov_noise": 2.36e-12},
    ("m52_m300", "vfe"): {   # cond(K_uu + jitter I) = 9.6e+07, cond(B) = 2.5e+04
        "ll": 7.74e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 1.08e-13, "r_lambda_r": 1.32e-16, "c_c": 4.5e-14, "trace": 1.26e-12, "mean": 4.21e-11, "std": 1.78e-12, "cov": 3.39e-12, "mean_noise": 4.21e-11, "std_noise": 1.78e-12, "cov_noise": 3.39e-12},
    ("sum_m257", "fitc"): {   # cond(K_uu + jitter I) = 1.6e+08, cond(B) = 2.4e+04
        "ll": 5.02e-12, "sum_log_lambda": 1.66e-13, "sum_log_diag_LB": 7.34e-13, "r_lambda_r": 6.5e-13, "c_c": 2.99e-13, "trace": 0, "mean": 6.38e-11, "std": 1.31e-11, "cov": 2.62e-11, "mean_noise": 6.38e-11, "std_noise": 1.31e-11, "cov_noise": 2.62e-11},
    ("sum_m257", "vfe"): {   # cond(K_uu + jitter I) = 1.6e+08, cond(B) = 2.5e+04
        "ll": 3.5e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 1.16e-13, "r_lambda_r": 0, "c_c": 5.51e-14, "trace": 8.4e-11, "mean": 5.49e-11, "std": 1.56e-11, "cov": 3.11e-11, "mean_noise": 5.49e-11, "std_noise": 1.56e-11, "cov_noise": 3.11e-11},
    ("m52_m520", "fitc"): {   # cond(K_uu + jitter I) = 1.9e+08, cond(B) = 5.1e+04
        "ll": 1.06e-12, "sum_log_lambda": 8.1e-15, "sum_log_diag_LB": 1.36e-13, "r_lambda_r": 1.69e-14, "c_c": 5.78e-14, "trace": 0, "mean": 1.94e-11, "std": 2.02e-12, "cov": 3.52e-12, "mean_noise": 1.94e-11, "std_noise": 2.02e-12, "cov_noise": 3.52e-12},
    ("m52_m520", "vfe"): {   # cond(K_uu + jitter I) = 1.9e+08, cond(B) = 5.2e+04
        "ll": 9.01e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 7.32e-14, "r_lambda_r": 0, "c_c": 5.6e-14, "trace": 1.89e-12, "mean": 1.75e-11, "std": 2.57e-12, "cov": 4.53e-12, "mean_noise": 1.75e-11, "std_noise": 2.57e-12, "cov_noise": 4.53e-12},
}
