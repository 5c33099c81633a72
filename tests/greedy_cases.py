"""The cases and the host's yardstick of the greedy inducing-input selection (tests/test_greedy_host.py, tests/test_gpu_greedy.py).

Not a test module.  The yardstick is the loop of DESIGN.md section 18.10 in numpy on covariance blocks from the CPU oracle's builder
(sparse_cases.gram; the one Gibbs case from the package's host evaluation of the same kernel class), run in float64 and in
numpy.longdouble on the SAME float64 blocks:

    d_i = k(x_i, x_i);  for j = 0 .. M-1:  p_j = the unselected candidate with the largest d_i (ties: the lowest row), dmax_j = d_{p_j};
    stop (count = j) if j > 0 and dmax_j <= tol dmax_0, or if dmax_j is not a positive finite number;
    l_i = (k(x_i, x_p) - sum_{t<j} L[i,t] L[p,t]) / sqrt(dmax_j) for EVERY candidate;  L[i,j] = l_i;  d_i -= l_i^2;  p_j is marked;
    trace_{j+1} = sum over the unselected of max(d_i, 0)   (trace_0 = sum d_i)

What entitles the device test to demand the float64 pivots entry for entry is the GAP condition test_greedy_host.py asserts: at every
step j >= 1 (j = 0 too where k(x, x) varies) the largest and the second-largest residual differ by at least GAP_MIN max k_ii = 1e-10,
about 1e6 u, where a residual's own rounding is at most about (j + 2) u max k_ii (6e-14 at j = 520); and the float64 and longdouble
pivot sequences are the same.  HOST_ERR: |dmax, trace (float64) - (longdouble)| in units of max k_ii, the largest over the steps; the
device's figures are held to ten times it (the ten covers the device's other summation order: tests/sparse_cases.py), never below
(j + 2) u for dmax_j and N (j + 2) u for trace_j -- the number format's bound for an inner product of j terms plus the two
roundings of the step, N of them added up.  TRACE_ERR: |trace_M - tr(K_ff - K_fu K_uu^-1 K_uf)|, the latter by LU on the selected rows,
same units.
"""
import numpy as np

import sparse_cases as S

U = 2.0 ** -53
GAP_MIN = 1e-10
M52 = [1.0, 0.3, 0.4]
# sigma_f, l_1, l_2, l_w, x_0 of GibbsKernel1dTanh: a long length scale left of x_0 = 0.35, a short one right of it.  The long side keeps every
# pair of points correlated (no residual stays at sigma_f^2 to the last bit while pivots are chosen elsewhere: with short scales
# throughout, exp underflows for distant pairs and the untouched rows tie exactly), the short side keeps 33 pivots above rounding
GIBBS = [1.1, 0.45, 0.025, 0.06, 0.35]

#: name -> terms (sparse_cases' form; "gibbs_tanh": GibbsKernel1dTanh), d, N, derivative rows (the last nder rows, order 1 in coordinate 0), M
CASES = {
    "m52_m63": dict(terms=[("m52", M52)], d=2, N=130, nder=0, M=63),
    "m52_m64": dict(terms=[("m52", M52)], d=2, N=130, nder=0, M=64),
    "m52_m127": dict(terms=[("m52", M52)], d=2, N=200, nder=0, M=127),
    "m52_m128": dict(terms=[("m52", M52)], d=2, N=200, nder=0, M=128),
    "m52_m257": dict(terms=[("m52", M52)], d=2, N=400, nder=0, M=257),
    "m52_m300": dict(terms=[("m52", M52)], d=2, N=700, nder=0, M=300),
    "m52_m520": dict(terms=[("m52", [1.0, 0.8, 0.8, 0.8])], d=3, N=900, nder=0, M=520),
    "se_40": dict(terms=S.CASES["se_300"]["terms"], d=2, N=300, nder=0, M=40),
    "sum_prod_70": dict(terms=S.CASES["sum_prod_1100"]["terms"], d=2, N=1100, nder=0, M=70),
    "gibbs_33": dict(terms=[("gibbs_tanh", GIBBS)], d=1, N=257, nder=0, M=33),
    # the one case with derivative rows: they are no candidates
    "m52_der": dict(terms=[("m52", M52)], d=2, N=130, nder=20, M=63),
}
#: k(x, x) is the same for every x: step 0 is a complete tie and the first pivot the lowest candidate.  That holds for the Gibbs case
#: too -- the kernel is not stationary, its VARIANCE is: k(x, x) = sigma_f^2 sqrt(2 l l / (l^2 + l^2)) = sigma_f^2 whatever l(x) is, and
#: the host's blocks give it the same bits in every row (test_greedy_host.py asserts that).  No kernel the library evaluates itself has a
#: k(x, x) that varies over value rows, so there is no case whose step 0 is decided by a gap
STATIONARY = {name: True for name in CASES}


def case_points(name):
    """X, n of a case (sparse_cases.inputs: seeded)."""
    c = CASES[name]
    X, n, _ = S.inputs(c["N"], c["d"], nder=c["nder"])
    return X, n


def plain_rows(n):
    return np.flatnonzero(np.all(np.asarray(n) == 0, axis=1))


def gram(O, terms, X):
    """K(X, X) at derivative orders zero, float64: the oracle's blocks; a Gibbs-tanh term by the package's host class."""
    z = np.zeros(X.shape, dtype=int)
    out = 0.0
    for t in terms:
        if t[0] == "gibbs_tanh":
            from gptools_amd.kernel.gibbs import GibbsKernel1d, tanh_warp
            k = GibbsKernel1d(tanh_warp, num_params=5, initial_params=t[1])
            ii, jj = np.meshgrid(np.arange(len(X)), np.arange(len(X)), indexing="ij")
            out = out + np.asarray(k(X[ii.ravel()], X[jj.ravel()], z[ii.ravel()], z[jj.ravel()]), dtype=float).reshape(len(X), len(X))
        else:
            out = out + S.gram(O, [t], X, z, X, z)
    return out


def yardstick(K, M, tol=0.0, dtype=np.float64):
    """The loop of the module docstring on the candidates' covariance matrix ``K`` (float64) in ``dtype``: dict of ``idx`` (positions
    among the candidates), ``dmax``, ``trace`` (count + 1), ``count`` and ``gap`` (per step: largest minus second-largest residual among the
    unselected, in units of max k_ii; inf where one candidate is left)."""
    K = np.asarray(K, dtype=float).astype(dtype)
    n = K.shape[0]
    d = np.diag(K).copy()
    kmax = d.max()
    L = np.zeros((n, M), dtype=dtype)
    sel = np.zeros(n, dtype=bool)
    idx, dmax, trace, gap = [], [], [d.sum()], []
    for j in range(M):
        dm = np.where(sel, -np.inf, d)
        p = int(np.argmax(dm))                       # (the first of equal values: the lowest row)
        dj = dm[p]
        if (j > 0 and dj <= dtype(tol) * dmax[0]) or not (dj > 0 and np.isfinite(dj)):
            break
        rest = np.delete(dm, p)
        gap.append(float((dj - rest.max()) / kmax) if rest.size and np.isfinite(rest.max()) else np.inf)
        l = (K[:, p] - L[:, :j].dot(L[p, :j])) / np.sqrt(dj)
        L[:, j] = l
        d = d - l * l
        sel[p] = True
        idx.append(p)
        dmax.append(dj)
        trace.append(np.maximum(d[~sel], 0).sum())
    return dict(idx=np.array(idx, dtype=int), dmax=np.array(dmax, dtype=dtype), trace=np.array(trace, dtype=dtype), count=len(idx),
                gap=np.array(gap), kmax=float(kmax))


def nystrom_trace(K, rows):
    """tr(K - K[:, rows] K[rows, rows]^-1 K[rows, :]) by LU with partial pivoting."""
    Kfu = K[:, rows]
    return float(np.trace(K) - np.sum(Kfu * np.linalg.solve(K[np.ix_(rows, rows)], Kfu.T).T))


_cache = {}


def reference(O, name):
    """(K of the candidates, the candidates' rows, float64 yardstick, longdouble yardstick) of a case: computed once."""
    if name not in _cache:
        X, n = case_points(name)
        rows = plain_rows(n)
        K = gram(O, CASES[name]["terms"], X[rows])
        _cache[name] = (K, rows, yardstick(K, CASES[name]["M"]), yardstick(K, CASES[name]["M"], dtype=np.longdouble))
    return _cache[name]


def host_figures(y64, yld):
    """HOST_ERR of one case as measured: |dmax, trace (float64) - (longdouble)| / max k_ii, the largest over the steps."""
    e = max(np.abs(y64["dmax"].astype(np.longdouble) - yld["dmax"]).max(), np.abs(y64["trace"].astype(np.longdouble) - yld["trace"]).max())
    return float(e / yld["kmax"])


def dmax_bound(name, j):
    return max(10.0 * HOST_ERR[name], (j + 2) * U)


def trace_bound(name, j, ncand):
    return max(10.0 * HOST_ERR[name], ncand * (j + 2) * U)


# ---- test 5 of tests/test_gpu_greedy.py: the selection against random subsets (the m52_m127 inputs, M = 64) -----------------------------
CLASS_CASE, CLASS_M, CLASS_NOISE = "m52_m127", 64, 0.1
#: seeds of the random 64-row subsets (numpy RandomState(seed).choice(N, 64, replace=False)) at which the HOST shows the subset's
#: Nystrom trace at least twice the greedy one (test_greedy_host.py asserts it; a property of these inputs, not a theorem)
CLASS_SEEDS = (0, 1, 2, 3, 4)


def random_subset(N, M, seed):
    return np.sort(np.random.RandomState(seed).choice(N, M, replace=False))


#: measured on the CPU by tests/test_greedy_host.py, which prints both tables (units of max k_ii)
HOST_ERR = {
    "m52_m63": 7.05e-15, "m52_m64": 7.05e-15, "m52_m127": 3.33e-14, "m52_m128": 3.33e-14, "m52_m257": 7.18e-14, "m52_m300": 2.18e-14,
    "m52_m520": 1.06e-13, "se_40": 2.33e-14, "sum_prod_70": 3.82e-13, "gibbs_33": 2.99e-14, "m52_der": 1.35e-14,
}
TRACE_ERR = {
    "m52_m63": 6.52e-15, "m52_m64": 3.09e-14, "m52_m127": 1.63e-14, "m52_m128": 2.09e-14, "m52_m257": 8.58e-14, "m52_m300": 4.31e-14,
    "m52_m520": 8.36e-14, "se_40": 4.75e-14, "sum_prod_70": 2.86e-13, "gibbs_33": 2.41e-16, "m52_der": 7.55e-15,
}
#: the smallest gap per case as test_greedy_host.py measures it (from step 1; units of max k_ii), for the record: m52_m63 / m52_m64
#: 4.4e-6, m52_m127 / m52_m128 7.2e-7, m52_m257 4.5e-8, m52_m300 2.5e-9, m52_m520 6.6e-10, se_40 1.6e-8, sum_prod_70 2.0e-8,
#: gibbs_33 1.5e-5, m52_der 3.5e-6
