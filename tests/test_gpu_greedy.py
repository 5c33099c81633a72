"""GPU suite (-m gpu): greedy conditional-variance selection of the inducing inputs -- gpt_sparse_select_inducing
(api_sparse_select.inc, kgreedy.hip) through greedy_inducing / SparseGaussianProcess.select_inducing, and its two kernels alone on raw
pointers (gpt_dev_greedy_update, gpt_dev_greedy_pick).

Yardsticks.  (1) The kernels alone: small-integer data with dmax in {1, 4, 16}, so every product, sum and the division by sqrt(dmax)
is exact -- equal bits demanded.  (2) The whole call: the host loop of tests/greedy_cases.py; the pivots entry for entry (the gap
condition tests/test_greedy_host.py asserts entitles the test to that), dmax and trace against the longdouble loop within ten times
the host's own float64 - longdouble discrepancy, never below (j + 2) u / N (j + 2) u.  Each figure is printed before it is asserted.

Measured on the MI355X, the worst ratio |device - longdouble| / bound per case (dmax, trace): m52_m63 / m52_m64 0.024, 0.31;
m52_m127 / m52_m128 0.0061, 0.13; m52_m257 0.0015, 0.11; m52_m300 0.0061, 0.39; m52_m520 0.0012, 0.23; se_40 0.0038, 0.10;
sum_prod_70 0.00023, 0.022; m52_der 0.0092, 0.14; gibbs_33 0.0044, 0.15; the pivots equal the yardstick's in each of them."""
import warnings

import numpy as np
import pytest

import greedy_cases as G
import sparse_cases as S

pytestmark = pytest.mark.gpu

UNROLL = 16          # GREEDY_UNROLL of kgreedy.hip
WG = 256             # GPT_GREEDY_ROWS_PER_PART
IMAX = np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


@pytest.fixture(scope="module")
def ctx():
    from gptools_amd import _lib
    return _lib.Context()


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def partials(d, mark, rows):
    """The partials of the update kernel from the residuals, in numpy: (part (2 nparts), pidx)."""
    nparts = (rows + WG - 1) // WG
    part, pidx = np.zeros(2 * nparts), np.full(nparts, IMAX, dtype=np.int32)
    for b in range(nparts):
        i0, i1 = b * WG, min(rows, (b + 1) * WG)
        free = np.flatnonzero(mark[i0:i1] == 0) + i0
        part[b] = d[free].max() if free.size else -np.inf
        part[nparts + b] = np.maximum(d[free], 0.0).sum()
        if free.size:
            pidx[b] = free[d[free] == part[b]].min()
    return part, pidx


# ---- (1) the kernels alone, integer data, exact bits ---------------------------------------------------------------------------------
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]
JS = [0, 1, UNROLL - 1, UNROLL, UNROLL + 1, 2 * UNROLL - 1, 2 * UNROLL, 2 * UNROLL + 1, 257]


def update_case(ctx, rows, j, dmax, stop=0, force=None):
    """One gpt_dev_greedy_update on seeded small integers; ld > rows, two columns behind column j, a pivot row longer than j: all
    padding non-zero.  Returns what the device left and what numpy expects."""
    import torch
    rs = np.random.RandomState(1000 * rows + 7 * j + int(dmax))
    ld, ncol = rows + 37, j + 3
    L = rs.randint(-3, 4, size=(ncol, ld)).astype(float)              # row t of this array = column t of the factor
    L[L == 0.0] = 1.0
    prow = rs.randint(-3, 4, size=j + 5).astype(float)
    prow[prow == 0.0] = 2.0
    resid = rs.randint(-40, 400, size=ld).astype(float)
    mark = (rs.rand(ld) < 0.2).astype(np.int32)
    s = L[:j, :rows].T.dot(prow[:j])
    l = (L[j, :rows] - s) / np.sqrt(dmax)
    d = resid[:rows] - l * l
    if force == "selected_largest":                                  # the largest residual present sits on a selected row
        top = int(np.argmax(d))
        resid[top] += 1000.0
        d[top] += 1000.0
        mark[top] = 1
    elif force is not None:                                          # a tie between two given rows, above everything else
        for r in force:
            resid[r] += 5000.0 - d[r]
            mark[r] = 0
        d = resid[:rows] - l * l
    nparts = ctx.dev_greedy_parts(rows)
    assert nparts == (rows + WG - 1) // WG
    dL, dprow, dres, dmark = dev(L), dev(prow), dev(resid), dev(mark)
    dscal, dwords = dev(np.array([dmax, 99.0])), dev(np.array([stop, 0, 0, 0], dtype=np.int32))
    dpart, dpidx = dev(np.full(2 * nparts + 3, 123.0)), dev(np.full(nparts + 3, 77, dtype=np.int32))
    torch.cuda.synchronize()
    ctx.dev_greedy_update(dL.data_ptr(), ld, rows, j, dL.data_ptr() + 8 * j * ld, dres.data_ptr(), dmark.data_ptr(), dprow.data_ptr(),
                          dscal.data_ptr(), dwords.data_ptr(), dpart.data_ptr(), dpidx.data_ptr())
    ctx.synchronize()
    got = dict(L=dL.cpu().numpy(), resid=dres.cpu().numpy(), part=dpart.cpu().numpy(), pidx=dpidx.cpu().numpy(), mark=dmark.cpu().numpy())
    want_L, want_res = L.copy(), resid.copy()
    want_L[j, :rows] = l
    want_res[:rows] = d
    part, pidx = partials(d, mark, rows)
    return got, dict(L=want_L, resid=want_res, part=part, pidx=pidx, L0=L, resid0=resid, mark=mark, nparts=nparts, d=d)


def check_update(got, want):
    nparts = want["nparts"]
    assert np.array_equal(got["L"], want["L"])                       # l_i exactly; rows >= rows, the other columns untouched
    assert np.array_equal(got["resid"], want["resid"])
    assert np.array_equal(got["mark"], want["mark"])
    assert np.array_equal(got["part"][:2 * nparts], want["part"]) and np.all(got["part"][2 * nparts:] == 123.0)
    assert np.array_equal(got["pidx"][:nparts], want["pidx"]) and np.all(got["pidx"][nparts:] == 77)


@pytest.mark.parametrize("rows", ROWS)
def test_update_kernel_exact(ctx, rows):
    for j in JS:
        for dmax in (1.0, 4.0, 16.0):
            got, want = update_case(ctx, rows, j, dmax)
            check_update(got, want)
    print("rows %d: l_i, d_i and the partials equal numpy's bits at j = %s, dmax 1, 4, 16" % (rows, JS))


def test_update_kernel_excludes_selected_rows_by_their_mark(ctx):
    for rows in (65, 257, 1025):
        got, want = update_case(ctx, rows, UNROLL + 1, 4.0, force="selected_largest")
        assert want["d"].max() > want["part"][:want["nparts"]].max()   # the largest residual is NOT among the partials
        check_update(got, want)


def test_update_kernel_stop_word_leaves_everything(ctx):
    got, want = update_case(ctx, 257, UNROLL + 1, 4.0, stop=1)
    assert np.array_equal(got["L"], want["L0"]) and np.array_equal(got["resid"], want["resid0"])
    assert np.all(got["part"] == 123.0) and np.all(got["pidx"] == 77)


def pick_case(ctx, part, pidx, j, M, tol, dmax0=0.0, stop=0, rows=None, cand=None, seed=0):
    """One gpt_dev_greedy_pick on given partials; the factor, X and the marks seeded.  Returns the device's state afterwards."""
    import torch
    nparts = len(pidx)
    rows = nparts * WG if rows is None else rows
    rs = np.random.RandomState(seed + nparts)
    ld, D = rows + 5, 3
    L = rs.randint(-5, 6, size=(max(j, 1) + 1, ld)).astype(float)
    X = rs.randint(-9, 10, size=(rows, D)).astype(float)
    dL, dX, dmark = dev(L), dev(X), dev(np.zeros(rows, dtype=np.int32))
    dscal, dwords = dev(np.array([55.0, dmax0])), dev(np.array([stop, 0, -7, 0], dtype=np.int32))
    didx, ddmax, dtrace = dev(np.full(M + 2, -5, dtype=np.int32)), dev(np.full(M + 2, -5.0)), dev(np.full(M + 3, -5.0))
    dxp, dprow = dev(np.full(16, -5.0)), dev(np.full(max(j, 1) + 4, -5.0))
    dpart, dpidx = dev(np.asarray(part, dtype=float)), dev(np.asarray(pidx, dtype=np.int32))
    dcand = None if cand is None else dev(np.asarray(cand, dtype=np.int32))
    torch.cuda.synchronize()
    ctx.dev_greedy_pick(j, M, tol, dpart.data_ptr(), dpidx.data_ptr(), nparts, None if cand is None else dcand.data_ptr(), dX.data_ptr(), D,
                        dL.data_ptr(), ld, dmark.data_ptr(), dscal.data_ptr(), dwords.data_ptr(), didx.data_ptr(), ddmax.data_ptr(),
                        dtrace.data_ptr(), dxp.data_ptr(), dprow.data_ptr())
    ctx.synchronize()
    return dict(mark=dmark.cpu().numpy(), scal=dscal.cpu().numpy(), words=dwords.cpu().numpy(), idx=didx.cpu().numpy(),
                dmax=ddmax.cpu().numpy(), trace=dtrace.cpu().numpy(), xp=dxp.cpu().numpy(), prow=dprow.cpu().numpy(), L=L, X=X)


@pytest.mark.parametrize("nparts", [1, 2, 255, 256, 257, 1000])
def test_pick_kernel_exact(ctx, nparts):
    rs = np.random.RandomState(nparts)
    vals = rs.randint(1, 50, size=nparts).astype(float)
    sums = rs.randint(0, 1000, size=nparts).astype(float)
    pidx = (np.arange(nparts) * WG + rs.randint(0, WG, size=nparts)).astype(np.int32)
    top = vals.max() + 3.0
    hits = sorted(set([nparts - 1, nparts // 2]))                  # the largest value twice (once for one partial): the lower row wins
    vals[hits] = top
    if nparts > 2:                                                   # ... and a workgroup with nothing left
        vals[1], pidx[1], sums[1] = -np.inf, IMAX, 0.0
    part = np.concatenate([vals, sums])
    j, M = 5, 9
    cand = np.arange(nparts * WG, dtype=np.int32) * 2 + 1
    r = pick_case(ctx, part, pidx, j, M, 0.0, dmax0=100.0, cand=cand)
    p = int(pidx[hits[0]])
    assert r["trace"][j] == sums.sum() and np.all(np.delete(r["trace"], j) == -5.0)
    assert r["idx"][j] == cand[p] and r["dmax"][j] == top and np.all(np.delete(r["idx"], j) == -5) and np.all(np.delete(r["dmax"], j) == -5.0)
    want_mark = np.zeros(nparts * WG, dtype=np.int32)
    want_mark[p] = 1
    assert np.array_equal(r["mark"], want_mark)
    assert r["scal"][0] == top and r["scal"][1] == 100.0 and list(r["words"]) == [0, j + 1, p, 0]
    assert np.array_equal(r["xp"][:3], r["X"][p]) and np.all(r["xp"][3:] == -5.0)
    assert np.array_equal(r["prow"][:j], r["L"][:j, p]) and np.all(r["prow"][j:] == -5.0)
    # step 0 sets dmax_0; the closing launch (j == M) writes the trace and nothing else
    r = pick_case(ctx, part, pidx, 0, M, 0.0)
    assert r["scal"][0] == top and r["scal"][1] == top and list(r["words"]) == [0, 1, p, 0] and r["idx"][0] == p
    r = pick_case(ctx, part, pidx, M, M, 0.0, dmax0=100.0)
    assert r["trace"][M] == sums.sum() and not r["mark"].any() and list(r["words"]) == [0, 0, -7, 0] and np.all(r["idx"] == -5)
    print("%d partials: pick, trace, marks, words, staging exact" % nparts)


def test_pick_kernel_stop_rule(ctx):
    part, pidx = np.array([4.0, 2.0, 10.0, 1.0]), np.array([3, 300], dtype=np.int32)
    r = pick_case(ctx, part, pidx, 3, 9, 0.05, dmax0=100.0)          # 4 <= 0.05 * 100: stop, count = 3
    assert list(r["words"]) == [1, 3, -7, 0] and r["trace"][3] == 11.0 and not r["mark"].any() and np.all(r["idx"] == -5)
    r = pick_case(ctx, part, pidx, 3, 9, 0.03, dmax0=100.0)          # 4 > 3: goes on
    assert list(r["words"]) == [0, 4, 3, 0]
    for bad in (0.0, -1.0, np.inf, np.nan):
        r = pick_case(ctx, np.array([bad, 2.0]), np.array([0], dtype=np.int32), 0, 9, 0.0)
        assert r["words"][0] == 1 and r["words"][1] == 0 and r["words"][3] == 1, bad
    r = pick_case(ctx, part, pidx, 3, 9, 0.0, dmax0=100.0, stop=1)   # already stopped: nothing is written
    assert list(r["words"]) == [1, 0, -7, 0] and np.all(r["trace"] == -5.0)


@pytest.mark.parametrize("pair", [(255, 256), (256, 767), (511, 768)])
def test_tie_across_workgroups_resolves_to_the_lower_row(ctx, pair):
    """The last row of one workgroup and the first row of another carry the same, largest residual: update, then pick."""
    rows, j = 1025, UNROLL + 1
    got, want = update_case(ctx, rows, j, 4.0, force=pair)
    check_update(got, want)
    nparts = want["nparts"]
    assert sorted(int(v) for v in want["pidx"][[pair[0] // WG, pair[1] // WG]]) == list(pair)
    r = pick_case(ctx, got["part"][:2 * nparts], got["pidx"][:nparts], 2, 9, 0.0, dmax0=1e9, rows=rows)
    assert r["idx"][2] == min(pair) and r["dmax"][2] == 5000.0


# ---- (2) the whole call against the yardstick ---------------------------------------------------------------------------------------
def kernel_of(g, terms, d):
    cls = {"se": g.SquaredExponentialKernel, "m52": g.Matern52Kernel, "gibbs_tanh": g.GibbsKernel1dTanh}

    def one(name, p):
        if name == "gibbs_tanh":
            return cls[name](initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
        return cls[name](num_dim=d, initial_params=list(p), param_bounds=[(0.0, 1e3)] * len(p))
    out = None
    for t in terms:
        k = one(t[0], t[1]) * one(t[2], t[3]) if len(t) == 4 else one(t[0], t[1])
        out = k if out is None else out + k
    return out


def compare(name, rows, y64, yld, info, label=""):
    """Pivots entry for entry, dmax and trace within the case's bounds; returns the worst ratios (dmax, trace)."""
    ncand, kmax = len(rows), yld["kmax"]
    assert len(info["indices"]) == y64["count"] and len(info["trace"]) == y64["count"] + 1
    first_diff = np.flatnonzero(info["indices"] != rows[y64["idx"]])
    print("%s%s: pivots differ at %s of %d" % (name, label, first_diff[:5], y64["count"]))
    rd = rt = 0.0
    for j in range(y64["count"] + 1):
        if j < y64["count"] and not first_diff.size:
            rd = max(rd, float(abs(np.longdouble(info["dmax"][j]) - yld["dmax"][j])) / kmax / G.dmax_bound(name, j))
        if not first_diff.size:
            rt = max(rt, float(abs(np.longdouble(info["trace"][j]) - yld["trace"][j])) / kmax / G.trace_bound(name, j, ncand))
    print("%s%s: worst |device - longdouble| / bound: dmax %.3g, trace %.3g (HOST_ERR %.3g)" % (name, label, rd, rt, G.HOST_ERR[name]))
    assert not first_diff.size, (name, first_diff[:5], info["indices"][first_diff[:5]], rows[y64["idx"]][first_diff[:5]])
    assert rd <= 1.0 and rt <= 1.0, (name, rd, rt)
    return rd, rt


@pytest.mark.parametrize("name", list(G.CASES))
def test_selection_against_the_yardstick(g, oracle, name):
    """Every case of the table: pivots entry for entry, dmax and trace within the case's bounds.  The Gibbs case's step 0 is a complete
    tie like every other case's (k(x, x) = sigma_f^2 whatever l(x) is): it passes because the device's Gibbs variance has the same bits in
    every row (gibbs_core takes the prefactor of equal length scales as exactly 1); with the prefactor as a product of roots, 1 within
    a few u, the device's first pivot was row 17 and 32 of the 33 pivots differed."""
    c = G.CASES[name]
    X, n = G.case_points(name)
    K, rows, y64, yld = G.reference(oracle, name)
    Z, info = g.greedy_inducing(kernel_of(g, c["terms"], c["d"]), X, c["M"], n=n)
    assert np.array_equal(Z, X[info["indices"]]) and Z.shape == (c["M"], c["d"])
    assert np.all(n[info["indices"]] == 0)                          # no derivative row is ever returned
    compare(name, rows, y64, yld, info)


# ---- (3) contract edges -------------------------------------------------------------------------------------------------------------
def device_terms(g, name):
    from gptools_amd import sparse
    c = G.CASES[name]
    return sparse._device_terms(g.GaussianProcess(kernel_of(g, c["terms"], c["d"])))


def test_derivative_rows_are_no_candidates(g):
    X, n = G.case_points("m52_der")
    k = kernel_of(g, G.CASES["m52_der"]["terms"], 2)
    with pytest.raises(ValueError, match="row 115"):
        g.greedy_inducing(k, X, 5, n=n, candidates=[3, 115, 7])


def test_candidate_subset_equals_the_yardstick_on_it(g, oracle):
    name = "m52_m127"
    X, n = G.case_points(name)
    sub = np.sort(np.random.RandomState(4).choice(len(X), 150, replace=False))
    K = G.gram(oracle, G.CASES[name]["terms"], X[sub])
    y64, yld = G.yardstick(K, 40), G.yardstick(K, 40, dtype=np.longdouble)
    assert np.array_equal(y64["idx"], yld["idx"]) and y64["gap"][1:].min() >= G.GAP_MIN
    Z, info = g.greedy_inducing(kernel_of(g, G.CASES[name]["terms"], 2), X, 40, n=n, candidates=sub[::-1])      # (sorted by the call)
    compare(name, sub, y64, yld, info, label=" (150 candidates)")
    with pytest.raises(ValueError, match="more than once"):
        g.greedy_inducing(kernel_of(g, G.CASES[name]["terms"], 2), X, 4, n=n, candidates=[1, 5, 5])
    # max_candidates: the seeded subsample, sorted, is what an explicit list of the same rows gives
    Za, ia = g.greedy_inducing(kernel_of(g, G.CASES[name]["terms"], 2), X, 10, n=n, max_candidates=50, seed=3)
    pool = np.sort(np.random.RandomState(3).choice(len(X), 50, replace=False))
    Zb, ib = g.greedy_inducing(kernel_of(g, G.CASES[name]["terms"], 2), X, 10, n=n, candidates=pool)
    assert np.array_equal(ia["indices"], ib["indices"]) and np.all(np.isin(ia["indices"], pool)) and np.array_equal(Za, Zb)


def test_duplicated_points_ties_and_the_stop_rule(g):
    X, _ = G.case_points("m52_m63")
    X2 = np.concatenate([X[:60], X[:60]])
    k = kernel_of(g, G.CASES["m52_m63"]["terms"], 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Z, info = g.greedy_inducing(k, X2, 60)
    print("duplicates, M = 60: pivots %s ..., dmax_59 = %.3g, trace_60 = %.3g" % (info["indices"][:6], info["dmax"][-1], info["trace"][-1]))
    assert len(info["indices"]) == 60 and np.all(info["indices"] < 60) and len(set(info["indices"])) == 60
    with pytest.warns(RuntimeWarning, match="stopped after 60 of 90"):
        Z, info = g.greedy_inducing(k, X2, 90, tol=1e-9)
    assert Z.shape == (60, 2) and len(info["indices"]) == 60 and len(info["dmax"]) == 60 and len(info["trace"]) == 61
    assert np.all(info["indices"] < 60)


def test_refusals_of_the_library(g):
    from gptools_amd import _lib
    name = "m52_m63"
    X, n = G.case_points(name)
    terms = device_terms(g, name)
    ctx = _lib.Context()
    with pytest.raises(_lib.GPTBackendError):                         # GPT_E_STATE: no data
        ctx.sparse_select_inducing(terms, 4)
    ctx.set_data(X, n)
    with pytest.raises(ValueError, match="exceeds the 130 candidates"):
        ctx.sparse_select_inducing(terms, 131)
    with pytest.raises(ValueError, match="exceeds the 3 candidates"):
        ctx.sparse_select_inducing(terms, 4, candidates=[1, 2, 3])
    with pytest.raises(ValueError, match="strictly ascending"):
        ctx.sparse_select_inducing(terms, 2, candidates=[1, 3, 2])
    with pytest.raises(ValueError, match="strictly ascending"):
        ctx.sparse_select_inducing(terms, 2, candidates=[1, 130])
    with pytest.raises(ValueError):
        ctx.sparse_select_inducing(terms, 0)
    with pytest.raises(ValueError):
        ctx.sparse_select_inducing(terms, 2, tol=-1.0)
    ctx.set_T(np.eye(len(X)))
    with pytest.raises(NotImplementedError, match="linear transform"):
        ctx.sparse_select_inducing(terms, 4)
    ctx.set_T(None)
    ctx.set_warp([(_lib.WARP_LINEAR, np.array([0.0, 0.0, 1.0, 1.0]))])
    with pytest.raises(NotImplementedError, match="warp layers"):
        ctx.sparse_select_inducing(terms, 4)
    ctx.set_warp(None)
    a = ctx.sparse_select_inducing(terms, 4)
    assert len(a[0]) == 4


def test_two_calls_give_equal_bits(g):
    from gptools_amd import _lib
    name = "sum_prod_70"
    X, n = G.case_points(name)
    terms = device_terms(g, name)
    ctx = _lib.Context()
    ctx.set_data(X, n)
    a = ctx.sparse_select_inducing(terms, 70)
    b = ctx.sparse_select_inducing(terms, 70)
    for u, v in zip(a, b):
        assert np.array_equal(u, v) and u.tobytes() == v.tobytes()


# ---- (4) nothing else moves ---------------------------------------------------------------------------------------------------------
def test_dense_and_sparse_state_survive_a_selection(g):
    from gptools_amd import _lib
    d = S.case_data("se_300")
    ctx = _lib.Context()
    ctx.set_data(d["X"], d["n"])
    N = len(d["y"])
    ctx.fit(_lib.KERNEL_SE, S.SE2, S.NOISE ** 2, d["y"], d["err_y"], 1e2 * np.finfo(float).eps)
    L0 = ctx.get_L(N).copy()
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    terms = [(_lib.KERNEL_SE, S.SE2)]
    ll0, parts0 = ctx.sparse_fit(_lib.SPARSE_METHODS["vfe"], terms, S.NOISE ** 2, d["y"], d["err_y"], S.JITTER, 128)
    c0 = ctx.sparse_get_c().copy()
    pred0 = ctx.sparse_predict(d["Xs"], d["ns"], 1)
    idx, dmax, trace = ctx.sparse_select_inducing(terms, 40)
    assert len(idx) == 40 and np.all(d["n"][idx] == 0)
    assert np.array_equal(ctx.get_L(N), L0)
    assert np.array_equal(ctx.sparse_get_c(), c0)
    pred1 = ctx.sparse_predict(d["Xs"], d["ns"], 1)                  # (the sparse fit is still resident: no GPT_E_STATE)
    for a, b in zip(pred0[:2], pred1[:2]):
        assert np.array_equal(a, b)
    ll1, parts1 = ctx.sparse_fit(_lib.SPARSE_METHODS["vfe"], terms, S.NOISE ** 2, d["y"], d["err_y"], S.JITTER, 128)
    assert ll1 == ll0 and np.array_equal(parts0, parts1)


# ---- (5) through the class ------------------------------------------------------------------------------------------------------------
def test_select_inducing_through_the_class(g, oracle):
    name, M = G.CLASS_CASE, G.CLASS_M
    c = G.CASES[name]
    X, n, y = S.inputs(c["N"], c["d"], nder=0)
    N = len(X)

    def gp_with(Z):
        return g.SparseGaussianProcess(kernel_of(g, c["terms"], c["d"]), Z, method="vfe", jitter=0.0, X=X, y=y, err_y=0, n=n,
                                       noise_k=g.DiagonalNoiseKernel(num_dim=c["d"], initial_noise=G.CLASS_NOISE, noise_bound=(0.0, 5.0)))

    def vfe_trace(gp):
        gp.compute_K_L_alpha_ll()
        return gp.ll_parts[4] * G.CLASS_NOISE ** 2

    gp = gp_with(X[:M])
    Z, info = gp.select_inducing(M)
    assert np.array_equal(gp.Z, Z) and np.all(gp.n_Z == 0) and not gp.K_up_to_date
    t_fit, t_sel = vfe_trace(gp), info["trace"][-1]
    K = G.reference(oracle, name)[0]
    kmax = np.diag(K).max()
    bound = max(10.0 * G.TRACE_ERR[name], N * M * G.U)
    print("greedy %d of %d: VFE trace of the fit %.15g, trace_M of the selection %.15g, difference %.3g of max k_ii (bound %.3g)"
          % (M, N, t_fit, t_sel, abs(t_fit - t_sel) / kmax, bound))
    assert abs(t_fit - t_sel) / kmax <= bound
    for seed in G.CLASS_SEEDS:
        t = vfe_trace(gp_with(X[G.random_subset(N, M, seed)]))
        print("    random subset, seed %d: VFE trace %.6g (greedy %.6g)" % (seed, t, t_fit))
        assert t_fit < t
    Z2, info2 = g.greedy_inducing(kernel_of(g, c["terms"], c["d"]), X, M, n=n)
    assert np.array_equal(Z, Z2) and np.array_equal(info["indices"], info2["indices"])
    Z3, _ = gp.select_inducing(8, set=False)
    assert Z3.shape == (8, c["d"]) and np.array_equal(gp.Z, Z)
