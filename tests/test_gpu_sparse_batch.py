"""GPU suite (-m gpu): a batch of sparse fits in one launch sequence -- gpt_sparse_fit_batch (api_sparse_batch.inc, the batched kernels of
ksparse.hip) through _lib.Context.sparse_fit_batch and SparseGaussianProcess.sparse_ll_batch, and its four kernel groups alone on raw
device pointers.

Two yardsticks.  Bits: an element's ll and five parts are those gpt_sparse_fit returns for that element alone with the same chunk_rows
(the single fit is the older code; the test cannot pass without the batched entry point).  Values: the host's dense route at each
element's parameters (tests/sparse_batch_cases.py), ten times the host's own discrepancy, measured on the CPU by
tests/test_sparse_batch_host.py.  Each figure is printed before it is asserted."""
import functools
import warnings

import numpy as np
import pytest

import sparse_cases as S
import sparse_batch_cases as SB

pytestmark = pytest.mark.gpu

PARAMS = [(name, m, ch) for name in SB.BATCH_CASES for m in S.CASES[name]["methods"] for ch in S.CASES[name]["chunks"]]
ULP4 = 4.0 * 2.0 ** -52


@pytest.fixture(scope="module")
def g():
    warnings.simplefilter("ignore")
    import gptools_amd
    return gptools_amd


def lib():
    from gptools_amd import _lib
    return _lib


def device_terms(terms):
    """sparse_cases' terms with the library's kernel ids."""
    kid = {"se": lib().KERNEL_SE, "m52": lib().KERNEL_M52, "rq": lib().KERNEL_RQ}
    return [tuple(kid[v] if i % 2 == 0 else list(v) for i, v in enumerate(t)) for t in terms]


@functools.lru_cache(maxsize=None)
def case_ctx(name):
    """One context per case with its data and inducing inputs: shared, the tests below leave both resident."""
    d = S.case_data(name)
    ctx = lib().Context()
    ctx.set_data(d["X"], d["n"])
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    return ctx


def elements(name):
    return [device_terms(t) for t in SB.element_terms(name)], np.array(SB.element_noise()) ** 2.0


@functools.lru_cache(maxsize=None)
def single_fits(name, method, chunk):
    """gpt_sparse_fit of every element alone: computed once, shared, never modified."""
    d, ctx = S.case_data(name), case_ctx(name)
    terms, nv = elements(name)
    out = [ctx.sparse_fit(lib().SPARSE_METHODS[method], terms[b], nv[b], d["y"], d["err_y"], S.JITTER, chunk or 0) for b in range(SB.NELEM)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def batch_fit(name, method, chunk, order, y=None, nv=None, err_y=None, jitter=S.JITTER):
    d, ctx = S.case_data(name), case_ctx(name)
    terms, nv0 = elements(name)
    nv = nv0 if nv is None else nv
    y = np.tile(d["y"], (SB.NELEM, 1)) if y is None else y
    order = list(order)
    return ctx.sparse_fit_batch(lib().SPARSE_METHODS[method], [terms[b] for b in order], nv[order], y[order],
                                d["err_y"] if err_y is None else err_y, jitter, chunk or 0)


@functools.lru_cache(maxsize=None)
def host_ref(name, method, b):
    from oracle import oracle as O
    O.build()
    return SB.host_routes(O, name, method, b)[1]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- 1. the fit, against the single fit and the host ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,chunk", PARAMS)
def test_batch_against_the_single_fit_and_the_host(name, method, chunk):
    """Five elements in one call: ll and the five parts of every element carry the bits of gpt_sparse_fit at that element's parameters
    with the same chunk_rows, and lie within the host's bound.  se1_64: M = 1, one leaf each; se_300: three methods, one chunk and
    three (the last with 44 rows); rq_257: d = 1, derivative rows among Z; se_m127 / se_m128: the padding edges (MPU < BP at 128);
    sum_m257: sum + product terms, three 128-blocks; m52_m520: MPU = 640 > 512, the left-looking leaf update with k > 0 and the
    remainder pass of the row kernel past 512."""
    N = S.CASES[name]["N"]
    ll1, parts1 = single_fits(name, method, chunk)
    ll, parts, info, which = batch_fit(name, method, chunk, range(SB.NELEM))
    assert not info.any() and not which.any()
    for b in range(SB.NELEM):
        fig = SB.fit_figures(dict(ll=ll[b], parts=parts[b]), host_ref(name, method, b))
        for k in SB.FIT_FIGURES:
            print("%s %s chunk %s element %d: %s device - host = %.3g (bound %.3g)" % (name, method, chunk, b, k, fig[k], SB.bound(name, k, N)))
    print("ll batch - single:", ll - ll1, " parts:", np.abs(parts - parts1).max(0))
    assert same_bits(ll, ll1) and same_bits(parts, parts1)
    for b in range(SB.NELEM):
        fig = SB.fit_figures(dict(ll=ll[b], parts=parts[b]), host_ref(name, method, b))
        for k in SB.FIT_FIGURES:
            assert fig[k] <= SB.bound(name, k, N), (b, k, fig[k])


# ---- 2. invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,method,chunk", [("se_300", "vfe", 128), ("sum_m257", "fitc", 128)])
def test_bits_do_not_depend_on_the_batch(name, method, chunk):
    """Reversed order, each element alone (nbatch = 1), as part of nbatch = 2 and 3, and the whole call twice: the same bits per element."""
    ll0, parts0, _, _ = batch_fit(name, method, chunk, range(SB.NELEM))
    for order in ([4, 3, 2, 1, 0], [0, 1, 2, 3, 4], [0], [1], [2], [3], [4], [1, 4], [3, 0], [2, 2], [4, 0, 2], [1, 3, 1]):
        ll, parts, info, which = batch_fit(name, method, chunk, order)
        assert not which.any() and not info.any()
        assert same_bits(ll, ll0[order]) and same_bits(parts, parts0[order]), order


# ---- 3. failing elements ----------------------------------------------------------------------------------------------------------------
def test_duplicated_inducing_row_fails_every_element():
    """Z is shared: Z[1] = Z[0] with sigma_f = 1 and jitter = 0 makes the second pivot of every element's K_uu exactly 0 -- which = 1 and
    info = 2 for all, and the call itself succeeds."""
    d = S.case_data("se_m64")
    Z = d["Z"].copy()
    Z[1] = Z[0]
    ctx = lib().Context()
    ctx.set_data(d["X"], d["n"])
    ctx.sparse_set_inducing(Z, d["nZ"])
    terms = [[(lib().KERNEL_SE, [1.0, 0.4 * f, 0.6 * f])] for f in (1.0, 0.9, 1.1)]
    ll, parts, info, which = ctx.sparse_fit_batch(0, terms, np.full(3, 0.01), np.tile(d["y"], (3, 1)), d["err_y"], 0.0, 64)
    assert np.array_equal(which, [1, 1, 1]) and np.array_equal(info, [2, 2, 2])
    with pytest.raises(np.linalg.LinAlgError):
        ctx.sparse_fit(0, terms[1], 0.01, d["y"], d["err_y"], 0.0, 64)


def test_one_bad_lambda_among_good_elements():
    """dtc with noise_var[1] = 0 and an err_y that holds a zero: Lambda_7 = 0 for element 1 alone -- which = 2 there, and the other
    elements keep the bits of their single fits at the same err_y."""
    name, d = "se_300", S.case_data("se_300")
    ctx = case_ctx(name)
    terms, nv = elements(name)
    nv = nv.copy()
    nv[1] = 0.0
    err = d["err_y"].copy()
    err[7] = 0.0
    ll, parts, info, which = batch_fit(name, "dtc", 128, range(SB.NELEM), nv=nv, err_y=err)
    assert np.array_equal(which, [0, 2, 0, 0, 0]) and not info.any()
    for b in (0, 2, 3, 4):
        l1, p1 = ctx.sparse_fit(2, terms[b], nv[b], d["y"], err, S.JITTER, 128)
        assert same_bits(ll[b], l1) and same_bits(parts[b], p1), b
    with pytest.raises(ValueError):
        ctx.sparse_fit(2, terms[1], 0.0, d["y"], err, S.JITTER, 128)


def test_a_nan_in_one_elements_y():
    """NaN in y of element 2: its augmented pivot fails -- which = 3, info = M -- and the others keep the bits of test 1."""
    name, method, chunk = "se_m127", "fitc", 64
    d = S.case_data(name)
    y = np.tile(d["y"], (SB.NELEM, 1))
    y[2, 11] = np.nan
    ll1, parts1 = single_fits(name, method, chunk)
    ll, parts, info, which = batch_fit(name, method, chunk, range(SB.NELEM), y=y)
    assert np.array_equal(which, [0, 0, 3, 0, 0]) and np.array_equal(info, [0, 0, S.CASES[name]["M"], 0, 0])
    keep = [0, 1, 3, 4]
    assert same_bits(ll[keep], ll1[keep]) and same_bits(parts[keep], parts1[keep])
    terms, nv = elements(name)
    with pytest.raises(np.linalg.LinAlgError):
        case_ctx(name).sparse_fit(0, terms[2], nv[2], y[2], d["err_y"], S.JITTER, chunk)


# ---- 4. residency ---------------------------------------------------------------------------------------------------------------------
def test_resident_fits_survive_a_batch(g):
    """A single sparse fit's ll, c and prediction, and the dense factor's prediction, are bit-equal before and after a batch on the same
    context; after release_batch_scratch a second batch gives the first one's bits."""
    d = S.case_data("se_300")
    nk = g.DiagonalNoiseKernel(num_dim=2, initial_noise=S.NOISE, noise_bound=(0.0, 5.0))
    terms, nv = elements("se_300")
    ctx = lib().Context()
    ctx.set_data(d["X"], d["n"])
    ctx.fit(lib().KERNEL_SE, S.SE2, S.NOISE ** 2, d["y"], d["err_y"], 1e2 * np.finfo(float).eps)
    dense_before = ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    ll_s, _ = ctx.sparse_fit(0, terms[0], nv[0], d["y"], d["err_y"], S.JITTER, 128)
    c_before, sp_before = ctx.sparse_get_c(), ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)
    y5 = np.tile(d["y"], (SB.NELEM, 1))
    first = ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER, 128)
    assert same_bits(first[0][0], ll_s)
    assert np.array_equal(ctx.sparse_get_c(), c_before)
    for a, b in zip(sp_before, ctx.sparse_predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(a, b)
    for a, b in zip(dense_before, ctx.predict(d["Xs"], d["ns"], 2, nk.params, nk.n)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    ctx.release_batch_scratch()
    second = ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER, 128)
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])
    assert np.array_equal(ctx.sparse_get_c(), c_before)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library():
    _lib = lib()
    d = S.case_data("se_300")
    terms, nv = elements("se_300")
    y5 = np.tile(d["y"], (SB.NELEM, 1))
    ctx = _lib.Context()
    with pytest.raises(_lib.GPTBackendError):                     # GPT_E_STATE: no data
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER)
    ctx.set_data(d["X"], d["n"])
    with pytest.raises(_lib.GPTBackendError):                     # no inducing inputs
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER)
    ctx.sparse_set_inducing(d["Z"], d["nZ"])
    ctx.set_T(np.eye(300))
    with pytest.raises(NotImplementedError):
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER)
    ctx.set_T(None)
    ctx.set_warp([(_lib.WARP_LINEAR, [-0.5, -0.25, 1.5, 2.0])])
    with pytest.raises(NotImplementedError):
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER)
    ctx.set_warp(None)
    ip, dp, z = _lib.iptr, _lib.dptr, np.zeros(8)
    ids, ids2, npar, npar1, flat = ctx._pack_terms(terms[0])
    info = np.zeros(2, dtype=np.int32)
    rc = _lib.load().gpt_sparse_fit_batch(ctx.handle, 0, 0, 1, ip(ids), ip(ids2), dp(flat), ip(npar), ip(npar1), dp(z), dp(_lib.f64(d["y"])),
                                          dp(_lib.f64(d["err_y"])), S.JITTER, 0, dp(z), None, ip(info), ip(info))
    assert rc == _lib.GPT_E_ARG                                   # nbatch = 0
    # one element's parameter out of its domain (a Matern order of 70, outside (0, 60)) fails the whole call with the parser's status
    ctx0 = _lib.Context()
    ctx0.set_data(d["X"], np.zeros_like(d["n"]))
    ctx0.sparse_set_inducing(d["Z"], d["nZ"])
    matern = [[(_lib.KERNEL_MATERN, [1.0, nu, 0.4, 0.6])] for nu in (1.5, 2.5, 1.5)]
    ll, _, _, which = ctx0.sparse_fit_batch(0, matern, nv[:3], y5[:3], d["err_y"], S.JITTER)
    assert np.all(np.isfinite(ll)) and not which.any()
    matern[2] = [(_lib.KERNEL_MATERN, [1.0, 70.0, 0.4, 0.6])]
    with pytest.raises(ValueError):
        ctx0.sparse_fit_batch(0, matern, nv[:3], y5[:3], d["err_y"], S.JITTER)
    with pytest.raises(ValueError):
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER, chunk_rows=100)
    with pytest.raises(ValueError):
        ctx.sparse_fit_batch(3, terms, nv, y5, d["err_y"], S.JITTER)
    with pytest.raises(ValueError):
        ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], -1.0)
    ll, _, info, which = ctx.sparse_fit_batch(0, terms, nv, y5, d["err_y"], S.JITTER)
    assert np.all(np.isfinite(ll)) and not which.any()


# ---- 6. Python ------------------------------------------------------------------------------------------------------------------------
def python_gp(g, **kw):
    d = S.case_data("se_300")
    hp = g.GammaJointPriorAlt([1.0, 0.4, 0.5], [0.5, 0.2, 0.3])
    k = g.SquaredExponentialKernel(num_dim=2, initial_params=S.SE2, hyperprior=hp)
    args = dict(noise_k=g.DiagonalNoiseKernel(num_dim=2, initial_noise=S.NOISE, noise_bound=(0.0, 5.0)), method="vfe", jitter=S.JITTER,
                chunk_rows=128, X=d["X"], y=d["y"], err_y=d["err_y"], n=np.zeros_like(d["n"]),
                mu=g.LinearMeanFunction(num_dim=2, initial_params=[0.2, -0.1, 0.05]))
    args.update(kw)
    return g.SparseGaussianProcess(k, d["Z"], **args)


def seven_vectors(gp):
    rs = np.random.RandomState(5)
    x0 = np.array(gp.free_params[:], dtype=float)
    vecs = [x0 * rs.uniform(0.9, 1.1, size=x0.size) for _ in range(7)]
    vecs[4][3] = 7.0                                             # the noise sigma outside its bound (0, 5): -inf
    return vecs


def test_sparse_ll_batch_is_update_hyperparameters_bit_for_bit(g):
    """7 vectors of a GP with a Gamma prior, bounds and a linear mean function with free parameters (y - mu differs per element)."""
    gp = python_gp(g)
    vecs = seven_vectors(gp)
    assert len(vecs[0]) == 7
    gp.compute_K_L_alpha_ll()
    here, ll_here = np.array(gp.free_params[:], dtype=float), gp.ll
    out = gp.sparse_ll_batch(vecs)
    assert np.array_equal(gp.free_params[:], here) and gp.K_up_to_date and gp.ll == ll_here
    loop = np.array([-gp.update_hyperparameters(v) for v in vecs])
    print("sparse_ll_batch:", out, "\nloop - batch:", loop - out)
    assert np.isneginf(out[4]) and np.all(np.isfinite(np.delete(out, 4)))
    assert same_bits(out, loop)
    gp.sparse_batch_grid = 3                                     # 3 + 3 + 1
    calls = []
    real = type(gp._ctx).sparse_fit_batch
    gp._ctx.sparse_fit_batch = lambda *a, **kw: calls.append(len(a[1])) or real(gp._ctx, *a, **kw)
    cut = gp.sparse_ll_batch(vecs)
    del gp._ctx.sparse_fit_batch
    assert calls == [3, 3] and same_bits(cut, out)               # (six vectors reach the device: the seventh is excluded by its prior)
    gp.sparse_batch_grid = 16
    assert same_bits(gp.sparse_ll_batch(vecs), out)


def test_compute_ll_matrix_and_the_host_stepped_sampler(g):
    """_ll_rows routes to sparse_ll_batch: a 2 x 2 x 2 grid equals the loop, and a seeded chain (8 walkers x 3 steps) is the same with
    sparse_batch_grid = 1 (the loop) and = 16."""
    d = S.case_data("se1_64")
    def gp_of(grid):
        k = g.SquaredExponentialKernel(num_dim=1, initial_params=[1.1, 0.35], param_bounds=[(0.5, 2.0), (0.1, 1.0)])
        gp = g.SparseGaussianProcess(k, d["Z"], noise_k=g.DiagonalNoiseKernel(num_dim=1, initial_noise=S.NOISE, noise_bound=(0.01, 0.5)),
                                     method="fitc", jitter=S.JITTER, X=d["X"], y=d["y"], err_y=d["err_y"], n=d["n"])
        gp.sparse_batch_grid = grid
        return gp
    grids = []
    for grid in (1, 16):
        gp = gp_of(grid)
        ll_vals, axes = gp.compute_ll_matrix([(0.8, 1.2), (0.3, 0.4), (0.05, 0.15)], 2)
        assert ll_vals.shape == (2, 2, 2) and np.all(np.isfinite(ll_vals))
        assert ll_vals[1, 0, 1] == -gp.update_hyperparameters([axes[0][1], axes[1][0], axes[2][1]])
        theta0 = np.array([1.1, 0.35, 0.1]) * np.random.RandomState(2).uniform(0.9, 1.1, size=(8, 3))
        s = gp.sample_hyperparameter_posterior(nwalkers=8, nsamp=3, theta0=theta0, random_state=7, stepping="host")
        grids.append((ll_vals, np.array(s.chain)))
    assert same_bits(grids[0][0], grids[1][0]) and same_bits(grids[0][1], grids[1][1])


# ---- 7. the kernels alone, through the device API -------------------------------------------------------------------------------------
def _ip(t):
    return lib().C.cast(t.data_ptr(), lib()._ip)


@pytest.mark.parametrize("nbatch", [1, 2, 3])
@pytest.mark.parametrize("rows,mg,nslices", [(1, 64, 1), (5, 192, 0), (130, 128, 7), (257, 64, 0)])
def test_gram_batch_kernel_alone(nbatch, rows, mg, nslices):
    """gpt_dev_sparse_gram_batch on integer data (every summation order gives the same bits): G_b += V_b^T V_b against numpy, exactly,
    with an element stride larger than rows x ldv whose gap holds NaN, and ldg > mg whose extra columns keep their bits; then on
    non-integer data bit-equal per element to gpt_dev_sparse_gram."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(rows + mg + nbatch)
    ldv, ldg = mg + 64, mg + 64
    vrows = rows + 3
    ctx = _lib.Context()
    low = np.tril(np.ones((mg // 64, mg // 64))).repeat(64, 0).repeat(64, 1) > 0
    for integer in (True, False):
        V = np.full((nbatch, vrows, ldv), np.nan)
        V[:, :rows] = rs.randint(-4, 5, size=(nbatch, rows, ldv)) if integer else rs.randn(nbatch, rows, ldv)
        G0 = rs.randint(-3, 4, size=(nbatch, mg, ldg)).astype(float)
        dV, dG = torch.tensor(V, device="cuda"), torch.tensor(G0, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_gram_batch(ctx.handle, nbatch, dV.data_ptr(), ldv, vrows * ldv, rows, mg, nslices, dG.data_ptr(),
                                                         ldg, mg * ldg))
        ctx.synchronize()
        got = dG.cpu().numpy()
        assert np.array_equal(got[:, :, mg:], G0[:, :, mg:])
        for b in range(nbatch):
            assert np.array_equal(got[b, :, :mg][~low], G0[b, :, :mg][~low])
            if integer:
                want = G0[b, :, :mg] + V[b, :rows, :mg].T.dot(V[b, :rows, :mg])
                assert np.array_equal(got[b, :, :mg][low], want[low]), b
            else:
                d1 = torch.tensor(G0[b], device="cuda")
                dVb = torch.tensor(V[b, :rows], device="cuda")
                torch.cuda.synchronize()
                _lib.check(_lib.load().gpt_dev_sparse_gram(ctx.handle, dVb.data_ptr(), ldv, rows, mg, nslices, d1.data_ptr(), ldg))
                ctx.synchronize()
                assert same_bits(got[b], d1.cpu().numpy()), b


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_row_pass_batch_alone(M, method):
    """gpt_dev_sparse_lambda_batch on six rows of integers, two elements with their own noise_var, k_i and r: q_i exactly (through
    (k_i - q_i) / s_i for vfe, s_i a power of two), log Lambda_i and the scaled row within 4 ulp, the columns behind M untouched, and
    every written bit equal to gpt_dev_sparse_lambda on the element alone.  fitc: a row of element 1 with Lambda < 0 raises word 1
    only and zeroes its own row (for vfe / dtc Lambda_i = s_i, which no row of one element alone can spoil: err is shared)."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(M + method)
    nb, rows, ldr = 2, 6, 8
    ldv = M + 3
    vrows = rows + 1
    V = rs.randint(-3, 4, size=(nb, vrows, ldv)).astype(float)
    q = (V[:, :rows, :M] ** 2).sum(2)
    kd = q + rs.randint(1, 9, size=(nb, rows))
    if method == 0:
        kd[1, 2] = -1e6
    r = rs.randint(-5, 6, size=(nb, rows)).astype(float)
    err = np.full(rows, 0.5)
    nv = np.array([0.75, 3.75])
    s = nv[:, None] + err[None, :] ** 2
    ctx = _lib.Context()
    dV = torch.tensor(V, device="cuda")
    dk, dr, de, dn = (torch.tensor(np.ascontiguousarray(a, dtype=float), device="cuda") for a in (kd, r, err, nv))
    drow = torch.full((nb, 2 * ldr + 1), -7.0, dtype=torch.float64, device="cuda")
    dbad = torch.zeros(nb + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_lambda_batch(ctx.handle, nb, dV.data_ptr(), ldv, vrows * ldv, rows, M, method, dk.data_ptr(), rows,
                                                       dr.data_ptr(), rows, de.data_ptr(), dn.data_ptr(), drow.data_ptr(), ldr, 2 * ldr + 1,
                                                       _ip(dbad)))
    ctx.synchronize()
    got, row, bad = dV.cpu().numpy(), drow.cpu().numpy(), dbad.cpu().numpy()
    assert np.array_equal(bad, [0, 1 if method == 0 else 0, 0])
    assert np.array_equal(got[:, :rows, M + 1:], V[:, :rows, M + 1:]) and np.array_equal(got[:, rows], V[:, rows])
    assert np.all(row[:, rows:ldr] == -7.0) and np.all(row[:, ldr + rows:] == -7.0)
    lam = (kd - q + s) if method == 0 else s
    ok = lam > 0
    if method == 1:
        assert np.array_equal(row[:, ldr:ldr + rows], (kd - q) / s)
    else:
        assert not row[:, ldr:ldr + rows].any()
    ref_log = np.where(ok, np.log(np.where(ok, lam, 1.0)), 0.0)
    assert np.all(np.abs(row[:, :rows] - ref_log) <= ULP4 * np.abs(ref_log))
    sc = np.where(ok, 1.0 / np.sqrt(np.where(ok, lam, 1.0)), 0.0)
    ref_rows = np.concatenate([V[:, :rows, :M] * sc[:, :, None], (r * sc)[:, :, None]], axis=2)
    assert np.all(np.abs(got[:, :rows, :M + 1] - ref_rows) <= ULP4 * np.abs(ref_rows))
    for b in range(nb):                                           # the element alone, through the single fit's launcher: the same bits
        dV1 = torch.tensor(V[b], device="cuda")
        d1 = torch.full((2 * ldr + 1,), -7.0, dtype=torch.float64, device="cuda")
        b1 = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_lambda(ctx.handle, dV1.data_ptr(), ldv, rows, M, method, dk[b].data_ptr(), dr[b].data_ptr(),
                                                     de.data_ptr(), float(nv[b]), d1.data_ptr(), ldr, _ip(b1)))
        ctx.synchronize()
        assert same_bits(got[b], dV1.cpu().numpy()) and same_bits(row[b], d1.cpu().numpy()) and int(b1.cpu()[0]) == bad[b]


@pytest.mark.parametrize("rows", [1, 256, 257, 1000])
def test_rowsum_batch_alone(rows):
    """gpt_dev_sparse_rowsum_batch on integers, three elements, two calls accumulating: both sums exactly onto what acc held; the
    entries between rows and ldr, the gap between the elements and acc[2:4] stay out."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(rows)
    nb, ldr = 3, rows + 5
    rv = rs.randint(-9, 10, size=(nb, 2 * ldr + 7)).astype(float)
    acc0 = rs.randint(-20, 20, size=(nb, 4)).astype(float)
    ctx = _lib.Context()
    drow, dacc = torch.tensor(rv, device="cuda"), torch.tensor(acc0, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        _lib.check(_lib.load().gpt_dev_sparse_rowsum_batch(ctx.handle, nb, drow.data_ptr(), ldr, 2 * ldr + 7, rows, dacc.data_ptr(), 4))
    ctx.synchronize()
    got = dacc.cpu().numpy()
    assert np.array_equal(got[:, 0], acc0[:, 0] + 2 * rv[:, :rows].sum(1))
    assert np.array_equal(got[:, 1], acc0[:, 1] + 2 * rv[:, ldr:ldr + rows].sum(1))
    assert np.array_equal(got[:, 2:], acc0[:, 2:])


@pytest.mark.parametrize("M", [1, 63, 127, 128, 129])
def test_assemble_b_batch_alone(M):
    """gpt_dev_sparse_assemble_b_batch from a G whose upper triangle is full: B, pre-filled with NaN, against the construction of the
    comment above the kernel, exactly, per element."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(M)
    nb, big = 2, 1e300
    bp, mg = (M + 128) // 128 * 128, (M + 64) // 64 * 64
    ldg = mg + 2
    G = rs.randint(-5, 6, size=(nb, mg + 1, ldg)).astype(float)
    ctx = _lib.Context()
    dG = torch.tensor(G, device="cuda")
    dB = torch.full((nb, bp * bp + 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_assemble_b_batch(ctx.handle, nb, dG.data_ptr(), ldg, (mg + 1) * ldg, M, dB.data_ptr(), bp,
                                                           bp * bp + 3, big))
    ctx.synchronize()
    got = dB.cpu().numpy()
    assert np.all(np.isnan(got[:, bp * bp:]))
    for b in range(nb):
        want = np.eye(bp)
        want[:M, :M] = np.tril(G[b, :M, :M]) + np.eye(M)
        want[M, :M] = G[b, M, :M]
        want[M, M] = big
        assert np.array_equal(got[b, :bp * bp].reshape(bp, bp), want), b


# ---- 8. strides and element offsets: the batched launchers against the single ones on padded layouts ------------------------------------
# The single and the batched launcher of each group run one kernel source; what a batch adds is an element stride per buffer.  Seeded data
# that is not integer, three elements, every stride a few rows or doubles above its lower bound, the gaps filled with a sentinel: every
# element carries the bits the single launcher gives on that element alone, and no gap changes.  (Inputs' gaps hold NaN: a read of one
# would show in the result.)
SENTINEL = -7.25


def _flat(nb, stride, fill):
    return np.full(nb * stride, fill, dtype=float)


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=float), device="cuda")


@pytest.mark.parametrize("rows,mg,nslices", [(5, 192, 0), (130, 128, 7), (257, 64, 0)])
def test_gram_batch_on_padded_strides_is_the_single_gram(rows, mg, nslices):
    """gpt_dev_sparse_gram_batch with vstride and gstride above rows x ldv and mg x ldg: element b of G equals gpt_dev_sparse_gram on that
    element's V bit for bit -- hence its upper tiles and the columns behind mg are what they were -- and the gaps between the elements
    of G keep the sentinel.  (5, 192): six tiles, two slices of four rows and of one; (130, 128, 7): seven slices, six of 20 rows and one of 10; (257, 64): one
    tile, the fit's slice count."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(1000 + rows + mg)
    nb, ldv, ldg = 3, mg + 64, mg + 8
    vstride, gstride = (rows + 3) * ldv + 5, (mg + 2) * ldg + 3
    V, G0 = _flat(nb, vstride, np.nan), _flat(nb, gstride, SENTINEL)
    for b in range(nb):
        V[b * vstride:b * vstride + rows * ldv] = rs.randn(rows * ldv)
        G0[b * gstride:b * gstride + mg * ldg] = rs.randn(mg * ldg)
    ctx = _lib.Context()
    dV, dG = _dev(V), _dev(G0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_gram_batch(ctx.handle, nb, dV.data_ptr(), ldv, vstride, rows, mg, nslices, dG.data_ptr(), ldg, gstride))
    ctx.synchronize()
    got = dG.cpu().numpy()
    low = np.zeros((mg, ldg), dtype=bool)
    low[:, :mg] = np.tril(np.ones((mg // 64, mg // 64))).repeat(64, 0).repeat(64, 1) > 0
    for b in range(nb):
        el, el0 = got[b * gstride:b * gstride + mg * ldg].reshape(mg, ldg), G0[b * gstride:b * gstride + mg * ldg].reshape(mg, ldg)
        assert np.all(got[b * gstride + mg * ldg:(b + 1) * gstride] == SENTINEL), b
        assert same_bits(el[~low], el0[~low]), b
        assert not same_bits(el[low], el0[low]), b
        d1, dVb = _dev(el0), _dev(V[b * vstride:b * vstride + rows * ldv])
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_gram(ctx.handle, dVb.data_ptr(), ldv, rows, mg, nslices, d1.data_ptr(), ldg))
        ctx.synchronize()
        assert same_bits(el, d1.cpu().numpy()), b


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 256, 257, 513])
def test_row_pass_batch_on_padded_strides_is_the_single_row_pass(M, method):
    """gpt_dev_sparse_lambda_batch with vstride, kstride, rstride and rvstride each above its lower bound (rows x ldv, rows, rows, 2 ldr):
    every element's rows, its two per-row values and its word equal gpt_dev_sparse_lambda's on the element alone, bit for bit; the
    gaps of V and of rowval and the word behind the last element keep their sentinel.  Row 2 of element 1 has a Lambda that is not
    positive (s_2 = -0.25 + 0.5^2 = 0, and k_2 far below q_2 for fitc): word 1 alone is raised, by both launchers.  M = 1: the r~ column
    next to one entry; 256 / 257 / 513: the edges of the row sum's two loops."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(2000 + 3 * M + method)
    nb, rows, ldr, ldv = 3, 5, 8, M + 3
    vstride, kstride, rstride, rvstride = (rows + 1) * ldv + 2, rows + 3, rows + 2, 2 * ldr + 5
    V, kd, r = _flat(nb, vstride, SENTINEL), _flat(nb, kstride, np.nan), _flat(nb, rstride, np.nan)
    for b in range(nb):
        Vb = rs.randn(rows, ldv)
        V[b * vstride:b * vstride + rows * ldv] = Vb.ravel()
        kd[b * kstride:b * kstride + rows] = (Vb[:, :M] ** 2).sum(1) + rs.uniform(0.5, 2.0, size=rows)
        r[b * rstride:b * rstride + rows] = rs.randn(rows)
    kd[1 * kstride + 2] = -1e6
    err = np.array([0.9, 0.8, 0.5, 0.7, 0.6])
    nv = np.array([0.3, -0.25, 1.7])
    ctx = _lib.Context()
    dV, dk, dr, de, dn = _dev(V), _dev(kd), _dev(r), _dev(err), _dev(nv)
    drow = _dev(_flat(nb, rvstride, SENTINEL))
    dbad = torch.zeros(nb + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_lambda_batch(ctx.handle, nb, dV.data_ptr(), ldv, vstride, rows, M, method, dk.data_ptr(), kstride,
                                                       dr.data_ptr(), rstride, de.data_ptr(), dn.data_ptr(), drow.data_ptr(), ldr, rvstride,
                                                       _ip(dbad)))
    ctx.synchronize()
    got, row, bad = dV.cpu().numpy(), drow.cpu().numpy(), dbad.cpu().numpy()
    assert np.array_equal(bad, [0, 1, 0, 0])
    for b in range(nb):
        assert np.all(got[b * vstride + rows * ldv:(b + 1) * vstride] == SENTINEL), b
        rb = row[b * rvstride:(b + 1) * rvstride]
        assert np.all(rb[rows:ldr] == SENTINEL) and np.all(rb[ldr + rows:] == SENTINEL), b
        dV1 = _dev(V[b * vstride:b * vstride + rows * ldv])
        d1 = _dev(np.full(2 * ldr, SENTINEL))
        b1 = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_lambda(ctx.handle, dV1.data_ptr(), ldv, rows, M, method, dk[b * kstride:].data_ptr(),
                                                     dr[b * rstride:].data_ptr(), de.data_ptr(), float(nv[b]), d1.data_ptr(), ldr, _ip(b1)))
        ctx.synchronize()
        assert same_bits(got[b * vstride:b * vstride + rows * ldv], dV1.cpu().numpy()), b
        assert same_bits(rb[:2 * ldr], d1.cpu().numpy()), b
        assert int(b1.cpu()[0]) == bad[b], b
    el1 = got[vstride:vstride + rows * ldv].reshape(rows, ldv)
    assert not el1[2, :M + 1].any() and el1[[0, 1, 3, 4], :M].all()          # the bad row is zeroed, its neighbours are scaled


@pytest.mark.parametrize("rows", [1, 257])
def test_rowsum_batch_on_padded_strides_is_the_single_rowsum(rows):
    """gpt_dev_sparse_rowsum_batch with rvstride above 2 ldr and astride = 4, as the fit lays its sums out: slots 0 and 1 of every
    element equal gpt_dev_sparse_rowsum's on the element alone bit for bit (onto what the slots held), slots 2 and 3 keep their sentinel.
    One row; one past the workgroup's 256 threads."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(3000 + rows)
    nb, ldr = 3, rows + 5
    rvstride = 2 * ldr + 7
    rv = rs.randn(nb * rvstride)
    acc0 = np.full((nb, 4), SENTINEL)
    acc0[:, :2] = rs.randn(nb, 2)
    ctx = _lib.Context()
    drow, dacc = _dev(rv), _dev(acc0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_rowsum_batch(ctx.handle, nb, drow.data_ptr(), ldr, rvstride, rows, dacc.data_ptr(), 4))
    ctx.synchronize()
    got = dacc.cpu().numpy()
    assert np.all(got[:, 2:] == SENTINEL)
    for b in range(nb):
        d1 = _dev(acc0[b, :2])
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_rowsum(ctx.handle, drow[b * rvstride:].data_ptr(), ldr, rows, d1.data_ptr()))
        ctx.synchronize()
        assert same_bits(got[b, :2], d1.cpu().numpy()) and not same_bits(got[b, :2], acc0[b, :2]), b


@pytest.mark.parametrize("M", [1, 127, 128])
def test_assemble_b_batch_on_padded_strides_is_the_single_assembly(M):
    """gpt_dev_sparse_assemble_b_batch with gstride above (M + 1) ldg and bstride above bp^2: every element's B equals
    gpt_dev_sparse_assemble_b's on the element's G bit for bit, the gaps between the elements of B keep their sentinel.  127: the
    augmented row is the last of the only 128-block; 128: it opens a second one."""
    import torch
    _lib = lib()
    rs = np.random.RandomState(4000 + M)
    nb, big = 3, 1e300
    bp, mg = (M + 128) // 128 * 128, (M + 64) // 64 * 64
    ldg = mg + 2
    gstride, bstride = (mg + 2) * ldg + 3, bp * bp + 5
    G = rs.randn(nb * gstride)
    ctx = _lib.Context()
    dG, dB = _dev(G), _dev(_flat(nb, bstride, SENTINEL))
    torch.cuda.synchronize()
    _lib.check(_lib.load().gpt_dev_sparse_assemble_b_batch(ctx.handle, nb, dG.data_ptr(), ldg, gstride, M, dB.data_ptr(), bp, bstride, big))
    ctx.synchronize()
    got = dB.cpu().numpy()
    for b in range(nb):
        assert np.all(got[b * bstride + bp * bp:(b + 1) * bstride] == SENTINEL), b
        d1 = _dev(np.full(bp * bp, SENTINEL))
        torch.cuda.synchronize()
        _lib.check(_lib.load().gpt_dev_sparse_assemble_b(ctx.handle, dG[b * gstride:].data_ptr(), ldg, M, d1.data_ptr(), bp, big))
        ctx.synchronize()
        one = d1.cpu().numpy()
        assert same_bits(got[b * bstride:b * bstride + bp * bp], one), b
        assert one[M * bp + M] == big and one[0] == G[b * gstride] + 1.0
