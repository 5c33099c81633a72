"""Option skip_pad_rows (default on): the trailing updates of a fit leave out the padding rows of the augmented factor of order
NP = round_up(N + 1, 128) -- the tiles that start below the augmented row N are not launched, and the tile row that holds row N reads and
stores nothing below it (gemm.hip gemm_launch_t, tile_order.hpp, api_schedule.inc potrf_enqueue).

The shapes are the smallest that take the merged, table-ordered launch (>= 512 tiles of 64 x 64) in each panel-width class: base
B = 2560 (panel width 256, first update 2304 rows = 666 tiles) and B = 5120 (NP = 5248, the first order of the 384 class).  Around
B = 2560 the orders walk the augmented row through a tile row: B - 1 and B + 127 have no padding row at all (the limit is a no-op),
B a thin tile row (one live row in 64) and a dropped one, B + 15 / B + 16 and B + 31 / B + 32 move the limit across the 16-row fragments
and the 32-row wave rows (and tile rows of the 32 x 32 kernel) inside a tile, B + 63 / B + 64 end a full tile row and start the next thin one.

Every case against the CPU oracle (ll_data and logdet_half to the 1e-8 relative gate of the full-size tests, alpha to the
2e-7 max|alpha| of the eager-alpha tests) and, in the same process, against the same library with the option off: equal floats, and
L, alpha, a solve and a predict equal bit for bit."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = sys.float_info.epsilon
KID_M52 = 1
D = 3
P = np.array([1.0, 0.3, 0.3, 0.3])
B1, B2 = 2560, 5120
ORDERS = [B1 - 1, B1, B1 + 15, B1 + 16, B1 + 31, B1 + 32, B1 + 63, B1 + 64, B1 + 127, B2, B2 + 16, B2 + 64]
VARIANTS = [{"lookahead": 0}, {"tile": 32}, {"edge_flags": 0}, {"tail_wait": 0}, {"eager_alpha": 1}, {"eager_alpha": 0}]


def inputs(N, seed=1234):
    """bench.synth-style data, C3 pattern: the last quarter of the rows are first-derivative observations."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    s = X.sum(1)
    n = np.zeros((N, D), dtype=int)
    y = np.sin(s)
    for i in range(3 * N // 4, N):
        n[i, i % D] = 1
        y[i] = np.cos(s[i])
    return X, n, y + 0.05 * rs.randn(N)


def evaluate(c, N, X, n, y, err):
    """One fit and everything that reads the factor: (ll_data, logdet_half), L, alpha, a solve, a predict with std."""
    rs = np.random.RandomState(N + 7)
    rhs = rs.randn(N, 2)
    Xs, ns = rs.rand(16, D), np.zeros((16, D), dtype=np.int32)
    ll, ld = c.fit(KID_M52, P, 0.0, y, err, 1e2 * EPS)
    mean, std, _ = c.predict(Xs, ns, 1)
    return {"ll": ll, "ld": ld, "L": c.get_L(N), "alpha": c.get_alpha(N), "solve": c.cho_solve(rhs.copy()), "mean": mean, "std": std}


def assert_same_bits(on, off, what):
    assert on["ll"] == off["ll"] and on["ld"] == off["ld"], (what, on["ll"], off["ll"], on["ld"], off["ld"])
    for key in ("L", "alpha", "solve", "mean", "std"):
        assert np.array_equal(on[key], off[key]), "%s: %s differs from the option-off result" % (what, key)


@pytest.fixture
def ctx():
    from gptools_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("N", ORDERS)
def test_skipped_pad_rows_against_the_oracle_and_the_full_updates(oracle, ctx, N):
    X, n, y = inputs(N)
    err = 0.05 * np.ones(N)
    ref = oracle.fit("m52", P, X, n, y, err, chol="scipy")
    ctx.set_data(X, n)
    out = {}
    for mode in (1, 0):
        ctx.set_option("skip_pad_rows", mode)
        out[mode] = evaluate(ctx, N, X, n, y, err)
    on, off = out[1], out[0]
    ll_err = abs(on["ll"] - ref["ll_data"]) / abs(ref["ll_data"])
    ld_err = abs(on["ld"] - ref["logdet_half"]) / abs(ref["logdet_half"])
    a_err = np.abs(on["alpha"] - ref["alpha"]).max() / np.abs(ref["alpha"]).max()
    print("N = %d: ll rel. err %.3g, logdet rel. err %.3g, alpha err / max|alpha| %.3g" % (N, ll_err, ld_err, a_err))
    assert ll_err <= 1e-8 and ld_err <= 1e-8
    assert a_err <= 2e-7
    assert_same_bits(on, off, "N = %d" % N)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join("%s=%d" % kv for kv in sorted(v.items())))
@pytest.mark.parametrize("N", [B1, B1 + 16])
def test_skipped_pad_rows_under_the_schedule_variants(ctx, N, variant):
    """The one-stream loop, forced 32 x 32 tiles, the event schedule (urgent and rest as separate
    launches), the wait kernel in place of the tail wait, and eager alpha on and off: the same bits with the option on and off."""
    X, n, y = inputs(N)
    err = 0.05 * np.ones(N)
    ctx.set_data(X, n)
    for key, value in variant.items():
        ctx.set_option(key, value)
    out = {}
    for mode in (1, 0):
        ctx.set_option("skip_pad_rows", mode)
        out[mode] = evaluate(ctx, N, X, n, y, err)
    assert np.isfinite(out[1]["ll"]) and np.isfinite(out[1]["L"]).all()
    assert_same_bits(out[1], out[0], "N = %d, %r" % (N, variant))


def test_a_failed_pivot_is_reported_alike(ctx):
    """A seeded SPD matrix of order B with one diagonal entry made negative fails at that pivot: the same status and the same
    reported leading minor with the option on and off."""
    N, bad = B1, 2000
    rs = np.random.RandomState(5)
    G = rs.randn(N, 64)
    K = G.dot(G.T) / 64.0 + np.eye(N)
    y = rs.randn(N)
    ctx.set_option("skip_pad_rows", 1)
    ll_ok = ctx.fit_matrix(K, y)
    assert np.isfinite(ll_ok[0])
    K[bad, bad] = -1.0
    msgs = []
    for mode in (1, 0):
        ctx.set_option("skip_pad_rows", mode)
        with pytest.raises(np.linalg.LinAlgError) as ei:
            ctx.fit_matrix(K, y)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]
    assert msgs[0].startswith("%d-th leading minor" % (bad + 1)), msgs[0]
