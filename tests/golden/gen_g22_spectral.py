#!/usr/bin/env python
"""g22_spectral.npz: values of one spectral-mixture component (Wilson & Adams 2013) and its derivatives from an independent
high-precision evaluation (mpmath, 80 digits) -- the statement tests/test_spectral_host.py and tests/test_gpu_spectral.py compare the
library's GPT_KERNEL_SPECTRAL with.  No reference code is involved (the reference has no such kernel); mpmath only.

    k(x, x') = sigma_f^2 exp(-sum_d tau_d^2 / (2 l_d^2)) cos(2 pi sum_d mu_d tau_d),   tau = x - x',
    d^ni/dx^ni d^nj/dx'^nj  k  =  (-1)^(sum nj) d^(ni + nj)/dtau^(ni + nj) k(tau),       params = [sigma_f, mu_1 .. mu_D, l_1 .. l_D].

Method: the CLOSED FORM above, as a function of the tau_d that carry an order, is differentiated by mpmath's numerical
differentiation with multivariate orders (mp.diff) -- nothing of the library's complex recurrence.  The kernel is not separable (one
cosine of the dot product), so the derivative is taken in all those dimensions at once.  l = inf is the envelope 1 in that dimension; an order on a dimension with mu = 0 and l = inf, which the closed form does not depend
on, is exactly 0 (a difference quotient would leave its rounding there).
mp.diff nests one central difference per dimension and multiplies its working precision by (order + 1) at every level -- over a
million bits for three dimensions of order 16 -- so the step is fixed at h = 2^-140 and the closed form is evaluated with at most
CAP = 8192 bits: the differences divide by at most (2 h)^48 = 2^-6672, which leaves more than 1500 good bits, and the truncation error
of a central difference, ~ h^2 f^(n+2) / f^(n), is below 1e-75 of the scale.

Coordinates are multiples of 2^-24, so that tau = x - x' is formed exactly in double precision and the comparison measures the
kernel's arithmetic, not the conditioning of its input.

Every entry carries its SCALE: sigma_f^2 times the product over the dimensions of the largest magnitude |H_n(tau)| exp(-a tau^2 / 2)
takes (a = 1 / l^2, H_n the polynomial with d^n/dtau^n exp(-a tau^2 / 2 + i w tau) = H_n exp(..), w = 2 pi mu), on a grid of 8193
points over |tau| <= 8 l; |w|^n for l = inf; 1 for n = 0.  It bounds the real part for any phase.  The derivatives have zeros, so a
deviation is measured against that scale, not against the value.  The scale is a yardstick found in double precision, not a
reference value.

Cases: D = 1, 2, 3 and one set at D = 16 (orders in at most three of its dimensions): every combined order 0 .. 16 per dimension,
on either or both points; tau = 0 rows; phases beyond 20 cycles; mu = 0; an infinite length scale beside a frequency (the pure
cosine in that dimension); a masked-out dimension (mu = 0, l = inf) with and without an order on it; negative frequencies.
About four minutes.
"""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 80
GRID = 2.0 ** -24
STEP = mp.ldexp(1, -140)
CAP = 8192


def k_deriv(params, D, tau, n):
    """d^n/dtau^n of the closed form at tau (multi-index n), 80 digits."""
    sf, mus, ls = params[0], params[1:1 + D], params[1 + D:]
    a = [mp.mpf(0) if np.isinf(l) else 1 / (mp.mpf(float(l)) * mp.mpf(float(l))) for l in ls]
    mu = [mp.mpf(float(m)) for m in mus]
    t = [mp.mpf(float(v)) for v in tau]
    act = [d for d in range(D) if n[d] > 0]
    if any(a[d] == 0 and mu[d] == 0 for d in act):
        return mp.mpf(0)                 # the closed form does not depend on that tau_d: its derivative is exactly 0

    def fun(*ts):
        tt = list(t)
        for d, v in zip(act, ts):
            tt[d] = v
        with mp.workprec(min(mp.mp.prec, CAP)):
            return mp.exp(-sum(a[d] * tt[d] ** 2 for d in range(D)) / 2) * mp.cos(2 * mp.pi * sum(mu[d] * tt[d] for d in range(D)))
    if not act:
        return mp.mpf(float(sf)) ** 2 * fun()
    if len(act) == 1:
        return mp.mpf(float(sf)) ** 2 * mp.diff(fun, t[act[0]], int(n[act[0]]), h=STEP)
    return mp.mpf(float(sf)) ** 2 * mp.diff(fun, tuple(t[d] for d in act), tuple(int(n[d]) for d in act), h=STEP)


_SCALES = {}


def h_scale(mu, l, n):
    """max over |tau| <= 8 l of |H_n(tau)| exp(-a tau^2 / 2) on 8193 points; |w|^n for l = inf; 1 for n = 0."""
    if n == 0:
        return 1.0
    w = 2.0 * np.pi * mu
    if np.isinf(l):
        return abs(w) ** n
    key = (float(mu), float(l), int(n))
    if key not in _SCALES:
        a = 1.0 / (l * l)
        tau = np.linspace(-8.0 * l, 8.0 * l, 8193)
        s = -a * tau + 1j * w
        hm, h = np.ones_like(s), s
        for m in range(1, n):
            hm, h = h, s * h - a * m * hm
        _SCALES[key] = float((np.abs(h) * np.exp(-0.5 * a * tau * tau)).max())
    return _SCALES[key]


def split(rs, tot, how):
    """A combined order as (ni, nj): all on the first point, all on the second, or shared."""
    if how == 0:
        return tot, 0
    if how == 1:
        return 0, tot
    a = int(rs.randint(0, tot + 1))
    return a, tot - a


def grid(v):
    return np.round(np.asarray(v, dtype=float) / GRID) * GRID


def entry(params, D, xi, xj, ni, nj):
    tau = [float(xi[d]) - float(xj[d]) for d in range(D)]
    for d in range(D):
        assert mp.mpf(tau[d]) == mp.mpf(float(xi[d])) - mp.mpf(float(xj[d])), "tau must be exact"
    n = [int(ni[d] + nj[d]) for d in range(D)]
    val = (-1) ** int(np.sum(nj)) * k_deriv(params, D, tau, n)
    scale = params[0] * params[0]
    for d in range(D):
        scale *= h_scale(params[1 + d], params[1 + D + d], n[d])
    return float(val), scale


def build_case(rs, D, params, orders, special=(), width=4.0):
    """orders: per pair, the combined order of every dimension; special: extra (xi, xj, ni, nj) rows; |tau| <= width l (l = inf: width)."""
    ls = np.asarray(params[1 + D:], dtype=float)
    ls = np.where(np.isinf(ls), 1.0, ls)
    rows = []
    for q, tot in enumerate(orders):
        xj = grid(rs.uniform(-2.0, 2.0, D))
        xi = grid(xj + ls * rs.uniform(-width, width, D))
        ni, nj = np.zeros(D, dtype=int), np.zeros(D, dtype=int)
        for d in range(D):
            ni[d], nj[d] = split(rs, int(tot[d]), q % 3)
        rows.append((xi, xj, ni, nj))
    rows += [tuple(np.asarray(v) for v in r) for r in special]
    out = {"params": np.array(params, dtype=float), "Xi": np.array([r[0] for r in rows], dtype=float),
           "Xj": np.array([r[1] for r in rows], dtype=float), "ni": np.array([r[2] for r in rows], dtype=np.int32),
           "nj": np.array([r[3] for r in rows], dtype=np.int32)}
    ks = [entry(params, D, *r) for r in rows]
    out["k"], out["scale"] = np.array([v[0] for v in ks]), np.array([v[1] for v in ks])
    return out


def main():
    rs = np.random.RandomState(2222)
    cases = []
    # D = 1: every combined order 0 .. 16, two pairs each, three parameter sets [sigma_f, mu, l] -- a moderate frequency, mu = 0 (the
    # squared exponential) and a high one (|tau| up to 12: up to 150 cycles); tau = 0 rows at even and odd orders
    for params in ([1.3, 0.75, 0.7], [0.8, 0.0, 2.5], [1.1, 12.5, 3.0]):
        orders = [[t] for t in range(17) for _ in range(2)]
        special = []
        if params[1] == 0.75:
            for t in (0, 1, 2, 3, 4, 8, 15, 16):
                a = t // 2
                special.append(([0.625], [0.625], [a], [t - a]))                       # tau = 0
        cases.append((1, build_case(rs, 1, params, orders, special)))
    # D = 2: orders in one or both dimensions, one negative frequency
    orders = [[rs.randint(0, 17), rs.randint(0, 17)] for _ in range(60)] + [[16, 16], [0, 16], [16, 0], [1, 1], [2, 1], [0, 0]]
    cases.append((2, build_case(rs, 2, [1.2, 0.9, -1.4, 0.6, 1.4], orders,
                                [([0.5, -1.0], [0.5, -1.0], [1, 0], [1, 2]), ([0.5, 1.0], [0.5, -1.0], [2, 1], [0, 1])])))
    # D = 2 with the second dimension masked out (mu = 0, l = inf, as MaskedKernel hands it over): without and with an order on it
    orders = [[rs.randint(0, 17), 0] for _ in range(12)] + [[rs.randint(0, 9), rs.randint(1, 5)] for _ in range(8)]
    cases.append((2, build_case(rs, 2, [0.9, 1.25, 0.0, 0.8, np.inf], orders)))
    # D = 2 with an infinite length scale beside a frequency: the pure cosine in the first dimension (|tau_1| <= 4: up to 28 cycles)
    orders = [[rs.randint(0, 17), rs.randint(0, 17) if rs.rand() < 0.5 else 0] for _ in range(30)]
    cases.append((2, build_case(rs, 2, [0.9, 7.0, -0.5, np.inf, 0.8], orders)))
    # D = 3
    orders = [[rs.randint(0, 17) if rs.rand() < 0.6 else 0 for _ in range(3)] for _ in range(60)]
    cases.append((3, build_case(rs, 3, [1.05, 0.5, -1.1, 2.2, 0.6, 1.7, 4.0], orders)))
    # D = 3, high frequencies of both signs: the phase runs to hundreds of cycles
    orders = [[rs.randint(0, 17) if rs.rand() < 0.5 else 0 for _ in range(3)] for _ in range(40)]
    cases.append((3, build_case(rs, 3, [0.7, 9.0, -7.0, 11.0, 2.0, 1.5, 2.5], orders)))
    # D = 16: values, and orders in up to three of the dimensions
    mus, ls = list(np.round(rs.uniform(-1.0, 1.0, 16), 3)), list(np.round(rs.uniform(0.8, 4.0, 16), 3))
    orders = []
    for q in range(24):
        o = [0] * 16
        for d in rs.choice(16, q % 4, replace=False):
            o[d] = int(rs.randint(1, 17))
        orders.append(o)
    cases.append((16, build_case(rs, 16, [1.15] + mus + ls, orders, width=1.0)))
    out = {"ncases": np.int64(len(cases))}
    for ci, (D, c) in enumerate(cases):
        out["c%d_D" % ci] = np.int64(D)
        for k, v in c.items():
            out["c%d_%s" % (ci, k)] = v
        ok = c["scale"] > 0
        print("case %d: D = %d, %d pairs, largest |k| / scale = %.3g" % (ci, D, len(c["k"]), np.abs(c["k"][ok] / c["scale"][ok]).max()),
              flush=True)
    np.savez_compressed(os.path.join(HERE, "g22_spectral.npz"), **out)
    print("wrote g22_spectral.npz")


if __name__ == "__main__":
    main()
