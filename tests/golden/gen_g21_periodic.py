#!/usr/bin/env python
"""g21_periodic.npz: values of the periodic (exp-sine-squared) kernel and its derivatives from an independent high-precision
evaluation (mpmath, 60 digits) -- the statement tests/test_periodic_host.py and tests/test_gpu_periodic.py compare the library's
GPT_KERNEL_PERIODIC with.  No reference code is involved (the reference has no such kernel); mpmath only.

    k(x, x') = sigma_f^2 prod_d f_d(tau_d),   f_d(tau) = exp(-2 sin^2(pi tau / p_d) / l_d^2),   tau = x - x',
    d^ni/dx^ni d^nj/dx'^nj  k  =  sigma_f^2 prod_d (-1)^nj_d f_d^(ni_d + nj_d)(tau_d).

Method: the kernel is separable, so an entry is a product of one-dimensional derivatives, each taken by mpmath's numerical
differentiation (mp.diff) of f_d itself -- nothing of the library's recurrence.  A dimension with l = inf is the constant 1: its
derivatives are exactly 0.

Coordinates are multiples of 2^-24, so that tau = x - x' is formed exactly in double precision and the comparison measures the
kernel's arithmetic, not the conditioning of its input.

Every entry carries its SCALE: sigma_f^2 times the product over the dimensions of the largest magnitude |f_d^(n_d)| takes over one
period (1 for a dimension without an order in it or with l = inf).  The derivatives have zeros, so a deviation is measured against
that scale, not against the value.  The scale is found on a grid of 4096 points per period in double precision (it is a yardstick,
not a reference value).

Cases: D = 1, 2, 3 (combined orders 0 .. 16 per dimension, on either or both points; tau = 0 rows; tau an exact multiple of the
period; |tau| up to four periods; D = 2 with one infinite length scale) and one set at D = 16.  ~1 minute.
"""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 60
GRID = 2.0 ** -24


def f_deriv(l, p, tau, n):
    """f^(n)(tau) for one dimension, 60 digits."""
    if np.isinf(l):
        return mp.mpf(1) if n == 0 else mp.mpf(0)
    a, w = 1 / (mp.mpf(l) * mp.mpf(l)), mp.pi / mp.mpf(p)
    fun = lambda t: mp.exp(-2 * a * mp.sin(w * t) ** 2)
    return fun(mp.mpf(tau)) if n == 0 else mp.diff(fun, mp.mpf(tau), n)


_SCALES = {}


def f_scale(l, p, n):
    """max over one period of |f^(n)|: the recurrence P_(m+1) = sum_k C(m, k) g^(k+1) P_(m-k) on a grid, double precision."""
    if n == 0 or np.isinf(l):
        return 1.0
    key = (float(l), float(p), int(n))
    if key not in _SCALES:
        from math import comb
        a, w = 1.0 / (l * l), 2.0 * np.pi / p
        th = np.linspace(0.0, 2.0 * np.pi, 4096, endpoint=False)
        G = [None] + [a * w ** k * np.cos(th + 0.5 * np.pi * k) for k in range(1, n + 1)]
        P = [np.ones_like(th)]
        for m in range(n):
            P.append(sum(comb(m, k) * G[k + 1] * P[m - k] for k in range(m + 1)))
        _SCALES[key] = float(np.abs(np.exp(a * (np.cos(th) - 1.0)) * P[n]).max())
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
    sf, ls, ps = params[0], params[1:1 + D], params[1 + D:]
    val, scale = mp.mpf(sf) ** 2, sf * sf
    for d in range(D):
        n = int(ni[d] + nj[d])
        tau = float(xi[d]) - float(xj[d])
        assert mp.mpf(tau) == mp.mpf(float(xi[d])) - mp.mpf(float(xj[d])), "tau must be exact"
        val *= (-1) ** int(nj[d]) * f_deriv(ls[d], ps[d], tau, n)
        scale *= f_scale(ls[d], ps[d], n)
    return float(val), scale


def build_case(rs, D, params, orders, special=()):
    """orders: per pair, the combined order of every dimension; special: extra (xi, xj, ni, nj) rows."""
    ps = np.asarray(params[1 + D:], dtype=float)
    rows = []
    for q, tot in enumerate(orders):
        xj = grid(rs.uniform(-2.0, 2.0, D))
        xi = grid(xj + ps * rs.uniform(-4.0, 4.0, D))            # |tau| up to four periods
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
    rs = np.random.RandomState(2121)
    cases = []
    # D = 1: every combined order 0 .. 16, six pairs each (two per way of sharing it), three parameter sets; then tau = 0 and
    # tau = k p rows (p = 0.75 and k p are exact) at the even and odd orders
    for params in ([1.3, 0.7, 0.75], [0.8, 2.5, 3.0], [1.1, 0.25, 0.4]):
        orders = [[t] for t in range(17) for _ in range(2)]
        special = []
        if params[2] == 0.75:
            for t in (0, 1, 2, 3, 4, 8, 15, 16):
                a = t // 2
                special.append(([0.625], [0.625], [a], [t - a]))                       # tau = 0
                special.append(([0.625 + 3 * 0.75], [0.625], [t - a], [a]))            # tau = 3 p
                special.append(([0.625], [0.625 + 5 * 0.75], [a], [t - a]))            # tau = -5 p
        cases.append((1, build_case(rs, 1, params, orders, special)))
    # D = 2: orders in one or both dimensions
    orders = [[rs.randint(0, 17), rs.randint(0, 17)] for _ in range(60)] + [[16, 16], [0, 16], [16, 0], [1, 1], [2, 1], [0, 0]]
    cases.append((2, build_case(rs, 2, [1.2, 0.6, 1.4, 0.9, 2.0], orders,
                                [([0.5, -1.0], [0.5, -1.0], [1, 0], [1, 2]), ([0.5, 1.0], [0.5, -1.0], [2, 1], [0, 1])])))
    # D = 2 with an infinite length scale in the second dimension (period 1 there, as MaskedKernel hands it over)
    orders = [[rs.randint(0, 17), 0] for _ in range(12)] + [[rs.randint(0, 9), rs.randint(1, 5)] for _ in range(8)]
    cases.append((2, build_case(rs, 2, [0.9, 0.8, np.inf, 1.25, 1.0], orders)))
    # D = 3
    orders = [[rs.randint(0, 17) if rs.rand() < 0.6 else 0 for _ in range(3)] for _ in range(60)]
    cases.append((3, build_case(rs, 3, [1.05, 0.5, 1.1, 2.2, 0.6, 1.7, 4.0], orders)))
    # D = 16: values, and orders in up to three of the dimensions
    ls, ps = list(np.round(rs.uniform(0.8, 4.0, 16), 3)), list(np.round(rs.uniform(0.5, 4.0, 16), 3))
    orders = []
    for q in range(24):
        o = [0] * 16
        for d in rs.choice(16, q % 4, replace=False):
            o[d] = int(rs.randint(1, 17))
        orders.append(o)
    cases.append((16, build_case(rs, 16, [1.15] + ls + ps, orders)))
    out = {"ncases": np.int64(len(cases))}
    for ci, (D, c) in enumerate(cases):
        out["c%d_D" % ci] = np.int64(D)
        for k, v in c.items():
            out["c%d_%s" % (ci, k)] = v
        print("case %d: D = %d, %d pairs, largest |k| / scale = %.3g" % (ci, D, len(c["k"]), np.abs(c["k"] / c["scale"]).max()), flush=True)
    np.savez_compressed(os.path.join(HERE, "g21_periodic.npz"), **out)
    print("wrote g21_periodic.npz")


if __name__ == "__main__":
    main()
