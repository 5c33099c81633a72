"""The host's yardstick of the sparse-gradient tests (tests/test_sparse_grad_host.py, tests/test_gpu_sparse_grad.py).

Not a test module.  The input sets and covariance blocks are those of tests/sparse_cases.py; this module restates the gradient of the
FITC / VFE / DTC objective in numpy / LAPACK, twice:

* ``adjoints`` + ``contract``: the adjoint form the library evaluates --
      t = L_B^-T c, beta = L_u^-T t, alpha_i = (r_i - v_i.t) / Lambda_i, w_i = L_B^-1 v_i,
      W_ii = alpha_i^2 - 1/Lambda_i + |w_i|^2 / Lambda_i^2, e_i = W_ii (fitc), -1/s_i (vfe), 0 (dtc),
      g_i = W_ii / 2 (+ (k_i - q_i) / (2 s_i^2), vfe),
      A_fu[i,:] = alpha_i beta^T - (1/Lambda_i) v_i^T B^-1 L_u^-1 - e_i v_i^T L_u^-1,
      A_uu = -1/2 (beta beta^T - L_u^-T (I - B^-1 + V diag(e) V^T) L_u^-1),
      d ll = sum A_uu dK_uu + sum A_fu dK_fu + 1/2 sum e_i dk_i + sum g_i ds_i;
* ``dense_gradient``: 1/2 tr((alpha alpha^T - Sigma^-1) dSigma) with N x N matrices and (K_uu + jitter I)^-1 by LU, as
  sparse_cases.dense -- the guard of the restated formulas themselves.

The yardstick of a device gradient of an SE model is the project's own (tests/test_gpu_grad_diff.py, ORACLE_DIFF_ERR and ten times
it): the adjoint form contracted with the CPU oracle's blocks differenced per pair at theta -+ eps, eps = 6e-6 max(1, |theta|),
against the same adjoint form contracted with the oracle's exact dK (its hyper_deriv), relative to the largest kernel-parameter
entry.  DIFF_ERR holds that figure per input set, the largest over the set's methods and parameters (rule (b) of DESIGN.md 18.5:
never one draw), measured on the CPU by tests/test_sparse_grad_host.py, which prints it.
"""
import numpy as np
import scipy.linalg

import sparse_cases as S

REL_STEP = 6e-6

#: the SE input sets of the device test: name -> chunk_rows values (None: the default)
SE_CASES = {"se_300": (None, 128), "se_m63": (64,), "se_m64": (64,), "se_m127": (64,), "se_m128": (64,), "se3_130": (64,), "se1_64": (None,)}
METHODS = ("fitc", "vfe", "dtc")


def blocks_at(O, name, terms, hyper_deriv=None):
    """K_uu, K_uf and k_i of a case's points for the model ``terms`` (one plain term with ``hyper_deriv``)."""
    d = S.case_data(name)
    if hyper_deriv is None:
        return dict(Kuu=S.gram(O, terms, d["Z"], d["nZ"], d["Z"], d["nZ"]), Kuf=S.gram(O, terms, d["Z"], d["nZ"], d["X"], d["n"]),
                    kd=S.kdiag(O, terms, d["X"], d["n"]))
    (kern, p), = terms

    def kb(Xi, ni, Xj, nj):
        return O.kbuild(kern, p, Xi, ni, Xj, nj, hyper_deriv=hyper_deriv)
    return dict(Kuu=kb(d["Z"], d["nZ"], d["Z"], d["nZ"]), Kuf=kb(d["Z"], d["nZ"], d["X"], d["n"]),
                kd=np.array([kb(d["X"][i:i + 1], d["n"][i:i + 1], d["X"][i:i + 1], d["n"][i:i + 1])[0, 0] for i in range(len(d["X"]))]))


def adjoints(b, r, s, method, jitter=S.JITTER):
    """alpha, e, g, A_fu (N x M) and A_uu (M x M) of the formulas above, from the Woodbury route's factors."""
    M = b["Kuu"].shape[0]
    Lu = scipy.linalg.cholesky(b["Kuu"] + jitter * np.eye(M), lower=True)
    V = scipy.linalg.solve_triangular(Lu, b["Kuf"], lower=True)
    q = (V ** 2).sum(0)
    kmq = b["kd"] - q
    lam = kmq + s if method == "fitc" else s.copy()
    B = np.eye(M) + (V / lam).dot(V.T)
    LB = scipy.linalg.cholesky(B, lower=True)
    c = scipy.linalg.solve_triangular(LB, V.dot(r / lam), lower=True)
    t = scipy.linalg.solve_triangular(LB, c, lower=True, trans="T")
    beta = scipy.linalg.solve_triangular(Lu, t, lower=True, trans="T")
    alpha = (r - V.T.dot(t)) / lam
    W = scipy.linalg.solve_triangular(LB, V, lower=True)
    wii = alpha ** 2 - 1.0 / lam + (W ** 2).sum(0) / lam ** 2
    e = wii if method == "fitc" else (-1.0 / s if method == "vfe" else np.zeros_like(s))
    g = 0.5 * wii + (0.5 * kmq / s ** 2 if method == "vfe" else 0.0)
    LuI = scipy.linalg.solve_triangular(Lu, np.eye(M), lower=True)
    Binv = scipy.linalg.cho_solve((LB, True), np.eye(M))
    Afu = np.outer(alpha, beta) - (V / lam).T.dot(Binv).dot(LuI) - (V * e).T.dot(LuI)
    mid = np.eye(M) - Binv + (V * e).dot(V.T)
    Auu = -0.5 * (np.outer(beta, beta) - LuI.T.dot(mid).dot(LuI))
    return dict(alpha=alpha, e=e, g=g, Afu=Afu, Auu=Auu, lam=lam)


def contract(adj, dKuu, dKuf, dkd):
    """sum A_uu dK_uu + sum A_fu dK_fu + 1/2 sum e_i dk_i"""
    return (adj["Auu"] * dKuu).sum() + (adj["Afu"] * dKuf.T).sum() + 0.5 * adj["e"].dot(dkd)


def dense_gradient(b, r, s, method, dKuu, dKuf, dkd, dnoise, jitter=S.JITTER):
    """d ll along (dK_uu, dK_uf, dk, d noise_var = dnoise) by the dense route: Sigma = Q_ff + Lambda whole, its inverse whole."""
    M, N = b["Kuf"].shape
    KiKuf = np.linalg.solve(b["Kuu"] + jitter * np.eye(M), b["Kuf"])
    Qff = b["Kuf"].T.dot(KiKuf)
    kmq = b["kd"] - np.diag(Qff)
    lam = kmq + s if method == "fitc" else s.copy()
    Si = np.linalg.inv(Qff + np.diag(lam))
    alpha = Si.dot(r)
    dQ = dKuf.T.dot(KiKuf) + KiKuf.T.dot(dKuf) - KiKuf.T.dot(dKuu).dot(KiKuf)
    dlam = np.full(N, float(dnoise)) + (dkd - np.diag(dQ) if method == "fitc" else 0.0)
    dS = dQ + np.diag(dlam)
    out = 0.5 * (alpha.dot(dS).dot(alpha) - (Si * dS).sum())
    if method == "vfe":
        out += -0.5 * ((dkd - np.diag(dQ)) / s).sum() + 0.5 * (kmq / s ** 2).sum() * dnoise
    return out


def stencil(theta, h, rel_step=REL_STEP):
    eps = rel_step * max(1.0, abs(theta[h]))
    ta, tb = list(theta), list(theta)
    ta[h] -= eps
    tb[h] += eps
    return ta, tb, tb[h] - ta[h]


def se_gradients(O, name, method):
    """(exact, differenced, dense, noise entries) of an SE case: the kernel-parameter entries of the adjoint form with the oracle's
    exact dK, the same with its blocks differenced per pair, the dense route with the exact dK; and (sum g_i, dense d/d noise_var)."""
    c, d = S.CASES[name], S.case_data(name)
    (kern, theta), = c["terms"]
    assert kern == "se"
    s = S.NOISE ** 2.0 + d["err_y"] ** 2.0
    b = blocks_at(O, name, c["terms"])
    adj = adjoints(b, d["y"], s, method)
    exact, diff, dens = [], [], []
    for h in range(len(theta)):
        dk = blocks_at(O, name, c["terms"], hyper_deriv=h)
        exact.append(contract(adj, dk["Kuu"], dk["Kuf"], dk["kd"]))
        dens.append(dense_gradient(b, d["y"], s, method, dk["Kuu"], dk["Kuf"], dk["kd"], 0.0))
        ta, tb, den = stencil(theta, h)
        ba, bb = blocks_at(O, name, [(kern, ta)]), blocks_at(O, name, [(kern, tb)])
        diff.append(contract(adj, bb["Kuu"] - ba["Kuu"], bb["Kuf"] - ba["Kuf"], bb["kd"] - ba["kd"]) / den)
    zero = dict(Kuu=0.0 * b["Kuu"], Kuf=0.0 * b["Kuf"], kd=0.0 * b["kd"])
    noise = (adj["g"].sum(), dense_gradient(b, d["y"], s, method, zero["Kuu"], zero["Kuf"], zero["kd"], 1.0))
    return np.array(exact), np.array(diff), np.array(dens), noise, adj


def bound(name):
    """What a device kernel-parameter entry of an SE case may differ from the exact one by, relative to the largest exact entry:
    ten times the host's own differencing error at that input set (the ten covers the device's other summation order)."""
    return 10.0 * DIFF_ERR[name]


#: the host's differencing error per input set: max over methods and kernel parameters of |differenced - exact| / max|exact|,
#: measured on the CPU by tests/test_sparse_grad_host.py::test_differencing_error (which prints this table and asserts its entries)
DIFF_ERR = {
    "se1_64": 1.41e-10,
    "se3_130": 1.5e-09,
    "se_300": 1.7e-07,
    "se_m127": 4.04e-08,
    "se_m128": 4.02e-08,
    "se_m63": 1.83e-08,
    "se_m64": 1.44e-08,
}
