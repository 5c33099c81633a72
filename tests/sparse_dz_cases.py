"""The host's yardstick of the inducing-input gradient (tests/test_sparse_dz_host.py, tests/test_gpu_sparse_dz.py).

Not a test module.  The input sets and covariance blocks are those of tests/sparse_cases.py, the adjoints A_fu and A_uu those of
tests/sparse_grad_cases.py.  The gradient of the FITC / VFE / DTC objective with respect to coordinate d of inducing input z_m
 needs no differences: the derivative of a covariance entry with respect to z_{m,d} is the kernel with that
point's derivative order raised by one in dimension d, which the CPU oracle's builder evaluates,

    dZ[m,d] = sum_i A_fu[i,m] k(x_i, z_m; n_i, n_m + e_d) + 2 sum_{m' != m} A_uu[m',m] k(z_m', z_m; n_m', n_m + e_d).

The pair m' = m is left out: K_uu[m,m] does not depend on z_m.  ``dense_entry`` is the guard of that form: the same coordinate by
sparse_grad_cases.dense_gradient (N x N matrices, an LU solve), with dK_uf and dK_uu carrying the coordinate's row and column only.

DZ_ERR holds the discrepancy of the two per input set, the largest over the set's methods and the sampled coordinates relative to
max|dZ| (rule (b) of DESIGN.md 18.5: the largest of a group, never one draw), measured on the CPU by tests/test_sparse_dz_host.py,
which prints it; a device entry is held to ten times it, never below sparse_cases.floor(N).
"""
import numpy as np

import sparse_cases as S
import sparse_grad_cases as SG

#: the input sets of the host and the device test: name -> chunk_rows values of the device test (None: the default)
CASES = {"se_300": (None, 128), "se_m63": (64,), "se_m64": (64,), "se_m127": (64,), "se_m128": (64,), "se3_130": (64,), "se1_64": (None,),
         "rq_257": (64,), "sum_m257": (128,)}
SAMPLE = 8


def raised(O, name):
    """Per dimension d the blocks at the raised orders: (k(z_m, x_i; n_m + e_d, n_i), M x N, and k(z_m, z_m'; n_m + e_d, n_m'), M x M)."""
    c, d = S.CASES[name], S.case_data(name)
    out = []
    for dim in range(c["d"]):
        up = d["nZ"].copy()
        up[:, dim] += 1
        out.append((S.gram(O, c["terms"], d["Z"], up, d["X"], d["n"]), S.gram(O, c["terms"], d["Z"], up, d["Z"], d["nZ"])))
    return out


def setup(O, name, method):
    """(blocks, s, adjoints, raised blocks) of a case."""
    c, d = S.CASES[name], S.case_data(name)
    b = SG.blocks_at(O, name, c["terms"])
    s = S.NOISE ** 2.0 + d["err_y"] ** 2.0
    return b, s, SG.adjoints(b, d["y"], s, method), raised(O, name)


def exact_dz(adj, up):
    """The host's exact dZ (M x D) from the adjoints and the raised blocks."""
    M = adj["Auu"].shape[0]
    dz = np.zeros((M, len(up)))
    off = 1.0 - np.eye(M)
    for dim, (dKuf, dKuu) in enumerate(up):
        dz[:, dim] = (adj["Afu"].T * dKuf).sum(1) + 2.0 * (adj["Auu"].T * dKuu * off).sum(1)
    return dz


def dense_entry(b, r, s, method, up, m, dim):
    """d ll / d z_{m,dim} by the dense route: dK_uf and dK_uu hold the row and the column of that coordinate, a zero diagonal entry."""
    dKuf_row, dKuu_row = up[dim][0][m], up[dim][1][m].copy()
    dKuu_row[m] = 0.0
    dKuf, dKuu = np.zeros_like(b["Kuf"]), np.zeros_like(b["Kuu"])
    dKuf[m, :] = dKuf_row
    dKuu[m, :] = dKuu_row
    dKuu[:, m] = dKuu_row
    return SG.dense_gradient(b, r, s, method, dKuu, dKuf, np.zeros_like(b["kd"]), 0.0)


def sample(dz, seed=5):
    """SAMPLE coordinates (m, d) at least (all of them where dZ has fewer): the two of largest |dZ| and seeded others."""
    flat = np.argsort(-np.abs(dz).ravel())
    pick = list(flat[:2])
    rest = np.random.RandomState(seed).permutation(flat[2:])
    pick += list(rest[:max(0, SAMPLE - len(pick))])
    return [np.unravel_index(int(i), dz.shape) for i in pick]


def bound(name):
    """What a device entry may differ from the host's exact one by, relative to max|dZ|: ten times the host's own discrepancy at that
    input set (the ten covers the device's other summation order), never below the floor of sparse_cases."""
    return max(10.0 * DZ_ERR[name], S.floor(S.CASES[name]["N"]))


#: the host's discrepancy per input set: max over methods and sampled coordinates of |exact form - dense route| / max|dZ|, measured on
#: the CPU by tests/test_sparse_dz_host.py::test_host_form_against_the_dense_route (which prints this table and asserts its entries)
DZ_ERR = {
    "rq_257": 1.15e-10,
    "se1_64": 3.57e-14,
    "se3_130": 2.72e-10,
    "se_300": 2.27e-10,
    "se_m127": 2.25e-10,
    "se_m128": 1.18e-09,
    "se_m63": 9.31e-10,
    "se_m64": 2.72e-10,
    "sum_m257": 2.34e-10,
}
