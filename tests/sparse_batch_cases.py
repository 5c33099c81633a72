"""The elements and the host's yardstick of the batched sparse-fit tests (tests/test_sparse_batch_host.py,
tests/test_gpu_sparse_batch.py).

Not a test module.  The input sets are those of sparse_cases.CASES, unchanged; a case becomes a batch of five ELEMENTS:
element 0 has the case's own kernel parameters, elements 1 ... 4 have every kernel parameter multiplied by a draw of
RandomState(211).uniform(0.85, 1.2) -- one generator per case, drawn element by element, term by term in order, a product term's
first factor before its second -- and the noise sigma is NOISE x (1, 0.7, 1.5, 1.0, 2.0).

The yardstick is sparse_cases' own: its Woodbury and dense routes on blocks from the CPU oracle's builder at each element's parameters.
Their discrepancy, measured on the CPU by tests/test_sparse_batch_host.py, is HOST_ERR_BATCH[(name, method, b)]; a device figure is held
to ten times the largest of its group ("fit": ll and the four sums; "trace": the VFE trace term) over the methods AND the elements of
the case, never below sparse_cases.floor(N) -- the convention of sparse_cases.bound.

Ceilings of the table.  Every figure of the fit group is held to the 1e-10 of sparse_cases.HOST_ERR.  The VFE trace figure is held to
1e-9, not 1e-10: sum_i (k_i - q_i) / s_i cancels in k_i - q_i and 1 / s_i amplifies what is left, and at the smaller noise levels of
the elements (sigma 0.07: 1 / s_i up to 190) the two routes differ by up to 2e-10 (se_m127, sum_m257, rq_257) -- the figure's own
scale, a property of the conditioning and not of either route.  All Lambda_i are positive at every element.
"""
import numpy as np

import sparse_cases as S

#: the cases of the batched tests: name -> what it exercises
BATCH_CASES = ("se1_64", "se_300", "rq_257", "se_m127", "se_m128", "sum_m257", "m52_m520")
NELEM = 5
NOISE_FACTORS = (1.0, 0.7, 1.5, 1.0, 2.0)
FIT_FIGURES = S.FIGURES[:6]
CEILING = {"fit": 1e-10, "trace": 1e-9}


def element_terms(name):
    """The five elements' models in the form of sparse_cases.CASES[name]["terms"]."""
    terms = S.CASES[name]["terms"]
    rs = np.random.RandomState(211)
    out = [[tuple(t) for t in terms]]
    for _ in range(1, NELEM):
        el = []
        for t in terms:
            scaled = list(t)
            for at in range(1, len(t), 2):
                scaled[at] = [float(v) for v in np.asarray(t[at], dtype=float) * rs.uniform(0.85, 1.2, size=len(t[at]))]
            el.append(tuple(scaled))
        out.append(el)
    return out


def element_noise():
    return [S.NOISE * f for f in NOISE_FACTORS]


def element_blocks(O, name, terms):
    """The blocks the fit's figures need at one element's parameters (the prediction blocks of sparse_cases.blocks are left empty)."""
    d = S.case_data(name)
    M = S.CASES[name]["M"]
    return dict(Kuu=S.gram(O, terms, d["Z"], d["nZ"], d["Z"], d["nZ"]), Kuf=S.gram(O, terms, d["Z"], d["nZ"], d["X"], d["n"]),
                kd=S.kdiag(O, terms, d["X"], d["n"]), Kus=np.zeros((M, 1)), Kss=np.zeros((1, 1)))


def host_routes(O, name, method, b):
    """(woodbury, dense) of element b of a case."""
    d = S.case_data(name)
    blocks = element_blocks(O, name, element_terms(name)[b])
    s = element_noise()[b] ** 2.0 + d["err_y"] ** 2.0
    return S.woodbury(blocks, d["y"], s, method), S.dense(blocks, d["y"], s, method)


def fit_figures(got, ref):
    """ll and the five sums of ``got`` against ``ref``, each relative to its own size (sparse_cases.figures without the predictions)."""
    out = {"ll": abs(got["ll"] - ref["ll"]) / abs(ref["ll"])}
    for i, k in enumerate(FIT_FIGURES[1:]):
        out[k] = abs(got["parts"][i] - ref["parts"][i]) / abs(ref["parts"][i]) if ref["parts"][i] != 0.0 else abs(got["parts"][i])
    return out


def group_of(figure):
    return "trace" if figure == "trace" else "fit"


def host_err(name, figure):
    group = [f for f in FIT_FIGURES if group_of(f) == group_of(figure)]
    return max(HOST_ERR_BATCH[(name, m, b)][f] for m in S.CASES[name]["methods"] for b in range(NELEM) for f in group)


def bound(name, figure, N):
    """What a device figure of any element of the case may differ from the host's by."""
    return max(10.0 * host_err(name, figure), S.floor(N))


#: Woodbury - dense per case, method and element, measured on the CPU by tests/test_sparse_batch_host.py (which prints these lines)
HOST_ERR_BATCH = {
    ("se1_64", "fitc", 0): {"ll": 1.42e-15, "sum_log_lambda": 2.1e-15, "sum_log_diag_LB": 2.7e-15, "r_lambda_r": 1.25e-14, "c_c": 1.48e-14, "trace": 0},   # cond(K_uu + jitter I) = 1.0e+00
    ("se1_64", "fitc", 1): {"ll": 5.44e-16, "sum_log_lambda": 1.55e-15, "sum_log_diag_LB": 1.04e-15, "r_lambda_r": 3.1e-15, "c_c": 2.84e-15, "trace": 0},   # cond(K_uu + jitter I) = 1.0e+00
    ("se1_64", "fitc", 2): {"ll": 3.47e-16, "sum_log_lambda": 3.54e-15, "sum_log_diag_LB": 3.03e-15, "r_lambda_r": 4.46e-15, "c_c": 5.47e-15, "trace": 0},   # cond(K_uu + jitter I) = 1.0e+00
    ("se1_64", "fitc", 3): {"ll": 2.44e-16, "sum_log_lambda": 1.18e-15, "sum_log_diag_LB": 8.73e-15, "r_lambda_r": 5.24e-15, "c_c": 6.03e-15, "trace": 0},   # cond(K_uu + jitter I) = 1.0e+00
    ("se1_64", "fitc", 4): {"ll": 1.24e-16, "sum_log_lambda": 2.9e-16, "sum_log_diag_LB": 1.54e-16, "r_lambda_r": 3.35e-16, "c_c": 2.05e-16, "trace": 0},   # cond(K_uu + jitter I) = 1.0e+00
    ("se_300", "fitc", 0): {"ll": 4.86e-13, "sum_log_lambda": 7.22e-14, "sum_log_diag_LB": 1.56e-13, "r_lambda_r": 2.01e-13, "c_c": 5.28e-14, "trace": 0},   # cond(K_uu + jitter I) = 2.8e+07
    ("se_300", "fitc", 1): {"ll": 5.29e-13, "sum_log_lambda": 5.75e-14, "sum_log_diag_LB": 2.68e-13, "r_lambda_r": 5.58e-13, "c_c": 5.98e-13, "trace": 0},   # cond(K_uu + jitter I) = 3.8e+07
    ("se_300", "fitc", 2): {"ll": 4.5e-13, "sum_log_lambda": 5.72e-14, "sum_log_diag_LB": 2.76e-13, "r_lambda_r": 7.39e-14, "c_c": 1.15e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.2e+07
    ("se_300", "fitc", 3): {"ll": 1.46e-12, "sum_log_lambda": 2.44e-13, "sum_log_diag_LB": 1.2e-12, "r_lambda_r": 4.34e-13, "c_c": 1.12e-13, "trace": 0},   # cond(K_uu + jitter I) = 4.3e+07
    ("se_300", "fitc", 4): {"ll": 1.17e-13, "sum_log_lambda": 8.97e-14, "sum_log_diag_LB": 5.01e-13, "r_lambda_r": 3.75e-13, "c_c": 5.35e-13, "trace": 0},   # cond(K_uu + jitter I) = 3.0e+07
    ("se_300", "vfe", 0): {"ll": 9.2e-14, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 4.31e-14, "r_lambda_r": 4.01e-16, "c_c": 9.88e-15, "trace": 1.4e-11},   # cond(K_uu + jitter I) = 2.8e+07
    ("se_300", "vfe", 1): {"ll": 8.6e-13, "sum_log_lambda": 1.45e-16, "sum_log_diag_LB": 4.86e-13, "r_lambda_r": 2.73e-16, "c_c": 5.03e-13, "trace": 1.17e-11},   # cond(K_uu + jitter I) = 3.8e+07
    ("se_300", "vfe", 2): {"ll": 3.63e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 4.79e-14, "r_lambda_r": 0, "c_c": 2.01e-13, "trace": 2.38e-11},   # cond(K_uu + jitter I) = 2.2e+07
    ("se_300", "vfe", 3): {"ll": 6.63e-13, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 2.6e-13, "r_lambda_r": 4.01e-16, "c_c": 4.28e-13, "trace": 4.95e-11},   # cond(K_uu + jitter I) = 4.3e+07
    ("se_300", "vfe", 4): {"ll": 1.64e-14, "sum_log_lambda": 2.36e-16, "sum_log_diag_LB": 1.98e-13, "r_lambda_r": 1.3e-16, "c_c": 3.41e-14, "trace": 3.3e-11},   # cond(K_uu + jitter I) = 3.0e+07
    ("se_300", "dtc", 0): {"ll": 1.88e-14, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 4.31e-14, "r_lambda_r": 4.01e-16, "c_c": 9.88e-15, "trace": 0},   # cond(K_uu + jitter I) = 2.8e+07
    ("se_300", "dtc", 1): {"ll": 8.96e-13, "sum_log_lambda": 1.45e-16, "sum_log_diag_LB": 4.86e-13, "r_lambda_r": 2.73e-16, "c_c": 5.03e-13, "trace": 0},   # cond(K_uu + jitter I) = 3.8e+07
    ("se_300", "dtc", 2): {"ll": 4.12e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 4.79e-14, "r_lambda_r": 0, "c_c": 2.01e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.2e+07
    ("se_300", "dtc", 3): {"ll": 8.16e-13, "sum_log_lambda": 1.66e-16, "sum_log_diag_LB": 2.6e-13, "r_lambda_r": 4.01e-16, "c_c": 4.28e-13, "trace": 0},   # cond(K_uu + jitter I) = 4.3e+07
    ("se_300", "dtc", 4): {"ll": 8.95e-14, "sum_log_lambda": 2.36e-16, "sum_log_diag_LB": 1.98e-13, "r_lambda_r": 1.3e-16, "c_c": 3.41e-14, "trace": 0},   # cond(K_uu + jitter I) = 3.0e+07
    ("rq_257", "vfe", 0): {"ll": 8.58e-15, "sum_log_lambda": 1.94e-16, "sum_log_diag_LB": 1.28e-14, "r_lambda_r": 0, "c_c": 1.47e-15, "trace": 8.13e-11},   # cond(K_uu + jitter I) = 2.4e+07
    ("rq_257", "vfe", 1): {"ll": 2.67e-14, "sum_log_lambda": 0, "sum_log_diag_LB": 4.52e-14, "r_lambda_r": 1.49e-16, "c_c": 1.49e-16, "trace": 7.49e-11},   # cond(K_uu + jitter I) = 3.1e+07
    ("rq_257", "vfe", 2): {"ll": 5.49e-15, "sum_log_lambda": 0, "sum_log_diag_LB": 1.13e-14, "r_lambda_r": 0, "c_c": 1.61e-16, "trace": 1.58e-11},   # cond(K_uu + jitter I) = 1.8e+07
    ("rq_257", "vfe", 3): {"ll": 4.36e-14, "sum_log_lambda": 1.94e-16, "sum_log_diag_LB": 6.06e-14, "r_lambda_r": 0, "c_c": 1.47e-16, "trace": 1.04e-10},   # cond(K_uu + jitter I) = 3.4e+07
    ("rq_257", "vfe", 4): {"ll": 3.54e-14, "sum_log_lambda": 2.76e-16, "sum_log_diag_LB": 5.99e-14, "r_lambda_r": 0, "c_c": 2.85e-16, "trace": 1.49e-10},   # cond(K_uu + jitter I) = 2.5e+07
    ("se_m127", "fitc", 0): {"ll": 6.07e-13, "sum_log_lambda": 2.02e-13, "sum_log_diag_LB": 5.36e-13, "r_lambda_r": 1.02e-13, "c_c": 1.24e-13, "trace": 0},   # cond(K_uu + jitter I) = 4.1e+07
    ("se_m127", "fitc", 1): {"ll": 3.86e-12, "sum_log_lambda": 5.25e-13, "sum_log_diag_LB": 1.36e-12, "r_lambda_r": 1.96e-13, "c_c": 4.61e-14, "trace": 0},   # cond(K_uu + jitter I) = 6.1e+07
    ("se_m127", "fitc", 2): {"ll": 4.67e-14, "sum_log_lambda": 5.1e-14, "sum_log_diag_LB": 5.72e-14, "r_lambda_r": 1.07e-13, "c_c": 1.34e-13, "trace": 0},   # cond(K_uu + jitter I) = 3.3e+07
    ("se_m127", "fitc", 3): {"ll": 1.85e-12, "sum_log_lambda": 4.94e-13, "sum_log_diag_LB": 1.5e-12, "r_lambda_r": 5.72e-13, "c_c": 4.99e-13, "trace": 0},   # cond(K_uu + jitter I) = 6.6e+07
    ("se_m127", "fitc", 4): {"ll": 6.42e-13, "sum_log_lambda": 5.28e-14, "sum_log_diag_LB": 1.38e-13, "r_lambda_r": 3.62e-14, "c_c": 8.3e-14, "trace": 0},   # cond(K_uu + jitter I) = 4.5e+07
    ("se_m127", "vfe", 0): {"ll": 1.58e-11, "sum_log_lambda": 0, "sum_log_diag_LB": 5.81e-15, "r_lambda_r": 1.16e-16, "c_c": 4.76e-14, "trace": 7.29e-11},   # cond(K_uu + jitter I) = 4.1e+07
    ("se_m127", "vfe", 1): {"ll": 1.56e-11, "sum_log_lambda": 1.15e-16, "sum_log_diag_LB": 3.55e-13, "r_lambda_r": 1.32e-16, "c_c": 1.82e-13, "trace": 2.3e-10},   # cond(K_uu + jitter I) = 6.1e+07
    ("se_m127", "vfe", 2): {"ll": 1.13e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 3.62e-14, "r_lambda_r": 0, "c_c": 4.19e-14, "trace": 3.46e-11},   # cond(K_uu + jitter I) = 3.3e+07
    ("se_m127", "vfe", 3): {"ll": 1.36e-11, "sum_log_lambda": 0, "sum_log_diag_LB": 5.29e-13, "r_lambda_r": 1.16e-16, "c_c": 6.54e-14, "trace": 1.74e-10},   # cond(K_uu + jitter I) = 6.6e+07
    ("se_m127", "vfe", 4): {"ll": 1.92e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 8.58e-14, "r_lambda_r": 2.02e-16, "c_c": 3.59e-14, "trace": 2.05e-11},   # cond(K_uu + jitter I) = 4.5e+07
    ("se_m128", "fitc", 0): {"ll": 1.2e-12, "sum_log_lambda": 1.12e-13, "sum_log_diag_LB": 8.85e-14, "r_lambda_r": 2.96e-13, "c_c": 3.58e-13, "trace": 0},   # cond(K_uu + jitter I) = 4.1e+07
    ("se_m128", "fitc", 1): {"ll": 1.15e-12, "sum_log_lambda": 5.38e-13, "sum_log_diag_LB": 1.63e-12, "r_lambda_r": 1.13e-12, "c_c": 1.15e-12, "trace": 0},   # cond(K_uu + jitter I) = 6.1e+07
    ("se_m128", "fitc", 2): {"ll": 6.54e-13, "sum_log_lambda": 2.76e-13, "sum_log_diag_LB": 8.5e-13, "r_lambda_r": 3.14e-13, "c_c": 3.82e-13, "trace": 0},   # cond(K_uu + jitter I) = 3.3e+07
    ("se_m128", "fitc", 3): {"ll": 2.38e-12, "sum_log_lambda": 3.49e-13, "sum_log_diag_LB": 6.65e-13, "r_lambda_r": 2.99e-13, "c_c": 2.08e-13, "trace": 0},   # cond(K_uu + jitter I) = 6.6e+07
    ("se_m128", "fitc", 4): {"ll": 5.44e-13, "sum_log_lambda": 2.94e-13, "sum_log_diag_LB": 7.47e-13, "r_lambda_r": 4.32e-13, "c_c": 4.94e-13, "trace": 0},   # cond(K_uu + jitter I) = 4.6e+07
    ("se_m128", "dtc", 0): {"ll": 2.45e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 1.58e-13, "r_lambda_r": 1.16e-16, "c_c": 9.2e-14, "trace": 0},   # cond(K_uu + jitter I) = 4.1e+07
    ("se_m128", "dtc", 1): {"ll": 5.86e-13, "sum_log_lambda": 1.15e-16, "sum_log_diag_LB": 2.31e-13, "r_lambda_r": 0, "c_c": 4.19e-14, "trace": 0},   # cond(K_uu + jitter I) = 6.1e+07
    ("se_m128", "dtc", 2): {"ll": 1.83e-13, "sum_log_lambda": 1.54e-16, "sum_log_diag_LB": 1.71e-13, "r_lambda_r": 1.18e-16, "c_c": 2.06e-14, "trace": 0},   # cond(K_uu + jitter I) = 3.3e+07
    ("se_m128", "dtc", 3): {"ll": 1.76e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 4.65e-13, "r_lambda_r": 1.16e-16, "c_c": 1.22e-13, "trace": 0},   # cond(K_uu + jitter I) = 6.6e+07
    ("se_m128", "dtc", 4): {"ll": 6.9e-13, "sum_log_lambda": 1.8e-16, "sum_log_diag_LB": 4.55e-14, "r_lambda_r": 2.02e-16, "c_c": 4.82e-14, "trace": 0},   # cond(K_uu + jitter I) = 4.6e+07
    ("sum_m257", "fitc", 0): {"ll": 5.02e-12, "sum_log_lambda": 1.66e-13, "sum_log_diag_LB": 7.34e-13, "r_lambda_r": 6.5e-13, "c_c": 2.99e-13, "trace": 0},   # cond(K_uu + jitter I) = 1.6e+08
    ("sum_m257", "fitc", 1): {"ll": 4.8e-12, "sum_log_lambda": 1.43e-13, "sum_log_diag_LB": 8.65e-13, "r_lambda_r": 1.35e-13, "c_c": 3.86e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.1e+08
    ("sum_m257", "fitc", 2): {"ll": 4.97e-12, "sum_log_lambda": 1.46e-13, "sum_log_diag_LB": 7.09e-13, "r_lambda_r": 7.07e-13, "c_c": 3.05e-13, "trace": 0},   # cond(K_uu + jitter I) = 1.7e+08
    ("sum_m257", "fitc", 3): {"ll": 4.34e-12, "sum_log_lambda": 1.16e-13, "sum_log_diag_LB": 5.1e-13, "r_lambda_r": 4.12e-13, "c_c": 8.64e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.0e+08
    ("sum_m257", "fitc", 4): {"ll": 3.1e-12, "sum_log_lambda": 1.29e-13, "sum_log_diag_LB": 6.73e-13, "r_lambda_r": 4.02e-13, "c_c": 7.97e-13, "trace": 0},   # cond(K_uu + jitter I) = 1.7e+08
    ("sum_m257", "vfe", 0): {"ll": 3.5e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 1.16e-13, "r_lambda_r": 0, "c_c": 5.51e-14, "trace": 8.4e-11},   # cond(K_uu + jitter I) = 1.6e+08
    ("sum_m257", "vfe", 1): {"ll": 2.12e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 6.31e-14, "r_lambda_r": 0, "c_c": 2.61e-13, "trace": 9.87e-11},   # cond(K_uu + jitter I) = 2.1e+08
    ("sum_m257", "vfe", 2): {"ll": 4.24e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 7.41e-14, "r_lambda_r": 0, "c_c": 4.85e-13, "trace": 1.43e-10},   # cond(K_uu + jitter I) = 1.7e+08
    ("sum_m257", "vfe", 3): {"ll": 4.08e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 8.43e-14, "r_lambda_r": 0, "c_c": 3.64e-13, "trace": 5.62e-11},   # cond(K_uu + jitter I) = 2.0e+08
    ("sum_m257", "vfe", 4): {"ll": 3.18e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 1.6e-13, "r_lambda_r": 0, "c_c": 2.99e-13, "trace": 1.65e-10},   # cond(K_uu + jitter I) = 1.7e+08
    ("m52_m520", "fitc", 0): {"ll": 1.06e-12, "sum_log_lambda": 8.1e-15, "sum_log_diag_LB": 1.36e-13, "r_lambda_r": 1.69e-14, "c_c": 5.78e-14, "trace": 0},   # cond(K_uu + jitter I) = 1.9e+08
    ("m52_m520", "fitc", 1): {"ll": 1.35e-12, "sum_log_lambda": 3.17e-14, "sum_log_diag_LB": 9.65e-15, "r_lambda_r": 6.38e-14, "c_c": 1.1e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.5e+08
    ("m52_m520", "fitc", 2): {"ll": 4.98e-12, "sum_log_lambda": 7.12e-14, "sum_log_diag_LB": 7.01e-13, "r_lambda_r": 1.77e-13, "c_c": 3.82e-14, "trace": 0},   # cond(K_uu + jitter I) = 3.1e+08
    ("m52_m520", "fitc", 3): {"ll": 3.27e-12, "sum_log_lambda": 5.8e-14, "sum_log_diag_LB": 5.29e-13, "r_lambda_r": 1.17e-13, "c_c": 2.36e-13, "trace": 0},   # cond(K_uu + jitter I) = 2.4e+08
    ("m52_m520", "fitc", 4): {"ll": 1.1e-12, "sum_log_lambda": 1.24e-14, "sum_log_diag_LB": 1.68e-13, "r_lambda_r": 1.16e-14, "c_c": 1.16e-13, "trace": 0},   # cond(K_uu + jitter I) = 1.8e+08
    ("m52_m520", "vfe", 0): {"ll": 9.01e-13, "sum_log_lambda": 0, "sum_log_diag_LB": 7.32e-14, "r_lambda_r": 0, "c_c": 5.6e-14, "trace": 1.89e-12},   # cond(K_uu + jitter I) = 1.9e+08
    ("m52_m520", "vfe", 1): {"ll": 5.9e-12, "sum_log_lambda": 1.93e-16, "sum_log_diag_LB": 1.37e-13, "r_lambda_r": 1.69e-16, "c_c": 3.12e-13, "trace": 2.63e-13},   # cond(K_uu + jitter I) = 2.5e+08
    ("m52_m520", "vfe", 2): {"ll": 6e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 2.1e-13, "r_lambda_r": 1.83e-16, "c_c": 3.11e-13, "trace": 5.4e-12},   # cond(K_uu + jitter I) = 3.1e+08
    ("m52_m520", "vfe", 3): {"ll": 3.47e-12, "sum_log_lambda": 0, "sum_log_diag_LB": 8.1e-14, "r_lambda_r": 0, "c_c": 1.66e-13, "trace": 5.53e-12},   # cond(K_uu + jitter I) = 2.4e+08
    ("m52_m520", "vfe", 4): {"ll": 8.08e-13, "sum_log_lambda": 3.15e-16, "sum_log_diag_LB": 1.01e-13, "r_lambda_r": 1.61e-16, "c_c": 8.95e-14, "trace": 3.04e-12},   # cond(K_uu + jitter I) = 1.8e+08
}
