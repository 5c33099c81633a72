"""ctypes binding of ``libgpt_hip.so`` (C ABI declared in ``include/gpt_hip.h``).

This is the only route from the Python host code to the GPU.  There is no CPU fallback: if the
shared library is missing or no HIP device is usable, every entry point raises.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgpt_hip.so")

GPT_OK = 0
GPT_E_ARG, GPT_E_VALUE, GPT_E_NOTIMPL, GPT_E_HIP, GPT_E_NOMEM, GPT_E_STATE = -1, -2, -3, -4, -5, -6
KERNEL_SE, KERNEL_M52, KERNEL_DIAGNOISE, KERNEL_ZERO, KERNEL_RQ, KERNEL_MATERN, KERNEL_PRODUCT = 0, 1, 2, 3, 4, 5, 6
KERNEL_GIBBS_TANH, KERNEL_GIBBS_DTANH, KERNEL_GIBBS_CUBIC, KERNEL_GIBBS_QUINTIC, KERNEL_GIBBS_EXPGAUSS = 7, 8, 9, 10, 11
KERNEL_GIBBS_BSPLINE = 12
GIBBS_MAX_GAUSS = 8      # GPT_GIBBS_MAX_GAUSS: most Gaussians of KERNEL_GIBBS_EXPGAUSS
GIBBS_MAX_KNOTS = 11     # GPT_GIBBS_MAX_KNOTS: most knots of KERNEL_GIBBS_BSPLINE
KERNEL_GIBBS_GP = 13
GIBBS_MAX_GP_POINTS = 12 # GPT_GIBBS_MAX_GP_POINTS: most points of KERNEL_GIBBS_GP
KERNEL_PERIODIC = 14
PERIODIC_MAXORD = 16     # GPT_PERIODIC_MAXORD: largest combined derivative order of a pair in one dimension for KERNEL_PERIODIC
KERNEL_SPECTRAL = 15
SPECTRAL_MAXORD = 16     # GPT_SPECTRAL_MAXORD: likewise for KERNEL_SPECTRAL
GIBBS_ON_DIM_MAX_D = 3   # GPT_GIBBS_ON_DIM_MAX_D: largest num_dim at which a Gibbs kernel id may carry the dimension it acts on
KERNEL_ON_DIM_STRIDE = 256


def kernel_on_dim(kernel_id, d):
    """GPT_KERNEL_ON_DIM(id, d): the 1-D Gibbs kernel ``kernel_id`` on dimension ``d`` of a model with more dimensions (a product
    factor, include/gpt_hip.h)."""
    return int(kernel_id) + KERNEL_ON_DIM_STRIDE * (int(d) + 1)


def kernel_base_id(kernel_id):
    """GPT_KERNEL_BASE_ID: the plain id of a kernel id with or without a dimension."""
    return int(kernel_id) % KERNEL_ON_DIM_STRIDE if int(kernel_id) >= KERNEL_ON_DIM_STRIDE else int(kernel_id)


MAX_DIM = 16
WARP_LINEAR, WARP_BETA, WARP_MAX_LAYERS = 1, 2, 4
SPARSE_METHODS = {"fitc": 0, "vfe": 1, "dtc": 2}      # GPT_SPARSE_FITC / _VFE / _DTC

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/gpt_hip.h one to one
SIGNATURES = {
    "gpt_version": (C.c_int, []),
    "gpt_last_error": (C.c_char_p, []),
    "gpt_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "gpt_ctx_destroy": (C.c_int, [_vp]),
    "gpt_ctx_set_option": (C.c_int, [_vp, C.c_char_p, _i64]),
    "gpt_ctx_synchronize": (C.c_int, [_vp]),
    "gpt_ctx_stream": (_vp, [_vp]),
    "gpt_ctx_edge_count": (C.c_int64, [_vp]),
    "gpt_concurrency_hint": (C.c_int, [C.c_int]),
    "gpt_kpairs": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _ip, _ip, _i64, C.c_int, C.c_int, C.c_int, _ip, _dp]),
    "gpt_kbuild": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _dp, _ip, _i64, _dp, _ip, _i64, C.c_int, C.c_int, _ip, _dp]),
    "gpt_kpairs2": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _ip, _ip, _i64, C.c_int, _dp]),
    "gpt_kbuild2": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _ip, _i64, _dp, _ip, _i64, C.c_int, _dp]),
    "gpt_fit_terms": (C.c_int, [_vp, C.c_int, _ip, _ip, _dp, _ip, _ip, C.c_double, _dp, _dp, C.c_double, _dp, _dp]),
    "gpt_set_data": (C.c_int, [_vp, _dp, _ip, _i64, C.c_int]),
    "gpt_set_T": (C.c_int, [_vp, _dp, _i64]),
    "gpt_set_warp": (C.c_int, [_vp, C.c_int, _ip, _dp]),
    "gpt_set_warp_batch": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp]),
    "gpt_fit": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, C.c_double, _dp, _dp]),
    "gpt_fit_sum": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip, C.c_double, _dp, _dp, C.c_double, _dp, _dp]),
    "gpt_fit_batch": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp, _ip]),
    "gpt_fit_batch_sum": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _dp, C.c_double, _dp, _dp, _ip]),
    "gpt_mem_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "gpt_release_batch_scratch": (C.c_int, [_vp]),
    "gpt_fit_batch_terms": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp, _dp, _dp, C.c_double, _dp, _dp, _ip]),
    "gpt_predict_batch": (C.c_int, [_vp, _dp, _ip, _i64, _ip, _ip, _dp, _dp, _dp, _dp]),
    "gpt_ensemble_run": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip, _ip, _dp, C.c_int, _ip, _dp, _dp, C.c_double, _dp, _dp, C.c_double,
                                   C.c_double, C.c_int, C.c_int, C.c_double, _dp, _ip, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "gpt_fit_matrix": (C.c_int, [_vp, _dp, _i64, _dp, _dp, _dp]),
    "gpt_get_L": (C.c_int, [_vp, _dp]),
    "gpt_get_alpha": (C.c_int, [_vp, _dp]),
    "gpt_ll_grad": (C.c_int, [_vp, C.c_int, _ip, _ip, _dp]),
    "gpt_ll_grad_diff": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, _dp]),
    "gpt_ll_grad_diff_batch": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, _ip, _dp, _dp]),
    "gpt_loo": (C.c_int, [_vp, _dp, _dp, _dp]),
    "gpt_loo_grad_diff": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpt_predict": (C.c_int, [_vp, _dp, _ip, _i64, C.c_int, _dp, _ip, _dp, _dp, _dp]),
    "gpt_host_alloc": (C.c_int, [_i64, C.POINTER(_vp)]),
    "gpt_host_free": (C.c_int, [_vp]),
    "gpt_cov_sample": (C.c_int, [_vp, _i64, C.c_double, _dp, _i64, _dp]),
    "gpt_solve_L": (C.c_int, [_vp, _dp, _i64]),
    "gpt_cho_solve": (C.c_int, [_vp, _dp, _i64]),
    "gpt_last_timings": (C.c_int, [_vp, _dp, C.c_int]),
    "gpt_gemm_profile_read": (C.c_int, [_vp, _dp]),
    "gpt_gemm_profile_read4": (C.c_int, [_vp, _dp]),
    "gpt_plan_unique_id": (C.c_int, [_vp]),
    "gpt_plan_create": (C.c_int, [C.c_int, C.POINTER(_vp), C.POINTER(_i64), _i64, C.c_int, _vp, _vp, C.c_int, _vp, C.POINTER(_vp)]),
    "gpt_plan_set_comm": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "gpt_plan_set_channel": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "gpt_plan_run": (C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_double, C.c_double]),
    "gpt_plan_last_enqueue_ms": (C.c_double, [_vp]),
    "gpt_plan_destroy": (C.c_int, [_vp]),
    "gpt_potrf_host": (C.c_int, [_vp, _dp, _i64]),
    "gpt_gemm_nt_host": (C.c_int, [_vp, _i64, _i64, _i64, C.c_double, _dp, _dp, C.c_double, _dp]),
    "gpt_dev_kbuild": (C.c_int, [_vp, C.c_int, _dp, C.c_int, _vp, _vp, _i64, _vp, _vp, _i64, C.c_int, C.c_int, C.c_int,
                                 _ip, C.c_int, _i64, _i64, _vp, C.c_double, C.c_double, _vp, _i64]),
    "gpt_dev_gemm_nt": (C.c_int, [_vp, _i64, _i64, _i64, C.c_double, _vp, _i64, _vp, _i64, C.c_double, _vp, _i64, C.c_int]),
    "gpt_dev_gemm_nt_stair": (C.c_int, [_vp, _i64, _i64, _i64, _i64, C.c_double, _vp, _i64, _vp, _i64, _i64, _i64, C.c_double, _vp, _i64]),
    "gpt_dev_gemm_nt_gridstair": (C.c_int, [_vp, _i64, _i64, _i64, _i64, C.c_double, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64,
                                           C.c_double, _vp, _i64]),
    "gpt_dev_row_sumsq": (C.c_int, [_vp, _vp, _i64, _vp]),
    "gpt_dev_potrf_panel": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64]),
    "gpt_dev_potrf": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "gpt_dev_trsm_rlt": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64]),
    "gpt_dev_trinv": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64]),
    "gpt_dev_copy2d": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _i64]),
    "gpt_dev_copy2d_on": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64]),
    "gpt_dev_pad_block": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, C.c_double]),
    "gpt_dev_panel_scalars": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "gpt_sparse_set_inducing": (C.c_int, [_vp, _dp, _ip, _i64]),
    "gpt_sparse_fit": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, C.c_double, _dp, _dp, C.c_double, _i64, _dp, _dp]),
    "gpt_sparse_predict": (C.c_int, [_vp, _dp, _ip, _i64, C.c_int, _dp, _ip, _dp, _dp, _dp]),
    "gpt_sparse_get_c": (C.c_int, [_vp, _dp]),
    "gpt_dev_sparse_gram": (C.c_int, [_vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _i64]),
    "gpt_dev_sparse_lambda": (C.c_int, [_vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, C.c_double, _vp, _i64, _ip]),
    "gpt_dev_sparse_rowsum": (C.c_int, [_vp, _vp, _i64, _i64, _vp]),
    "gpt_dev_sparse_var": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "gpt_dev_sparse_assemble_b": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, C.c_double]),
    "gpt_sparse_fit_batch": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _ip, _ip, _dp, _dp, _dp, C.c_double, _i64, _dp, _dp,
                                       _ip, _ip]),
    "gpt_dev_sparse_lambda_batch": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, C.c_int, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64,
                                              _vp]),
    "gpt_dev_sparse_rowsum_batch": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64]),
    "gpt_dev_sparse_gram_batch": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, C.c_int, _vp, _i64, _i64]),
    "gpt_dev_sparse_assemble_b_batch": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _i64, C.c_double]),
    "gpt_sparse_grad_diff": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpt_dev_sparse_grad_rows": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp, _i64,
                                           _vp, _vp, _vp]),
    "gpt_dev_sparse_gram2": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, C.c_int, _vp, _i64]),
    "gpt_dev_sparse_grad_pairs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _vp, _vp, _i64,
                                            _vp, _vp, _i64, _vp, _i64, _vp, _dp]),
    "gpt_sparse_grad_z": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpt_dev_sparse_grad_dz_pairs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _vp, _vp, _i64, _vp, _vp, _i64,
                                               _vp, _i64, C.c_int, _dp]),
    "gpt_sparse_select_inducing": (C.c_int, [_vp, C.c_int, _ip, _ip, _dp, _ip, _ip, _ip, _i64, _i64, C.c_double, _ip, _dp, _dp,
                                             C.POINTER(_i64)]),
    "gpt_dev_greedy_parts": (_i64, [_i64]),
    "gpt_dev_greedy_update": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpt_dev_greedy_pick": (C.c_int, [_vp, _i64, _i64, C.c_double, _vp, _vp, _i64, _vp, _vp, C.c_int, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
}

_lib = None
_lock = threading.Lock()


class GPTBackendError(RuntimeError):
    """The HIP backend is missing or failed; there is deliberately no CPU fallback."""


def build(verbose=False):
    """Compile ``libgpt_hip.so`` for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise GPTBackendError("building libgpt_hip.so failed")
    return LIB_PATH


def load():
    """Load the shared library and declare every prototype; raises if it is absent."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise GPTBackendError(
                    "%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(gptools_amd has no CPU fallback)" % LIB_PATH)
            try:
                # torch wheels bundle their own libamdhip64; it has to be the first HIP runtime in the process,
                # otherwise torch.cuda (streams, RCCL in gptools_amd.dist) stays unavailable afterwards
                import torch  # noqa: F401
            except ImportError:
                pass
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)          # AttributeError if the export is missing
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def last_error():
    return load().gpt_last_error().decode("utf-8", "replace")


def check(rc):
    """Map a C status to the exception the reference would raise at the same place."""
    if rc == GPT_OK:
        return
    msg = last_error()
    if rc > 0:
        raise np.linalg.LinAlgError(msg or "%d-th leading minor of the array is not positive definite" % rc)
    if rc in (GPT_E_ARG, GPT_E_VALUE):
        raise ValueError(msg)
    if rc == GPT_E_NOTIMPL:
        raise NotImplementedError(msg)
    if rc == GPT_E_NOMEM:
        raise MemoryError(msg)
    raise GPTBackendError("libgpt_hip: %s (code %d)" % (msg, rc))


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_ip)


class _PinnedOwner(object):
    """Returns a gpt_host_alloc block to the pool (or frees it) when the numpy array built over it is collected."""

    def __init__(self, lib, ptr, nbytes):
        self._lib, self._ptr, self._nbytes = lib, ptr, nbytes

    def __del__(self):
        try:
            if self._ptr:
                _pinned_release(self._lib, self._ptr, self._nbytes)
                self._ptr = None
        except Exception:
            pass


# Page-locking memory costs about as much as moving it once through the pageable path (~0.1 ms per MB), so blocks are kept
# for the next result of the same size -- the usual pattern is predict after predict at the same number of points -- up
# to PINNED_POOL_BYTES in total.
PINNED_POOL_BYTES = 2 << 30
_pinned_free = {}
_pinned_held = [0]


def _pinned_release(lib, ptr, nbytes):
    with _lock:
        if _pinned_held[0] + nbytes <= PINNED_POOL_BYTES:
            _pinned_free.setdefault(nbytes, []).append(ptr)
            _pinned_held[0] += nbytes
            return
    lib.gpt_host_free(ptr)


def pinned_empty(shape, min_bytes=1 << 20):
    """``numpy.empty(shape)`` of float64 in page-locked host memory (gpt_host_alloc) when it is at least ``min_bytes`` large
    -- the device writes such an array by asynchronous DMA (the (M, M) covariance of predict) -- else a plain array."""
    n = int(np.prod(shape))
    if n * 8 < min_bytes:
        return np.empty(shape, dtype=np.float64)
    lib = load()
    p = None
    with _lock:
        blocks = _pinned_free.get(n * 8)
        if blocks:
            p = blocks.pop()
            _pinned_held[0] -= n * 8
    if p is None:
        p = _vp()
        check(lib.gpt_host_alloc(n * 8, C.byref(p)))
    buf = (C.c_double * n).from_address(p.value)
    buf._owner = _PinnedOwner(lib, p, n * 8)     # lives as long as the array (numpy keeps `buf` as the array's base)
    return np.ctypeslib.as_array(buf).reshape(shape)


class concurrent_evaluations(object):
    """``with concurrent_evaluations():`` brackets a section in which several contexts of this process evaluate at the same
    time (one host thread each): the library then keeps every look-ahead on event edges (gpt_concurrency_hint)."""

    def __enter__(self):
        load().gpt_concurrency_hint(1)
        return self

    def __exit__(self, *exc):
        load().gpt_concurrency_hint(-1)
        return False


class Context(object):
    """One GPU + stream; owns the device-resident X, n, K_tot/L, invd, alpha."""

    def __init__(self, device=0, stream=None):
        lib = load()
        h = _vp()
        check(lib.gpt_ctx_create(int(device), _vp(stream) if stream else None, C.byref(h)))
        self._h = h
        self._lib = lib
        self.device = int(device)
        self._warp_key = None               # the layers the library holds (set_warp); None: no warp
        self._term_nparams = None           # parameter counts of the terms of the last successful fit / fit_sum / fit_terms
        self._batch_shape = None            # (elements, N, parameter counts of the terms) of the last successful fit_batch*

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise GPTBackendError("context already destroyed")
        return self._h

    def set_option(self, key, value):
        check(self._lib.gpt_ctx_set_option(self.handle, key.encode(), int(value)))

    def synchronize(self):
        check(self._lib.gpt_ctx_synchronize(self.handle))

    @property
    def stream(self):
        return self._lib.gpt_ctx_stream(self.handle)

    @property
    def edge_count(self):
        """Flag edges raised so far (does not grow while the look-ahead runs on events: another evaluation in flight in the
        process, a profiler's counter collection, GPT_EDGE_FLAGS=0, n > 12288, after a flag timeout)."""
        return int(self._lib.gpt_ctx_edge_count(self.handle))

    # ---- Kernel.__call__ / compute_Kij -------------------------------------------------------
    @staticmethod
    def _pair_args(Xi, Xj, ni, nj):
        """Points and orders of a pair list -> ``(argument tuple of gpt_kpairs*, D, out, keep)``; ``keep`` holds the contiguous
        copies the pointers point into: the caller keeps it alive across the C call."""
        Xi, Xj, ni, nj = f64(Xi), f64(Xj), i32(ni), i32(nj)
        if Xi.ndim != 2 or Xi.shape != Xj.shape or ni.shape != Xi.shape or nj.shape != Xi.shape:
            raise ValueError("Lengths/widths of Xi, Xj, ni, nj don't match")
        M, D = Xi.shape
        return (dptr(Xi), dptr(Xj), iptr(ni), iptr(nj), M), D, np.empty(M, dtype=np.float64), (Xi, Xj, ni, nj)

    @staticmethod
    def _block_args(Xi, ni, Xj, nj):
        """Points and orders of a Gram block (``Xj`` None: of ``Xi`` with itself) -> ``(argument tuple of gpt_kbuild*, D, out,
        keep)``; ``keep`` as in :meth:`_pair_args`."""
        Xi, ni = f64(Xi), i32(ni)
        M, D = Xi.shape
        if Xj is None:
            Xj_, nj_, P = None, None, M
        else:
            Xj_, nj_ = f64(Xj), i32(nj)
            P = Xj_.shape[0]
        return (dptr(Xi), iptr(ni), M, dptr(Xj_), iptr(nj_), P), D, np.empty((M, P), dtype=np.float64), (Xi, ni, Xj_, nj_)

    def kpairs(self, kernel_id, params, Xi, Xj, ni, nj, hyper_deriv=None, symmetric=False, noise_n=None):
        params = f64(params)
        pts, D, out, keep = self._pair_args(Xi, Xj, ni, nj)
        nn = None if noise_n is None else i32(noise_n)
        check(self._lib.gpt_kpairs(self.handle, kernel_id, dptr(params), len(params), *pts, D,
                                   -1 if hyper_deriv is None else int(hyper_deriv), int(bool(symmetric)), iptr(nn), dptr(out)))
        return out

    def kbuild(self, kernel_id, params, Xi, ni, Xj=None, nj=None, hyper_deriv=None, noise_n=None):
        params = f64(params)
        pts, D, out, keep = self._block_args(Xi, ni, Xj, nj)
        nn = None if noise_n is None else i32(noise_n)
        check(self._lib.gpt_kbuild(self.handle, kernel_id, dptr(params), len(params), *pts, D,
                                   -1 if hyper_deriv is None else int(hyper_deriv), iptr(nn), dptr(out)))
        return out

    def kpairs2(self, kid1, params1, kid2, params2, Xi, Xj, ni, nj):
        """Pair list of the product of two native kernels (gpt_kpairs2)."""
        p1, p2 = f64(params1), f64(params2)
        pts, D, out, keep = self._pair_args(Xi, Xj, ni, nj)
        check(self._lib.gpt_kpairs2(self.handle, kid1, dptr(p1), len(p1), kid2, dptr(p2), len(p2), *pts, D, dptr(out)))
        return out

    def kbuild2(self, kid1, params1, kid2, params2, Xi, ni, Xj=None, nj=None):
        """Covariance matrix of the product of two native kernels (gpt_kbuild2)."""
        p1, p2 = f64(params1), f64(params2)
        pts, D, out, keep = self._block_args(Xi, ni, Xj, nj)
        check(self._lib.gpt_kbuild2(self.handle, kid1, dptr(p1), len(p1), kid2, dptr(p2), len(p2), *pts, D, dptr(out)))
        return out

    @staticmethod
    def _flat_params(terms):
        """The parameters of a model (see :meth:`_pack_terms`) concatenated, both factors of a product term."""
        return np.concatenate([np.asarray(p, dtype=float) for t in terms for p in t[1::2]])

    @staticmethod
    def _pack_terms(terms):
        """A model as a list of ``(kernel_id, params)`` or ``(kernel_id1, params1, kernel_id2, params2)`` (a product term) ->
        ``(ids, ids2, nparams, nparams1, flat parameters)`` as gpt_fit_terms / gpt_fit_batch_terms take them."""
        ids = i32(np.asarray([t[0] for t in terms]))
        ids2 = i32(np.asarray([t[2] if len(t) == 4 else -1 for t in terms]))
        npar1 = i32(np.asarray([len(t[1]) for t in terms]))
        npar = i32(np.asarray([len(t[1]) + (len(t[3]) if len(t) == 4 else 0) for t in terms]))
        return ids, ids2, npar, npar1, f64(Context._flat_params(terms))

    def fit_terms(self, terms, noise_var, y, err_y, diag_add):
        """gpt_fit_terms: ``terms`` is a list of ``(kernel_id, params)`` or ``(kernel_id1, params1, kernel_id2, params2)``
        (a product term)."""
        ids, ids2, npar, npar1, flat = self._pack_terms(terms)
        y, err_y = f64(y), f64(err_y)
        ll = C.c_double()
        ld = C.c_double()
        self._term_nparams = None
        check(self._lib.gpt_fit_terms(self.handle, len(ids), iptr(ids), iptr(ids2), dptr(flat), iptr(npar), iptr(npar1),
                                      float(noise_var), dptr(y), dptr(err_y), float(diag_add), C.byref(ll), C.byref(ld)))
        self._term_nparams = [int(v) for v in npar]
        return ll.value, ld.value

    # ---- fit / state ---------------------------------------------------------------------------
    def set_data(self, X, n):
        X, n = f64(X), i32(n)
        self._warp_key = None               # (gpt_set_data drops the layers)
        self._num_dim = X.shape[1]
        check(self._lib.gpt_set_data(self.handle, dptr(X), iptr(n), X.shape[0], X.shape[1]))

    def set_warp(self, layers):
        """gpt_set_warp: ``layers`` is a list of ``(type, params)`` (``WARP_LINEAR`` / ``WARP_BETA``, 2 D parameters each), the
        first applied first; an empty list (or ``None``) clears the warp.  Every call that changes the layers drops the resident
        factorisation; a call with the layers the library already holds is a no-op, so that reading ``K`` or predicting after a
        fit leaves the factor alone."""
        layers = [(int(t), f64(p).ravel()) for t, p in (layers or [])]
        key = tuple((t, p.tobytes()) for t, p in layers) or None
        if key == self._warp_key:
            return
        self._warp_key = None
        if not layers:
            check(self._lib.gpt_set_warp(self.handle, 0, None, None))
            return
        types = i32(np.asarray([t for t, _ in layers]))
        flat = f64(np.concatenate([p for _, p in layers]))
        if any(p.size != 2 * getattr(self, "_num_dim", -1) for _, p in layers):
            raise ValueError("set_warp needs set_data first, and every layer takes 2 * num_dim parameters")
        check(self._lib.gpt_set_warp(self.handle, len(layers), iptr(types), dptr(flat)))
        self._warp_key = key

    def set_warp_batch(self, layers_list):
        """gpt_set_warp_batch: element b's layers ``layers_list[b]`` (as :meth:`set_warp` takes them; the same types in every
        element) for the next ``fit_batch*`` of ``len(layers_list)`` elements, which consumes them."""
        types = [int(t) for t, _ in layers_list[0]]
        D = getattr(self, "_num_dim", -1)
        rows = []
        for layers in layers_list:
            if [int(t) for t, _ in layers] != types:
                raise ValueError("set_warp_batch: every element takes the same layer types")
            ps = [f64(p).ravel() for _, p in layers]
            if any(p.size != 2 * D for p in ps):
                raise ValueError("set_warp_batch needs set_data first, and every layer takes 2 * num_dim parameters")
            rows.append(np.concatenate(ps) if ps else np.zeros(0))
        flat = f64(np.array(rows))
        check(self._lib.gpt_set_warp_batch(self.handle, len(layers_list), len(types), iptr(i32(np.asarray(types))), dptr(flat)))

    def set_T(self, T):
        """Resident linear transform (Ny, N) for the data set given to set_data; ``None`` removes it."""
        if T is None:
            check(self._lib.gpt_set_T(self.handle, None, 0))
            return
        T = f64(T)
        if T.ndim != 2:
            raise ValueError("T must be 2-dimensional")
        check(self._lib.gpt_set_T(self.handle, dptr(T), T.shape[0]))

    def fit(self, kernel_id, params, noise_var, y, err_y, diag_add):
        params, y, err_y = f64(params), f64(y), f64(err_y)
        ll = C.c_double()
        ld = C.c_double()
        self._term_nparams = None
        check(self._lib.gpt_fit(self.handle, kernel_id, dptr(params), len(params), float(noise_var), dptr(y),
                                dptr(err_y), float(diag_add), C.byref(ll), C.byref(ld)))
        self._term_nparams = [len(params)]
        return ll.value, ld.value

    def fit_sum(self, kernel_ids, params_list, noise_var, y, err_y, diag_add):
        """gpt_fit for a sum of native kernels: ``kernel_ids[t]`` with parameters ``params_list[t]``."""
        ids = i32(np.asarray(kernel_ids))
        npar = i32(np.asarray([len(p) for p in params_list]))
        flat = f64(np.concatenate([np.asarray(p, dtype=float) for p in params_list]))
        y, err_y = f64(y), f64(err_y)
        ll = C.c_double()
        ld = C.c_double()
        self._term_nparams = None
        check(self._lib.gpt_fit_sum(self.handle, len(ids), iptr(ids), dptr(flat), iptr(npar), float(noise_var), dptr(y),
                                    dptr(err_y), float(diag_add), C.byref(ll), C.byref(ld)))
        self._term_nparams = [int(v) for v in npar]
        return ll.value, ld.value

    def fit_batch(self, kernel_id, params, noise_var, y, err_y, diag_add):
        """gpt_fit_batch: ``params`` (B, nparams), ``noise_var`` (B,), ``y`` (B, N), shared ``err_y`` (N,) ->
        ``(ll_data (B,), logdet_half (B,), info (B,) int32)``; ``info[b] > 0``: element b is not positive definite."""
        params, noise_var, y, err_y = f64(np.atleast_2d(params)), f64(noise_var), f64(np.atleast_2d(y)), f64(err_y)
        B = params.shape[0]
        if noise_var.shape != (B,) or y.shape[0] != B or y.shape[1] != err_y.shape[0]:
            raise ValueError("fit_batch: params (B, p), noise_var (B,), y (B, N), err_y (N,) expected")
        ll, ld, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
        self._batch_shape = None
        check(self._lib.gpt_fit_batch(self.handle, B, kernel_id, dptr(params), params.shape[1], dptr(noise_var), dptr(y),
                                      dptr(err_y), float(diag_add), dptr(ll), dptr(ld), iptr(info)))
        self._batch_shape = (B, y.shape[1], [params.shape[1]])
        return ll, ld, info

    def fit_batch_sum(self, kernel_ids, params, nparams, noise_var, y, err_y, diag_add):
        """gpt_fit_batch_sum: as :meth:`fit_batch` for a sum of native kernels; ``params`` (B, sum(nparams)) holds each
        element's term parameters concatenated."""
        ids, npar = i32(kernel_ids), i32(nparams)
        params, noise_var, y, err_y = f64(np.atleast_2d(params)), f64(noise_var), f64(np.atleast_2d(y)), f64(err_y)
        B = params.shape[0]
        if (noise_var.shape != (B,) or y.shape[0] != B or y.shape[1] != err_y.shape[0] or len(ids) != len(npar)
                or params.shape[1] != int(npar.sum())):
            raise ValueError("fit_batch_sum: params (B, sum(nparams)), noise_var (B,), y (B, N), err_y (N,) expected")
        ll, ld, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
        self._batch_shape = None
        check(self._lib.gpt_fit_batch_sum(self.handle, B, len(ids), iptr(ids), dptr(params), iptr(npar), dptr(noise_var),
                                          dptr(y), dptr(err_y), float(diag_add), dptr(ll), dptr(ld), iptr(info)))
        self._batch_shape = (B, y.shape[1], [int(v) for v in npar])
        return ll, ld, info

    def fit_batch_terms(self, terms_list, noise_var, y, err_y, diag_add):
        """gpt_fit_batch_terms: ``terms_list[b]`` is element b's model in the form :meth:`fit_terms` takes (the same kernels in
        every element, only the parameters differ); ``y`` (B, Ny); with a transform set (:meth:`set_T`) K_tot is T (K + noise) T^T."""
        ids, ids2, npar, npar1, _ = self._pack_terms(terms_list[0])
        params = f64(np.array([self._flat_params(terms) for terms in terms_list]))
        noise_var, y, err_y = f64(noise_var), f64(np.atleast_2d(y)), f64(err_y)
        B = params.shape[0]
        if noise_var.shape != (B,) or y.shape[0] != B or y.shape[1] != err_y.shape[0] or params.shape[1] != int(npar.sum()):
            raise ValueError("fit_batch_terms: one parameter set per element, noise_var (B,), y (B, N), err_y (N,) expected")
        ll, ld, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int32)
        self._batch_shape = None
        check(self._lib.gpt_fit_batch_terms(self.handle, B, len(ids), iptr(ids), iptr(ids2), dptr(params), iptr(npar), iptr(npar1),
                                            dptr(noise_var), dptr(y), dptr(err_y), float(diag_add), dptr(ll), dptr(ld), iptr(info)))
        self._batch_shape = (B, y.shape[1], [int(v) for v in npar])
        return ll, ld, info

    def ensemble_run(self, terms, free_idx, lo, hi, log_prior, noise_var, y, err_y, diag_add, a, u_stretch, partner, u_accept,
                     pos, lnp, max_chunk):
        """gpt_ensemble_run: ``u_stretch.shape[0]`` steps of the ensemble sampler's loop inside the library.  ``terms``: the model
        as :meth:`fit_terms` takes it, at the values of the parameters that are not free; ``free_idx[f]``: the place of free
        parameter f in the concatenated term parameters, or their count for the noise sigma; ``lo`` / ``hi``: the prior's box,
        ``log_prior`` its constant log-density; the variates ``(nsteps, nwalkers)`` as ``sampler.draw_variates`` gives them;
        ``pos`` (nwalkers, nfree) and ``lnp`` (nwalkers,) the start.  Returns ``(chain (nsteps, nwalkers, nfree), lnp_chain
        (nsteps, nwalkers), naccept (nwalkers,))``; the walkers' last state is the chain's last step."""
        ids, ids2, npar, npar1, base = self._pack_terms(terms)
        free_idx, lo, hi = i32(free_idx), f64(lo), f64(hi)
        u_stretch, partner, u_accept = f64(u_stretch), i32(partner), f64(u_accept)
        pos, lnp, y, err_y = np.array(pos, dtype=np.float64, order="C"), np.array(lnp, dtype=np.float64), f64(y), f64(err_y)
        nsteps, K = u_stretch.shape
        nfree = free_idx.shape[0]
        if (pos.shape != (K, nfree) or lnp.shape != (K,) or partner.shape != (nsteps, K) or u_accept.shape != (nsteps, K)
                or lo.shape != (nfree,) or hi.shape != (nfree,) or y.shape != err_y.shape or y.ndim != 1):
            raise ValueError("ensemble_run: variates (nsteps, nwalkers), pos (nwalkers, nfree), lnp (nwalkers,), lo / hi (nfree,), "
                             "y and err_y (N,) expected")
        chain, lnp_chain = np.empty((nsteps, K, nfree)), np.empty((nsteps, K))
        naccept = np.zeros(K, dtype=np.int32)
        self._batch_shape = None            # (the run's last chunk becomes the resident batch: not one ll_grad_diff_batch may size)
        check(self._lib.gpt_ensemble_run(self.handle, len(ids), iptr(ids), iptr(ids2), iptr(npar), iptr(npar1), dptr(base), nfree,
                                         iptr(free_idx), dptr(lo), dptr(hi), float(log_prior), dptr(y), dptr(err_y), float(diag_add),
                                         float(noise_var), K, nsteps, float(a), dptr(u_stretch), iptr(partner), dptr(u_accept),
                                         int(max_chunk), dptr(pos), dptr(lnp), dptr(chain), dptr(lnp_chain), iptr(naccept)))
        return chain, lnp_chain, naccept

    def predict_batch(self, Xstar, nstar, keep, noise_n=None, want_var=True, want_cov=False, want_cov_sum=False):
        """gpt_predict_batch: prediction at ``Xstar`` (M, D) from every element of the resident batch (the last
        :meth:`fit_batch_terms` and its kin); ``keep`` (B,) -- 0 skips an element (its rows stay NaN here).  Returns
        ``(mean (B, M), var (B, M) or None, cov (B, M, M) or None, cov_sum (M, M) or None)``, ``cov_sum`` the sum of the kept
        elements' covariances."""
        Xstar, nstar, keep = f64(Xstar), i32(nstar), i32(np.asarray(keep) != 0)
        B, M = keep.shape[0], Xstar.shape[0]
        mean = np.full((B, M), np.nan)
        var = np.full((B, M), np.nan) if want_var else None
        cov = np.full((B, M, M), np.nan) if want_cov else None
        cov_sum = np.empty((M, M)) if want_cov_sum else None
        nn = None if noise_n is None else i32(np.asarray(noise_n).reshape(-1))
        check(self._lib.gpt_predict_batch(self.handle, dptr(Xstar), iptr(nstar), M, iptr(nn), iptr(keep), dptr(mean), dptr(var),
                                          dptr(cov), dptr(cov_sum)))
        return mean, var, cov, cov_sum

    def mem_info(self):
        """(free, total) bytes of this context's GPU."""
        f, t = _i64(), _i64()
        check(self._lib.gpt_mem_info(self.handle, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def release_batch_scratch(self):
        check(self._lib.gpt_release_batch_scratch(self.handle))

    def ll_grad(self, term_idx, local_idx):
        """Data-term gradient for the listed (term, parameter) pairs plus the noise trace term (last entry)."""
        ti, li = i32(np.asarray(term_idx)), i32(np.asarray(local_idx))
        out = np.empty(len(ti) + 1)
        check(self._lib.gpt_ll_grad(self.handle, len(ti), iptr(ti), iptr(li), dptr(out)))
        return out

    def ll_grad_diff(self, term_idx, params_a, params_b, denom):
        """gpt_ll_grad_diff: the data-term gradient by per-pair central differences.  For every entry h the resident model's
        term ``term_idx[h]`` with its complete parameter vector (both factors of a product) at the two stencil points,
        ``params_a[h]`` and ``params_b[h]``, and ``denom[h]`` = theta_b - theta_a; returns the gradient entries followed by the
        noise trace term, as :meth:`ll_grad`."""
        ti, pa, pb, dn = self._pack_stencil("ll_grad_diff", term_idx, params_a, params_b, denom)
        out = np.empty(len(ti) + 1)
        check(self._lib.gpt_ll_grad_diff(self.handle, len(ti), iptr(ti), dptr(pa), dptr(pb), dptr(dn), dptr(out)))
        return out

    def _pack_stencil(self, who, term_idx, params_a, params_b, denom, counts=None):
        """The stencil arguments of :meth:`ll_grad_diff` / :meth:`loo_grad_diff` checked and flattened: ``(term_idx, params_a,
        params_b, denom)`` as the exports read them."""
        ti, dn = i32(np.asarray(term_idx)), f64(np.asarray(denom, dtype=float))
        if not (len(ti) == len(params_a) == len(params_b) == len(dn)):
            raise ValueError("%s: %d terms, %d / %d stencil points, %d steps"
                             % (who, len(ti), len(params_a), len(params_b), len(dn)))
        # The library reads, per entry, as many doubles as the resident term has parameters (the export carries no lengths): the
        # counts are those of this context's last successful fit, and every vector is checked against them here
        # (``counts``: those of the resident sparse fit, for sparse_grad_diff)
        counts = self._term_nparams if counts is None else counts
        if len(ti) and counts is None:
            raise GPTBackendError("%s needs a factorisation made by fit / fit_sum / fit_terms on this context" % who)
        for h, t in enumerate(ti):
            if not 0 <= t < len(counts):
                raise ValueError("%s: term_idx[%d] = %d, the resident model has %d terms" % (who, h, t, len(counts)))
            for p in (params_a[h], params_b[h]):
                if np.size(p) != counts[t]:
                    raise ValueError("%s: entry %d holds %d parameters, term %d of the resident model has %d"
                                     % (who, h, np.size(p), t, counts[t]))
        pa = f64(np.concatenate([np.asarray(p, dtype=float).ravel() for p in params_a])) if len(ti) else f64(np.zeros(1))
        pb = f64(np.concatenate([np.asarray(p, dtype=float).ravel() for p in params_b])) if len(ti) else f64(np.zeros(1))
        return ti, pa, pb, dn

    def loo(self, N):
        """gpt_loo: leave-one-out cross-validation from the resident factor over its ``N`` observations.  Returns ``(loo_ll, resid,
        var)``: the leave-one-out log predictive probability, ``resid[i] = y_i - m_i`` and ``var[i] = s_i^2``, mean and variance
        of the prediction at point i by the model that has not seen it."""
        ll = C.c_double()
        resid, var = np.empty(int(N)), np.empty(int(N))
        check(self._lib.gpt_loo(self.handle, C.byref(ll), dptr(resid), dptr(var)))
        return ll.value, resid, var

    def loo_grad_diff(self, term_idx, params_a, params_b, denom, N):
        """gpt_loo_grad_diff: the gradient of the leave-one-out log predictive probability by per-pair central differences; the
        stencil arguments are :meth:`ll_grad_diff`'s, ``N`` the number of observations.  Returns ``(out, loo_ll, resid, var, u)``:
        the gradient entries followed by the noise trace term, what :meth:`loo` returns, and ``u = K_tot^-1 resid`` (a mean
        function's parameters take their derivative against it)."""
        ti, pa, pb, dn = self._pack_stencil("loo_grad_diff", term_idx, params_a, params_b, denom)
        out = np.empty(len(ti) + 1)
        ll = C.c_double()
        resid, var, u = np.empty(int(N)), np.empty(int(N)), np.empty(int(N))
        check(self._lib.gpt_loo_grad_diff(self.handle, len(ti), iptr(ti), dptr(pa), dptr(pb), dptr(dn), dptr(out), C.byref(ll),
                                          dptr(resid), dptr(var), dptr(u)))
        return out, ll.value, resid, var, u

    def ll_grad_diff_batch(self, term_idx, params_a, params_b, denom, keep, want_alpha=False):
        """gpt_ll_grad_diff_batch: :meth:`ll_grad_diff` for every element of the resident batch (the last :meth:`fit_batch_terms`
        and its kin) in one launch sequence.  ``term_idx`` (nh,) is shared; ``params_a[b][h]`` / ``params_b[b][h]`` are element
        b's stencil points of entry h (the term's complete parameter vector), ``denom`` (B, nh) its steps; ``keep`` (B,) -- 0
        skips an element, whose rows come back as NaN (pass ``info == 0``).  Returns ``(out (B, nh + 1), alpha (B, N) or None)``,
        row b of ``out`` what :meth:`ll_grad_diff` returns for element b alone."""
        ti, keep = i32(np.asarray(term_idx)).reshape(-1), i32(np.asarray(keep) != 0).reshape(-1)
        nh = len(ti)
        dn = f64(np.asarray(denom, dtype=float)).reshape(-1, nh) if nh else f64(np.zeros((len(keep), 0)))
        # The library reads, per element and entry, as many doubles as the batch's term has parameters (the export carries no
        # lengths): the counts are those of this context's last successful fit_batch*, and every vector is checked against them
        if self._batch_shape is None:
            raise GPTBackendError("ll_grad_diff_batch needs a batch fitted by fit_batch / fit_batch_sum / fit_batch_terms on this context")
        B, N, counts = self._batch_shape
        if not (len(keep) == len(params_a) == len(params_b) == dn.shape[0] == B):
            raise ValueError("ll_grad_diff_batch: the resident batch has %d elements; %d / %d stencil rows, %d rows of steps, %d keep flags"
                             % (B, len(params_a), len(params_b), dn.shape[0], len(keep)))
        for h, t in enumerate(ti):
            if not 0 <= t < len(counts):
                raise ValueError("ll_grad_diff_batch: term_idx[%d] = %d, the resident batch's model has %d terms" % (h, t, len(counts)))
        for b in range(B):
            if not (len(params_a[b]) == len(params_b[b]) == nh):
                raise ValueError("ll_grad_diff_batch: element %d holds %d / %d stencil points for %d entries"
                                 % (b, len(params_a[b]), len(params_b[b]), nh))
            for h, t in enumerate(ti):
                for p in (params_a[b][h], params_b[b][h]):
                    if np.size(p) != counts[t]:
                        raise ValueError("ll_grad_diff_batch: element %d, entry %d holds %d parameters, term %d of the resident batch's "
                                         "model has %d" % (b, h, np.size(p), t, counts[t]))

        def flat(rows):
            if not nh:
                return f64(np.zeros(1))
            return f64(np.concatenate([np.asarray(p, dtype=float).ravel() for row in rows for p in row]))
        pa, pb = flat(params_a), flat(params_b)
        out = np.empty((B, nh + 1))
        alpha = np.empty((B, N)) if want_alpha else None
        if not nh:
            dn = f64(np.zeros(1))
        check(self._lib.gpt_ll_grad_diff_batch(self.handle, nh, iptr(ti), dptr(pa), dptr(pb), dptr(dn), iptr(keep), dptr(out),
                                               dptr(alpha)))
        return out, alpha

    def fit_matrix(self, K_tot, y):
        K_tot, y = f64(K_tot), f64(y)
        ll = C.c_double()
        ld = C.c_double()
        self._term_nparams = None
        check(self._lib.gpt_fit_matrix(self.handle, dptr(K_tot), K_tot.shape[0], dptr(y), C.byref(ll), C.byref(ld)))
        return ll.value, ld.value

    def get_L(self, N):
        L = np.empty((N, N), dtype=np.float64)
        check(self._lib.gpt_get_L(self.handle, dptr(L)))
        return L

    def get_alpha(self, N):
        a = np.empty(N, dtype=np.float64)
        check(self._lib.gpt_get_alpha(self.handle, dptr(a)))
        return a

    def predict(self, Xstar, nstar, want, noise_params=None, noise_n=None, device_cov=False):
        """``device_cov`` (with ``want == 2``): the covariance stays on the device (for :meth:`cov_sample`); ``cov`` is None."""
        Xstar, nstar = f64(Xstar), i32(nstar)
        M = Xstar.shape[0]
        mean = np.empty(M)
        std = np.empty(M) if want >= 1 else None
        cov = pinned_empty((M, M)) if (want == 2 and not device_cov) else None
        npar = None if noise_params is None else f64(noise_params)
        nn = None if noise_n is None else i32(noise_n)
        check(self._lib.gpt_predict(self.handle, dptr(Xstar), iptr(nstar), M, int(want), dptr(npar), iptr(nn),
                                    dptr(mean), dptr(std), dptr(cov)))
        return mean, std, cov

    # ---- inducing-point approximations (gpt_sparse_*) ----------------------------------------------
    def sparse_set_inducing(self, Z, nZ=None):
        Z = f64(Z)
        nZ = None if nZ is None else i32(nZ)
        self._sparse_M = None
        check(self._lib.gpt_sparse_set_inducing(self.handle, dptr(Z), iptr(nZ), Z.shape[0]))
        self._sparse_M, self._sparse_D = Z.shape[0], Z.shape[1]

    def sparse_fit(self, method, terms, noise_var, y, err_y, jitter, chunk_rows=0):
        """gpt_sparse_fit: ``method`` one of ``SPARSE_METHODS``' values, ``terms`` as :meth:`fit_terms` takes them ->
        ``(ll, parts)`` with ``parts`` the five sums of the header."""
        ids, ids2, npar, npar1, flat = self._pack_terms(terms)
        y, err_y = f64(y), f64(err_y)
        ll = C.c_double()
        parts = np.zeros(5)
        self._sparse_nparams = None
        check(self._lib.gpt_sparse_fit(self.handle, int(method), len(ids), iptr(ids), iptr(ids2), dptr(flat), iptr(npar), iptr(npar1),
                                       float(noise_var), dptr(y), dptr(err_y), float(jitter), int(chunk_rows), C.byref(ll),
                                       dptr(parts)))
        self._sparse_nparams = [int(v) for v in npar]
        return ll.value, parts

    def sparse_fit_batch(self, method, terms_list, noise_var, y, err_y, jitter, chunk_rows=0):
        """gpt_sparse_fit_batch: ``terms_list[b]`` is element b's model in the form :meth:`fit_terms` takes (the same kernels in every
        element, only the parameters differ), ``noise_var`` (B,), ``y`` (B, N), shared ``err_y`` (N,) -> ``(ll (B,), parts (B, 5),
        info (B,) int32, which (B,) int32)``.  ``which[b]``: 0 element b is good, 1 ``K_uu + jitter I`` is not positive definite (``info[b]``
        the leading minor), 2 a Lambda_i is not a positive finite number, 3 ``B`` is not positive definite.  An element's ``ll`` and
        ``parts`` are the bits :meth:`sparse_fit` returns for it alone with the same ``chunk_rows``.  The resident single sparse fit
        is not disturbed."""
        ids, ids2, npar, npar1, _ = self._pack_terms(terms_list[0])
        params = f64(np.array([self._flat_params(terms) for terms in terms_list]))
        noise_var, y, err_y = f64(noise_var), f64(np.atleast_2d(y)), f64(err_y)
        B = params.shape[0]
        if (noise_var.shape != (B,) or y.shape[0] != B or err_y.ndim != 1 or y.shape[1] != err_y.shape[0]
                or params.shape[1] != int(npar.sum())):
            raise ValueError("sparse_fit_batch: one parameter set per element, noise_var (B,), y (B, N), err_y (N,) expected")
        ll, parts = np.empty(B), np.zeros((B, 5))
        info, which = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        check(self._lib.gpt_sparse_fit_batch(self.handle, B, int(method), len(ids), iptr(ids), iptr(ids2), dptr(params), iptr(npar),
                                             iptr(npar1), dptr(noise_var), dptr(y), dptr(err_y), float(jitter), int(chunk_rows), dptr(ll),
                                             dptr(parts), iptr(info), iptr(which)))
        return ll, parts, info, which

    def _sparse_grad(self, who, term_idx, params_a, params_b, denom, y, err_y, want_alpha, want_dz):
        """The one body of :meth:`sparse_grad_diff` and :meth:`sparse_grad_z` (``want_dz``): ``(out, alpha, dZ or None)``."""
        counts = getattr(self, "_sparse_nparams", None)
        if counts is None:
            counts = []              # (no sparse fit on this context: the library answers GPT_E_STATE)
        ti, pa, pb, dn = self._pack_stencil(who, term_idx, params_a, params_b, denom, counts=counts)
        y, err_y = f64(y), f64(err_y)
        if y.shape != err_y.shape or y.ndim != 1:
            raise ValueError("%s: y and err_y must be vectors of one length, got %s and %s" % (who, y.shape, err_y.shape))
        out = np.empty(len(ti) + 1)
        alpha = np.empty(len(y)) if want_alpha else None
        args = (self.handle, len(ti), iptr(ti), dptr(pa), dptr(pb), dptr(dn), dptr(y), dptr(err_y), dptr(out), dptr(alpha))
        if not want_dz:
            check(self._lib.gpt_sparse_grad_diff(*args))
            return out, alpha, None
        M = getattr(self, "_sparse_M", None)      # (no inducing inputs on this context: the library answers GPT_E_STATE)
        dz = np.full((int(M), int(self._sparse_D)) if M else (1, 1), np.nan)
        check(self._lib.gpt_sparse_grad_z(*(args + (dptr(dz),))))
        return out, alpha, dz

    def sparse_grad_diff(self, term_idx, params_a, params_b, denom, y, err_y, want_alpha=False):
        """gpt_sparse_grad_diff: the gradient of the resident sparse fit's objective by per-pair central differences.  The stencil
        arguments are :meth:`ll_grad_diff`'s, against the terms of the last :meth:`sparse_fit`; ``y`` and ``err_y`` as that fit took
        them.  Returns ``(out, alpha)``: the entries of the kernel parameters followed by the derivative with respect to the noise
        variance, and ``alpha = (Q_ff + Lambda)^-1 y`` (``None`` unless ``want_alpha``)."""
        return self._sparse_grad("sparse_grad_diff", term_idx, params_a, params_b, denom, y, err_y, want_alpha, False)[:2]

    def sparse_grad_z(self, term_idx, params_a, params_b, denom, y, err_y, want_alpha=False):
        """gpt_sparse_grad_z: :meth:`sparse_grad_diff` and, from the same pass over the data, the gradient of the objective with
        respect to the inducing inputs.  Returns ``(out, alpha, dZ)``: the first two as :meth:`sparse_grad_diff` returns them, bit for
        bit, ``dZ`` an (M, D) array (no entry of the stencil is needed for it: ``term_idx`` may be empty)."""
        return self._sparse_grad("sparse_grad_z", term_idx, params_a, params_b, denom, y, err_y, want_alpha, True)

    def sparse_predict(self, Xstar, nstar, want, noise_params=None, noise_n=None):
        Xstar, nstar = f64(Xstar), i32(nstar)
        M = Xstar.shape[0]
        mean = np.empty(M)
        std = np.empty(M) if want >= 1 else None
        cov = np.empty((M, M)) if want == 2 else None
        npar = None if noise_params is None else f64(noise_params)
        nn = None if noise_n is None else i32(noise_n)
        check(self._lib.gpt_sparse_predict(self.handle, dptr(Xstar), iptr(nstar), M, int(want), dptr(npar), iptr(nn), dptr(mean),
                                           dptr(std), dptr(cov)))
        return mean, std, cov

    def sparse_get_c(self):
        out = np.empty(int(self._sparse_M))
        check(self._lib.gpt_sparse_get_c(self.handle, dptr(out)))
        return out

    def sparse_select_inducing(self, terms, M, candidates=None, tol=0.0):
        """gpt_sparse_select_inducing on the resident data: ``terms`` as :meth:`fit_terms` takes them, ``candidates`` strictly ascending
        row indices (``None``: every row whose derivative orders are all zero) -> ``(indices, dmax, trace)`` cut to the ``count`` pivots
        the stop rule let through: ``count`` row indices, ``count`` values of dmax, ``count + 1`` of the trace."""
        ids, ids2, npar, npar1, flat = self._pack_terms(terms)
        M = int(M)
        cand = None if candidates is None else i32(candidates)
        idx = np.full(max(M, 1), -1, dtype=np.int32)
        dmax, trace = np.full(max(M, 1), np.nan), np.full(max(M, 1) + 1, np.nan)
        count = _i64(0)
        check(self._lib.gpt_sparse_select_inducing(self.handle, len(ids), iptr(ids), iptr(ids2), dptr(flat), iptr(npar), iptr(npar1),
                                                   iptr(cand), 0 if cand is None else len(cand), M, float(tol), iptr(idx), dptr(dmax),
                                                   dptr(trace), C.byref(count)))
        n = int(count.value)
        return idx[:n].astype(np.int64), dmax[:n], trace[:n + 1]

    def dev_greedy_parts(self, rows):
        """gpt_dev_greedy_parts: the partials (workgroups) of ``rows`` candidate rows."""
        return int(self._lib.gpt_dev_greedy_parts(int(rows)))

    def dev_greedy_update(self, dL, ld, rows, j, d_col, d_resid, d_mark, d_prow, d_scal, d_words, d_part, d_pidx):
        """gpt_dev_greedy_update on raw device pointers (integers), on the context's stream; the caller synchronises."""
        check(self._lib.gpt_dev_greedy_update(self.handle, dL, int(ld), int(rows), int(j), d_col, d_resid, d_mark, d_prow, d_scal, d_words,
                                              d_part, d_pidx))

    def dev_greedy_pick(self, j, M, tol, d_part, d_pidx, nparts, d_cand, dX, D, dL, ld, d_mark, d_scal, d_words, d_idx, d_dmax, d_trace,
                        d_xp, d_prow):
        """gpt_dev_greedy_pick on raw device pointers (integers; ``d_cand`` may be ``None``), on the context's stream."""
        check(self._lib.gpt_dev_greedy_pick(self.handle, int(j), int(M), float(tol), d_part, d_pidx, int(nparts), d_cand, dX, int(D), dL,
                                            int(ld), d_mark, d_scal, d_words, d_idx, d_dmax, d_trace, d_xp, d_prow))

    def cov_sample(self, diag_add, rand_vars):
        """``cholesky(cov + diag_add I) @ rand_vars`` for the covariance the last ``predict(..., want=2, device_cov=True)`` left
        on the device; ``rand_vars`` (M, S)."""
        R = f64(np.atleast_2d(rand_vars))
        out = np.empty(R.shape)
        check(self._lib.gpt_cov_sample(self.handle, R.shape[0], float(diag_add), dptr(R), R.shape[1], dptr(out)))
        return out

    def solve_L(self, B):
        B2 = np.array(B, dtype=np.float64, order="C")
        shp = B2.shape
        B2 = np.ascontiguousarray(B2.reshape(shp[0], -1))
        check(self._lib.gpt_solve_L(self.handle, dptr(B2), B2.shape[1]))
        return B2.reshape(shp)

    def cho_solve(self, B):
        B2 = np.array(B, dtype=np.float64, order="C")
        shp = B2.shape
        B2 = np.ascontiguousarray(B2.reshape(shp[0], -1))
        check(self._lib.gpt_cho_solve(self.handle, dptr(B2), B2.shape[1]))
        return B2.reshape(shp)

    def last_timings(self):
        out = np.zeros(5)
        self._lib.gpt_last_timings(self.handle, dptr(out), 5)
        return dict(upload=out[0], kbuild=out[1], potrf=out[2], tail=out[3], total=out[4])

    def gemm_profile_read(self, with_bytes=False):
        """(algorithmic flops, summed launch ms, launches[, algorithmic bytes]) of the profiled GEMM launches since the last read."""
        out = np.zeros(4)
        check(self._lib.gpt_gemm_profile_read4(self.handle, dptr(out)))
        if with_bytes:
            return float(out[0]), float(out[1]), int(out[2]), float(out[3])
        return float(out[0]), float(out[1]), int(out[2])

    def potrf_host(self, A):
        L = np.array(A, dtype=np.float64, order="C")
        check(self._lib.gpt_potrf_host(self.handle, dptr(L), L.shape[0]))
        return L

    def gemm_nt_host(self, alpha, A, B, beta, Cm):
        A, B = f64(A), f64(B)
        Cm = np.array(Cm, dtype=np.float64, order="C")
        check(self._lib.gpt_gemm_nt_host(self.handle, A.shape[0], B.shape[0], A.shape[1], float(alpha), dptr(A),
                                         dptr(B), float(beta), dptr(Cm)))
        return Cm


_default_ctx = {}


def default_context(device=0):
    """Process-wide lazily created context (one per device, re-created after fork)."""
    key = (os.getpid(), int(device))
    ctx = _default_ctx.get(key)
    if ctx is None:
        ctx = Context(device)
        _default_ctx[key] = ctx
    return ctx
