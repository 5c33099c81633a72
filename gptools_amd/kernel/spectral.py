r"""Spectral mixture kernel (Wilson & Adams, ICML 2013) with derivative observations, evaluated on the GPU.

The reference has no such kernel.  Its spectral density is a mixture of Gaussians; with enough components it approximates any
stationary kernel, and it extrapolates the patterns it finds.  ONE component, :class:`SpectralKernel`, has the hyperparameters
``[sigma_f, mu_1 .. mu_D, l_1 .. l_D]``:

.. math::  k(x, x') = \sigma_f^2 \exp\left(-\sum_d \frac{\tau_d^2}{2 l_d^2}\right) \cos\left(2 \pi \sum_d \mu_d \tau_d\right),\qquad \tau = x - x'

-- one cosine of the dot product, not a product of cosines.  ``mu = 0`` is the squared exponential; ``l_d = inf`` drops the envelope
in dimension ``d``.  The mixture of ``Q`` components is their sum, :func:`spectral_mixture`: up to 8 components are one device model
(one fused builder pass per term), more take the host sum over per-term device calls, like any longer sum.

A component is a native term and a native product factor (beside SE, Matern52, RationalQuadratic, Matern, Periodic or another
Spectral factor; a product with a Gibbs kernel is combined on the host).  Derivative observations of any order up to a combined
order of 16 per dimension, ``ni[m, d] + nj[m, d] <= 16`` (``ValueError`` beyond, before anything is launched).  Device code:
gptools_amd/csrc/spectral.hpp (the complex two-term recurrence, the phase kept and reduced in cycles) and ``spectral_pair`` in
gptools_amd/csrc/kpair.hpp.  A frequency that is not finite, or a length scale that is NaN or zero, is a ``ValueError``.
Hyperparameter derivatives raise ``NotImplementedError`` like the Periodic kernel: the device gradient of the log-posterior
(``GaussianProcess.ll_gradient``) differences the pair function instead.  The likelihood is multimodal in the frequencies:
``GaussianProcess.optimize_hyperparameters`` with random starts and the ensemble sampler are the tools for it.
"""
import numpy as np

from .core import Kernel
from .. import _lib

__all__ = ["SpectralKernel", "spectral_mixture"]


class SpectralKernel(Kernel):
    _gpt_kernel_id = _lib.KERNEL_SPECTRAL
    _gpt_hyper_deriv = False

    def __init__(self, num_dim=1, **kwargs):
        names = ([r"\sigma_f"] + [r"\mu_{:d}".format(i + 1) for i in range(num_dim)] +
                 ["l_{:d}".format(i + 1) for i in range(num_dim)])
        super(SpectralKernel, self).__init__(num_dim=num_dim, num_params=2 * num_dim + 1, param_names=names, **kwargs)


def spectral_mixture(num_dim=1, num_mixtures=2, initial_params=None, param_bounds=None, fixed_params=None, enforce_bounds=False):
    """The spectral mixture of ``num_mixtures`` components: the left-nested ``SumKernel`` ``((c_1 + c_2) + c_3) + ...`` of
    :class:`SpectralKernel` (a single component for ``num_mixtures = 1``).  Its parameters are component-major,
    ``[sigma_f, mu_1 .. mu_D, l_1 .. l_D]`` of the first component, then of the second, ...

    ``initial_params`` and ``fixed_params``: flat, of length ``Q (2 D + 1)``, or of shape ``(Q, 2 D + 1)``.  ``param_bounds``: one
    list of ``2 D + 1`` ``(lower, upper)`` pairs for every component, or a list of ``Q`` such lists."""
    if isinstance(num_mixtures, bool) or not isinstance(num_mixtures, (int, np.integer)) or num_mixtures < 1:
        raise ValueError("num_mixtures must be an integer > 0!")
    if isinstance(num_dim, bool) or not isinstance(num_dim, (int, np.integer)) or num_dim < 1:
        raise ValueError("num_dim must be an integer > 0!")
    Q, P = int(num_mixtures), 2 * int(num_dim) + 1

    def per_component(v, what, dtype):
        if v is None:
            return [None] * Q
        v = np.asarray(v, dtype=dtype)
        if v.shape not in ((Q * P,), (Q, P)):
            raise ValueError("%s must have %d entries, flat or of shape (%d, %d)!" % (what, Q * P, Q, P))
        return [list(r) for r in v.reshape(Q, P)]
    values, fixed = per_component(initial_params, "initial_params", float), per_component(fixed_params, "fixed_params", bool)
    if param_bounds is None:
        bounds = [None] * Q
    else:
        b = np.asarray(param_bounds, dtype=float)
        if b.shape == (P, 2):
            b = np.tile(b, (Q, 1, 1))
        elif b.shape != (Q, P, 2):
            raise ValueError("param_bounds must be %d (lower, upper) pairs, or %d lists of them!" % (P, Q))
        bounds = [[(float(lo), float(hi)) for lo, hi in comp] for comp in b]
    k = None
    for q in range(Q):
        c = SpectralKernel(num_dim=int(num_dim), initial_params=values[q], param_bounds=bounds[q], fixed_params=fixed[q],
                           enforce_bounds=enforce_bounds)
        k = c if k is None else k + c
    return k
