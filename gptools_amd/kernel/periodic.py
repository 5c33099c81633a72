r"""Periodic (exp-sine-squared) kernel with derivative observations, evaluated on the GPU.

The reference has no such kernel.  Hyperparameters ``[sigma_f, l_1 .. l_D, p_1 .. p_D]``:

.. math::  k(x, x') = \sigma_f^2 \prod_d \exp\left(-\frac{2 \sin^2(\pi \tau_d / p_d)}{l_d^2}\right),\qquad \tau = x - x' .

Alone it describes seasonal or rotational data; ``SquaredExponentialKernel * PeriodicKernel`` is the locally periodic model, a
periodic signal that drifts.  Both run natively (a product: beside SE, Matern52, RationalQuadratic, Matern or another Periodic
factor; a product with a Gibbs kernel is combined on the host).

Derivative observations of any order up to a combined order of 16 per dimension, ``ni[m, d] + nj[m, d] <= 16`` (``ValueError``
beyond, before anything is launched).  Device code: gptools_amd/csrc/periodic.hpp (the per-dimension recurrence, argument
reduction in units of the period) and ``periodic_pair`` in gptools_amd/csrc/kpair.hpp.  A period that is not finite and positive,
or a length scale that is NaN or zero, is a ``ValueError``; ``l_d = inf`` masks dimension ``d`` out.  Hyperparameter derivatives
raise ``NotImplementedError`` like the RationalQuadratic and Matern kernels: the device gradient of the log-posterior
(``GaussianProcess.ll_gradient``) differences the pair function instead.
"""
from .core import Kernel
from .. import _lib

__all__ = ["PeriodicKernel"]


class PeriodicKernel(Kernel):
    _gpt_kernel_id = _lib.KERNEL_PERIODIC
    _gpt_hyper_deriv = False

    def __init__(self, num_dim=1, **kwargs):
        names = ([r"\sigma_f"] + ["l_{:d}".format(i + 1) for i in range(num_dim)] +
                 ["p_{:d}".format(i + 1) for i in range(num_dim)])
        super(PeriodicKernel, self).__init__(num_dim=num_dim, num_params=2 * num_dim + 1, param_names=names, **kwargs)
