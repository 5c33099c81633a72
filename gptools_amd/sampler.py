"""Affine-invariant ensemble sampler (Goodman & Weare 2010, the stretch move) over a BATCHED log-probability.

``EnsembleSampler`` has the attributes the reference and ``GaussianProcess._mcmc_trace`` read from an emcee 2.x sampler
(``chain``, ``lnprobability``, ``flatchain``, ``acceptance_fraction``, ``run_mcmc``, ``reset`` ...; ref:
gptools/gaussian_process.py:1694-1838 drives ``emcee.EnsembleSampler``).  emcee evaluates one walker per call; here the
log-probability takes all the proposals of half an ensemble at once -- ``GaussianProcess.ll_batch`` evaluates them in one launch
sequence on the GPU.

One step handles the two halves in order, (first, second) then (second, first).  For the half S (h walkers) against the
complementary half C (hc walkers) the variates come from ``random_state`` in exactly this order::

    z = ((a - 1) * rand(h) + 1) ** 2 / a;    j = randint(hc, size=h);    [evaluation]    u = rand(h)

with the proposal ``q = C[j] - z[:, None] * (C[j] - S)``, accepted where ``(dim - 1) * log(z) + lnp(q) - lnp(S) > log(u)``.
:func:`draw_variates` draws the variates of N steps beforehand in that order, and the loop uses those arrays: a stepper that is not
this Python loop (``gpt_ensemble_run``, the same loop inside the HIP library; csrc/ensemble.hpp) gets the same variates and
gives the same chain bit for bit.  For that the logarithms are the C library's (``math.log``), not numpy's vectorised ones.
"""
import math

import numpy as np

__all__ = ["EnsembleSampler", "draw_variates", "host_steps"]


def draw_variates(random_state, nwalkers, nsteps):
    """The variates of ``nsteps`` steps of an ensemble of ``nwalkers``, drawn from ``random_state`` in the order the steps use
    them: ``(u_stretch, partner, u_accept)``, each ``(nsteps, nwalkers)`` and indexed by the walker they move -- the uniform
    variate behind its stretch ``z``, the index of its partner INTO the complementary half (int32), the uniform variate of
    its accept test."""
    h = nwalkers // 2
    halves = ((slice(0, h), nwalkers - h), (slice(h, nwalkers), h))
    u_stretch, u_accept = np.empty((nsteps, nwalkers)), np.empty((nsteps, nwalkers))
    partner = np.empty((nsteps, nwalkers), dtype=np.int32)
    for s in range(nsteps):
        for S, hc in halves:
            n = S.stop - S.start
            u_stretch[s, S] = random_state.rand(n)
            partner[s, S] = random_state.randint(hc, size=n)
            u_accept[s, S] = random_state.rand(n)
    return u_stretch, partner, u_accept


def _clog(v):
    """Element-wise ``math.log`` (the C library's, as csrc/ensemble.hpp calls it); ``log(0) = -inf``."""
    return np.array([math.log(x) if x > 0.0 else -np.inf for x in v])


def _no_nan(lnp):
    lnp = np.array(lnp, dtype=float).reshape(-1)
    lnp[np.isnan(lnp)] = -np.inf
    return lnp


def host_steps(lnprob_batch, pos, lnp, a, u_stretch, partner, u_accept):
    """The Python loop: ``u_stretch.shape[0]`` steps from ``pos`` (nwalkers, dim) / ``lnp`` (nwalkers,).  Returns ``(chain (nsteps,
    nwalkers, dim), lnp_chain (nsteps, nwalkers), naccept (nwalkers,))``."""
    pos, lnp = np.array(pos, dtype=float), np.array(lnp, dtype=float)
    nsteps, K = u_stretch.shape
    dim, h = pos.shape[1], K // 2
    chain, lnp_chain = np.empty((nsteps, K, dim)), np.empty((nsteps, K))
    naccept = np.zeros(K, dtype=np.int32)
    for s in range(nsteps):
        for S, C in ((slice(0, h), slice(h, K)), (slice(h, K), slice(0, h))):
            t = (a - 1.0) * u_stretch[s, S] + 1.0
            z = t * t / a
            Cj = pos[C][partner[s, S]]
            q = Cj - z[:, None] * (Cj - pos[S])
            new = _no_nan(lnprob_batch(q))
            with np.errstate(invalid="ignore"):              # (-inf against -inf: NaN, no acceptance)
                accept = (dim - 1) * _clog(z) + new - lnp[S] > _clog(u_accept[s, S])
            idx = np.arange(S.start, S.stop)[accept]
            pos[idx] = q[accept]
            lnp[idx] = new[accept]
            naccept[idx] += 1
        chain[s], lnp_chain[s] = pos, lnp
    return chain, lnp_chain, naccept


class EnsembleSampler(object):
    """``EnsembleSampler(nwalkers, dim, lnprob_batch, a=2.0, random_state=None)``: ``lnprob_batch`` maps a ``(K, dim)`` array to
    ``(K,)`` log-probabilities (called with ``K = nwalkers / 2``, and with ``K = nwalkers`` once at the start of a run that is
    given no ``lnprob0``); a NaN it returns counts as ``-inf``.  ``random_state``: a ``numpy.random.RandomState`` or a seed.

    ``chain`` (nwalkers, steps, dim), ``lnprobability`` (nwalkers, steps), ``flatchain``, ``flatlnprobability``,
    ``acceptance_fraction`` (nwalkers,), ``a``, ``dim``, ``k`` (= nwalkers), ``random_state``; ``route`` names the stepping of
    the last run: ``"host"`` (this module's loop) or what a ``stepper`` called itself (``"library"``)."""

    def __init__(self, nwalkers, dim, lnprob_batch, a=2.0, random_state=None):
        nwalkers, dim = int(nwalkers), int(dim)
        if nwalkers % 2 != 0:
            raise ValueError("The number of walkers must be even.")
        if nwalkers < 2 * dim:
            raise ValueError("The number of walkers needs to be at least twice the dimension of the parameter space.")
        self.k, self.dim, self.a = nwalkers, dim, a
        self.lnprob_batch = lnprob_batch
        self.random_state = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        #: ``stepper(pos, lnp, a, u_stretch, partner, u_accept) -> (chain, lnp_chain, naccept)`` in place of :func:`host_steps`,
        #: with an attribute ``route``; None: the Python loop
        self.stepper = None
        self.route = None
        self.reset()

    def reset(self):
        """Forget the chain (the random state goes on)."""
        self._chain = np.empty((self.k, 0, self.dim))
        self._lnprob = np.empty((self.k, 0))
        self.naccepted = np.zeros(self.k)
        self._last_lnprob = None

    @property
    def chain(self):
        return self._chain

    @property
    def lnprobability(self):
        return self._lnprob

    @property
    def flatchain(self):
        return self._chain.reshape((-1, self.dim))

    @property
    def flatlnprobability(self):
        return self._lnprob.reshape(-1)

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(1, self._chain.shape[1])

    def run_mcmc(self, pos0, N, lnprob0=None):
        """``N`` more steps from ``pos0`` (nwalkers, dim); ``lnprob0``: the log-probabilities there, where known.  Appends to the
        chain and returns ``(pos, lnprob)``, the walkers' last state."""
        pos = np.array(pos0, dtype=float)
        if pos.shape != (self.k, self.dim):
            raise ValueError("pos0 must have shape (nwalkers, dim) = (%d, %d)" % (self.k, self.dim))
        lnp = np.array(self.lnprob_batch(pos) if lnprob0 is None else lnprob0, dtype=float).reshape(-1)
        if lnp.shape != (self.k,):
            raise ValueError("one log-probability per walker expected")
        if np.isnan(lnp).any():
            raise ValueError("The initial lnprob was NaN.")
        N = int(N)
        if N > 0:
            variates = draw_variates(self.random_state, self.k, N)
            if self.stepper is None:
                chain, lnp_chain, naccept = host_steps(self.lnprob_batch, pos, lnp, self.a, *variates)
                self.route = "host"
            else:
                chain, lnp_chain, naccept = self.stepper(pos, lnp, self.a, *variates)
                self.route = self.stepper.route
            self._chain = np.concatenate((self._chain, np.transpose(chain, (1, 0, 2))), axis=1)
            self._lnprob = np.concatenate((self._lnprob, lnp_chain.T), axis=1)
            self.naccepted = self.naccepted + naccept
            pos, lnp = np.array(chain[-1]), np.array(lnp_chain[-1])
        self._last_lnprob = np.array(lnp)
        return pos, lnp
