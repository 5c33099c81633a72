"""Multi-start optimisation in lockstep: the starts of ``optimize_hyperparameters(random_starts=R)`` ask for their evaluations
together.

The reference runs the random starts in a process pool (ref: gptools/gaussian_process.py:723-735).  A HIP context is not shared
across processes, and one after another every evaluation of every start is a launch sequence of its own.  Here one thread runs per
start, each an ordinary ``scipy.optimize.minimize(fun, x0, jac=True, ...)`` whose ``fun`` hands its point to a dispatcher and
blocks; when every start that is still running waits, the dispatcher evaluates all pending points in ONE call -- on the GPU one
batched fit and one batched gradient (``GaussianProcess.ll_gradient_batch``) -- and releases them.  Every start sees exactly the
values it would see alone, so its iterates, ``x``, ``fun`` and ``nfev`` are those of a sequential run bit for bit (the evaluator's
results must not depend on the batch, which the batched routes promise), and the number of rounds is the LARGEST ``nfev`` of any
start, not the sum.

Host only: this module imports no GPU module.  Only the dispatcher -- the calling thread -- ever calls ``evaluate``, so objects the
evaluator touches (the GP, its kernel and mean function) are never used from two threads.
"""
import threading

import numpy as np
import scipy.optimize


class _Aborted(Exception):
    """Raised inside a start's ``fun`` when the driver gives up (``evaluate`` raised, or the driver itself was interrupted)."""


def lockstep_minimize(starts, evaluate, **minimize_kwargs):
    """Run ``scipy.optimize.minimize(fun, x0, jac=True, **minimize_kwargs)`` from every ``x0`` of ``starts`` with the objective
    evaluations of all starts served together.

    ``evaluate(points) -> (f, g)`` takes the list of pending points (one per start that is still running, in the order of the
    starts) and returns their values ``f`` (len(points)) and gradients ``g`` (len(points), dim).  A value that is not finite is
    passed on to scipy with a zero gradient.  An entry of ``f`` that is an exception instance is raised in that start's ``fun``:
    the start's run ends there and counts as one that raised.

    Returns ``(results, rounds)``: ``results[i]`` is the ``OptimizeResult`` of start i, ``None`` where its run raised;
    ``rounds`` the number of calls of ``evaluate``.  If ``evaluate`` itself raises, every waiting start receives an exception, all
    threads end and the exception leaves this function.  No thread outlives the call, on any path."""
    if "jac" in minimize_kwargs:
        raise ValueError("lockstep_minimize drives minimize with jac=True: the evaluator returns the gradients")
    starts = [np.array(x0, dtype=float) for x0 in starts]
    cond = threading.Condition()
    pending, answers = {}, {}
    state = {"live": len(starts), "aborted": False}
    results = [None] * len(starts)

    def make_fun(i):
        def fun(x):
            with cond:
                if state["aborted"]:
                    raise _Aborted()
                pending[i] = np.array(x, dtype=float)          # (a copy: scipy reuses its array)
                cond.notify_all()
                while i not in answers and not state["aborted"]:
                    cond.wait()
                if i not in answers:
                    raise _Aborted()
                ans = answers.pop(i)
            if isinstance(ans, BaseException):
                raise ans
            f, g = ans
            if not np.isfinite(f):
                return f, np.zeros(len(x))
            return f, g
        return fun

    def work(i):
        try:
            results[i] = scipy.optimize.minimize(make_fun(i), starts[i], jac=True, **minimize_kwargs)
        except BaseException:           # (the start is dropped, as a sequential loop drops a start whose run raised)
            results[i] = None
        finally:
            with cond:
                pending.pop(i, None)
                state["live"] -= 1
                cond.notify_all()

    threads = [threading.Thread(target=work, args=(i,), name="lockstep-start-%d" % i) for i in range(len(starts))]
    rounds = 0
    try:
        for t in threads:
            t.start()
        while True:
            with cond:
                while state["live"] > 0 and len(pending) < state["live"]:
                    cond.wait()
                if state["live"] == 0:
                    break
                batch = sorted(pending.items())
                pending.clear()
            f, g = evaluate([x for _, x in batch])
            rounds += 1
            if len(f) != len(batch) or len(g) != len(batch):
                raise ValueError("lockstep_minimize: evaluate returned %d values and %d gradients for %d points"
                                 % (len(f), len(g), len(batch)))
            with cond:
                for (i, _), fi, gi in zip(batch, f, g):
                    answers[i] = fi if isinstance(fi, BaseException) else (float(fi), np.array(gi, dtype=float))
                cond.notify_all()
    finally:
        # every way out: whoever still waits (evaluate raised, an interrupt) is woken with an exception, and every thread is joined
        with cond:
            state["aborted"] = True
            cond.notify_all()
        for t in threads:
            if t.ident is not None:
                t.join()
    return results, rounds
