"""The reference's outer loop, once, for every driver (cg.py:150-234,
gmres.py:179-234, minres.py:160-236, bicgstab.py:100-141, stationary.py:136-
155, ...): the stop rule over all columns, the explicit-residual recheck, the
``maxiter`` bound, and the history assembled from chunks of device steps.
Pure NumPy, no device calls: the drivers pass in what runs a chunk.
"""
import numpy as np


def stop_rule_loop(first, criterion, maxiter, run, *, chunk, entry, recheck=None, on_step=None, on_chunk=None):
    """Iterate until ``np.all(resnorms[-1] <= criterion)`` or ``maxiter`` steps.

    ``first``: history entry 0; ``criterion``: ``max(tol * first, atol)``;
    ``maxiter``: an int, or None for no bound.
    ``run(k, steps)`` runs up to ``steps`` (``chunk``, clipped to ``maxiter -
    k``) steps after step k and returns ``(rows, mid)``: one device row per
    step it ran (it stops itself after the first step that meets the rule)
    and a mid-step row or None. ``entry(row)`` makes a row a history entry.
    ``recheck()``: the explicit residual's entry, which replaces the last one
    when the rule is met and decides (cg.py:156-164); None: the rule alone
    decides (stationary.py:138-140).
    ``on_step(k, entry)`` runs after every appended entry (k counts the steps
    before it), ``on_chunk(k, entry)`` after a chunk (k steps done so far).
    A mid-step row replaces the last entry and ends the solve with success
    (bicgstab.py:124-127). A chunk with no row and no mid-step row raises
    ``RuntimeError`` instead of being run again for ever.
    Returns ``(success, k, resnorms)``."""
    resnorms = [first]
    k = 0
    while True:
        if np.all(resnorms[-1] <= criterion):
            if recheck is not None:
                resnorms[-1] = recheck()
            if recheck is None or np.all(resnorms[-1] <= criterion):
                return True, k, resnorms
        if k == maxiter:
            return False, k, resnorms
        rows, mid = run(k, chunk if maxiter is None else min(chunk, maxiter - k))
        if len(rows) == 0 and mid is None:
            raise RuntimeError("a chunk made no progress")
        for row in rows:
            resnorms.append(entry(row))
            if on_step is not None:
                on_step(k, resnorms[-1])
            k += 1
        if mid is not None:
            resnorms[-1] = entry(mid)
            return True, k, resnorms
        if on_chunk is not None:
            on_chunk(k, resnorms[-1])
