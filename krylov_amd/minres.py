"""Preconditioned MINRES driver (reference ``minres.py:28-253``) over the
device loop: Lanczos (arnoldi.py:203-281), the two-rotation QR update, the
three-term direction recurrence and the x update run on the GPU
(``kry_minres_*``), in chunks with one host sync per chunk.
"""
import numpy as np

from . import _helpers
from ._helpers import Info, Problem
from ._loop import stop_rule_loop
from ._state import CoreState
from .device import HostOut


class _MinresState(CoreState):
    PREFIX, PRECOND = "kry_minres", ("M", "Ml", "Mr")

    def update_path(self):
        """(one_launch_tail, fallbacks) of the last run chunk
        (kry_minres_update_path)."""
        one_launch, fallbacks = self._pair("update_path")
        return bool(one_launch), fallbacks


def _num_operations(k):
    return {
        "A": 1 + k,
        "M": 2 + k,
        "Ml": 2 + k,
        "Mr": 1 + k,
        "inner": 2 + 2 * k,
        "axpy": 4 + 8 * k,
    }


def lanczos(A, v, maxiter, M=None, inner=None):
    """The device Lanczos process of ``minres`` on its own (``ArnoldiLanczos``,
    ``arnoldi.py:203-281``): up to ``maxiter`` steps from ``v``, stopping at an
    invariant subspace. Returns ``(V, H, P, is_invariant)`` with the bases as
    lists of vectors and the (steps + 1) x steps tridiagonal H (steps x steps
    after an invariant step), as tests/test_arnoldi.py assembles them."""
    v = np.asarray(v)
    if v.ndim != 1:
        raise ValueError("lanczos takes one start vector")
    prob = Problem(A, v, None, inner, M=M)
    st = _MinresState(prob)
    st.start()
    st.set_criterion(prob.pad_cols(np.full(prob.kc, -1.0), np.inf))  # never "converged"

    def vec(which):
        return st.get(which)[:, 0].copy()

    V, P, cols = [vec(2)], [vec(1)], []
    prev_h2 = 0.0
    invariant = False
    for _ in range(maxiter):
        hist, invariant = st.run(1)
        if len(hist) == 0:
            break
        h = st.get(3, out=np.empty((3, prob.kpad)))
        cols.append(np.array([prev_h2, h[1, 0], h[2, 0]]))
        prev_h2 = h[2, 0]
        if invariant:
            break
        V.append(vec(2))
        P.append(vec(1))
    k = len(cols)
    H = np.zeros((k + 1, k))
    for i, hv in enumerate(cols):
        if i == 0:
            H[:2, 0] = hv[1:]
        else:
            H[i - 1:i + 2, i] = hv
    if invariant:
        H = H[:k]
    return V, H.astype(prob.dtype), P, invariant


def minres(A, b, M=None, Ml=None, Mr=None, inner=None, x0=None, tol=1e-5, atol=1.0e-15, maxiter=None,
           callback=None, *, devices=None):
    """Preconditioned MINRES, reference signature (``minres.py:28-40``).
    ``devices=[...]``: the columns of a block ``b`` over several GPUs of this
    process (``krylov_amd.multi``)."""
    if devices is not None:
        from .multi import solve

        return solve("minres", A, b, devices, x0=x0, inner=inner, tol=tol, atol=atol, maxiter=maxiter,
                     callback=callback, M=M, Ml=Ml, Mr=Mr)
    prob = Problem(A, b, x0, inner, M=M, Ml=Ml, Mr=Mr)
    maxiter = prob.A.shape[0] if maxiter is None else maxiter

    st = _MinresState(prob)
    host_out = HostOut((prob.n, prob.kpad), prob.dtype)  # pages faulted in while the device iterates
    first = prob.colvals(st.start())
    if callback is not None:
        callback(prob.x0_or_zeros(), np.array(first))
    criterion = np.maximum(tol * first, atol)
    st.set_criterion(prob.pad_cols(criterion, np.inf))
    # a step's entry is |y[0]| of the QR recurrence, which the reference keeps
    # in float64 whatever the vectors' dtype (minres.py:195,219); only the
    # first entry and the explicit residual are norms in the vectors' dtype
    success, k, resnorms = stop_rule_loop(
        first, criterion, maxiter, lambda _k, steps: (st.run(steps)[0], None),
        entry=lambda row: prob.colvals(row, np.float64),
        chunk=1 if callback is not None else _helpers.CHUNK, recheck=lambda: prob.colnorms(st.residual_norm2()),
        on_chunk=None if callback is None else lambda _k, rn: callback(st.xk(), np.array(rn)))
    xk = st.xk(out=host_out.take())
    return xk if success else None, Info(success, xk, k, resnorms, num_operations=_num_operations(k),
                                         renumbered=prob.A.renumbered)
