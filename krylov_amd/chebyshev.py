"""The reference's Chebyshev iteration on the device (chebyshev.py:12-99).

The recurrence's ``alpha`` and ``beta`` depend only on the eigenvalue
estimates and the step number: the host evaluates the reference's own
expressions (chebyshev.py:78-86) and enqueues them per step; everything else
of a chunk of iterations runs on the device scalar chain (extra.py).
"""
import numpy as np

from ._helpers import Problem
from .extra import LC_AXPY, LC_COPY, SOP_SET, _Chain, _Dev, _real, _run_chain, _start
from .stationary import _check_columns


def chebyshev(A, b, eigenvalue_estimates, M=None, x0=None, inner=None, tol=1e-5, atol=1.0e-15, maxiter=None,
              callback=None):
    """Chebyshev iteration, reference signature and iteration
    (chebyshev.py:12-99)."""
    b = np.asarray(b)
    assert len(eigenvalue_estimates) == 2
    assert eigenvalue_estimates[0] <= eigenvalue_estimates[1]
    lmin, lmax = eigenvalue_estimates
    d = (lmax + lmin) / 2
    c = (lmax - lmin) / 2
    _check_columns(b)
    prob = Problem(A, b, x0, inner, M=M)
    D = _Dev(prob)
    mm = prob.ops["M"] is not None

    def norm(v):  # chebyshev.py:42-46
        return np.sqrt(_real(D.dot(v, D.op("M", v))))

    x, r = _start(D, x0)
    first = D.cols(norm(r))
    if callback is not None:
        callback(D.host(x), D.host(r))
    C = _Chain(D, ["alpha", "beta", "nr"])
    p, ap = D.zeros(), D.zeros()
    zt, t1 = (D.zeros(), D.zeros()) if mm else (None, None)

    coef = []  # (alpha, beta) of step k, chebyshev.py:78-86

    def coefficients(kk):
        while len(coef) <= kk:
            j = len(coef)
            if j == 0:
                coef.append((1.0 / d, None))
                continue
            alpha = coef[-1][0]
            beta = 0.5 * (c * alpha) ** 2
            if j > 1:
                beta *= 0.5
            coef.append((1.0 / (d - beta / alpha), beta))
        return coef[kk]

    def step(st, kk):
        alpha, beta = coefficients(kk)
        z = C.apply("M", r, zt, st)
        C.sc(SOP_SET, "alpha", st, value=alpha)
        if kk == 0:
            C.lc(LC_COPY, p, z, st)
        else:
            C.sc(SOP_SET, "beta", st, value=beta)
            C.lc(LC_AXPY, p, z, st, y=p, a="beta")  # p = z + beta p
        C.lc(LC_AXPY, x, x, st, y=p, a="alpha")  # x += alpha p
        C.spmv(prob.A, p, ap, st)
        C.lc(LC_AXPY, r, r, st, y=ap, a="alpha", sa=-1.0)  # r -= alpha (A p)
        C.norm(r, t1, "nr", st, M="M" if mm else None)
        C.check("nr", st)

    return _run_chain(D, C, x, r, first, norm, step, tol, atol, maxiter, callback)
