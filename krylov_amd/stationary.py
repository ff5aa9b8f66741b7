"""The reference's stationary iterations on the device: ``richardson``,
``jacobi``, ``gauss_seidel``, ``sor`` and ``ssor`` (stationary.py:11-157).

``x += update(r); r = b - A x`` with the reference's control flow on the
host and the arithmetic of a chunk of iterations enqueued on the device
scalar chain (extra.py's ``_Chain``): one host sync per chunk, one iteration
per chunk with a callback. The triangular solves of gauss_seidel / sor / ssor
are ``TriangularOperator`` solves (csrc/tri.hip) on the caller's triangle, so
they and jacobi refuse an operator the device renumbered at upload
(``NotImplementedError``); richardson and chebyshev run on one.
"""
import numpy as np
import scipy.sparse

from ._helpers import Problem
from .device import DeviceVector
from .extra import LC_ADD, LC_AXPY, LC_SUB, _Chain, _Dev, _real, _run_chain, _start
from .sparse import CsrOperator, _next_pow2
from .triangular import MAX_COLS, TriangularOperator, canonical_triangle


def _needs_matrix(A, name):
    if isinstance(A, CsrOperator):
        raise TypeError(
            f"{name} needs the matrix's diagonal / triangle, which a CsrOperator does not keep: pass the scipy.sparse "
            "matrix or dense array itself (its device copy is cached, so this costs no second upload)"
        )
    if not (scipy.sparse.issparse(A) or (isinstance(A, np.ndarray) and A.ndim == 2)):
        raise TypeError(f"{name} needs a scipy.sparse matrix or a dense 2-D array, not {type(A).__name__}")


def _check_columns(b):
    """The chain's column limit, before any device work."""
    b = np.asarray(b)
    kc = int(np.prod(b.shape[1:])) if b.ndim > 1 else 1
    if _next_pow2(kc) > MAX_COLS:
        raise NotImplementedError("at most 64 right-hand-side columns on the stationary solvers and chebyshev")


def _triangle(A, lower, diag):
    """tril(A) / triu(A) with its diagonal replaced by ``diag`` (None: kept),
    checked on the host (LinAlgError on a zero diagonal)."""
    S = scipy.sparse.csr_matrix(A)
    if diag is None:
        T = scipy.sparse.tril(S) if lower else scipy.sparse.triu(S)
    else:
        off = scipy.sparse.tril(S, -1) if lower else scipy.sparse.triu(S, 1)
        T = off + scipy.sparse.diags(np.asarray(diag, dtype=S.dtype), format="csr")
    return canonical_triangle(T.tocsr(), lower)


class _TriUpdate:
    """u = T^-1 r for chain vectors (the caller's numbering)."""

    def __init__(self, D, tris):
        prob = D.prob
        self.ops = [TriangularOperator(T, lower=lo, ctx=prob.ctx, dtype=prob.dtype) for T, lo in tris]
        self.scale = None  # ssor: the n-vector between the two solves

    def __call__(self, C, r, u, st):
        C.trisolve(self.ops[0], r, u, st)
        if len(self.ops) == 2:
            C.rowscale(True, u, u, self.scale, st)
            C.trisolve(self.ops[1], u, u, st)
        return u


def _diag_vector(D, d):
    """An (n,) host vector as a device vector of the solve's dtype."""
    return DeviceVector.from_host(D.ctx, np.asarray(d).reshape(-1, 1), dtype=D.prob.dtype)


def richardson(A, b, *args, omega=1.0, **kwargs):
    """Richardson iteration, x += omega r (stationary.py:11-12)."""
    return _stationary(("scale", omega, None), A, b, *args, **kwargs)


def jacobi(A, b, *args, omega=1.0, **kwargs):
    """Jacobi iteration, x += omega (r / D) (stationary.py:15-23)."""
    _needs_matrix(A, "jacobi")
    return _stationary(("jacobi", omega, A.diagonal()), A, b, *args, **kwargs)


def gauss_seidel(A, b, *args, omega=1.0, lower=True, **kwargs):
    """Gauss-Seidel, x += omega tril(A)^-1 r (triu for lower=False;
    stationary.py:26-40)."""
    _needs_matrix(A, "gauss_seidel")
    _check_columns(b)
    return _stationary(("tri", omega, [(_triangle(A, lower, None), lower)]), A, b, *args, **kwargs)


def sor(A, b, *args, omega=1.0, lower=True, **kwargs):
    """Successive over-relaxation, x += (D / omega + L)^-1 r
    (stationary.py:43-61)."""
    _needs_matrix(A, "sor")
    _check_columns(b)
    d_ = A.diagonal() / omega
    return _stationary(("tri", None, [(_triangle(A, lower, d_), lower)]), A, b, *args, **kwargs)


def ssor(A, b, *args, omega=1.0, **kwargs):
    """Symmetric SOR, x += (2 - omega) / omega (D / omega + U)^-1 D
    (D / omega + L)^-1 r (stationary.py:64-94)."""
    _needs_matrix(A, "ssor")
    _check_columns(b)
    d = A.diagonal()
    tris = [(_triangle(A, True, d / omega), True), (_triangle(A, False, d / omega), False)]
    return _stationary(("ssor", (2 - omega) / omega, (tris, d)), A, b, *args, **kwargs)


def _stationary(update, A, b, x0=None, inner=None, tol=1e-5, atol=1.0e-15, maxiter=None, callback=None):
    """stationary.py:97-157 with ``update`` = (kind, factor, data)."""
    kind, factor, data = update
    _check_columns(b)
    prob = Problem(A, b, x0, inner)
    if kind != "scale" and prob.A.renumbered:
        # the diagonal / triangle is the caller's, the chain's vectors the operator's numbering
        raise NotImplementedError(
            "jacobi / gauss_seidel / sor / ssor on an operator the device renumbered at upload (a scattered matrix "
            "with x over 8 MB) are not supported; KRY_RENUMBER=0 keeps the caller's numbering"
        )
    D = _Dev(prob)
    x, r = _start(D, x0)  # x0.copy() / zeros; r = b - A x / b.copy()
    if callback is not None:
        callback(D.host(x), D.host(r))

    first = D.cols(np.sqrt(_real(D.dot(r, r))))
    C = _Chain(D, ["f", "nr"])
    if factor is not None:
        C.set("f", factor)
    u, ax = D.zeros(), D.zeros()
    tri = dvec = None
    if kind == "jacobi":
        dvec = _diag_vector(D, data)
    elif kind == "tri":
        tri = _TriUpdate(D, data)
    elif kind == "ssor":
        tri = _TriUpdate(D, data[0])
        tri.scale = _diag_vector(D, data[1])

    def step(st, _k):
        if kind == "scale":
            C.lc(LC_AXPY, x, x, st, y=r, a="f")  # x += omega * r
        elif kind == "jacobi":
            C.rowscale(False, u, r, dvec, st)
            C.lc(LC_AXPY, x, x, st, y=u, a="f")  # x += omega * (r / D)
        else:
            tri(C, r, u, st)
            if factor is None:
                C.lc(LC_ADD, x, x, st, y=u)  # sor: x += T^-1 r
            else:
                C.lc(LC_AXPY, x, x, st, y=u, a="f")
        C.spmv(prob.A, x, ax, st)
        C.lc(LC_SUB, r, D.b, st, y=ax)  # r = b - A x
        C.norm(r, None, "nr", st)
        C.check("nr", st)

    # no explicit-residual recheck (stationary.py:138-140)
    return _run_chain(D, C, x, r, first, None, step, tol, atol, maxiter, callback)
