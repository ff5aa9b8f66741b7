"""Factorised preconditioners on the device: ``SsorPreconditioner`` and
``Ilu0Preconditioner``, objects that go where a matrix goes as ``M`` / ``Ml``
/ ``Mr`` of cg, gmres, gmres_restarted, minres, bicgstab, cgs, cgr and
chebyshev (the reference takes any object with ``@`` there, _helpers.py:83-90,
and its users hand it SSOR and incomplete-LU operators built on scipy
``spsolve_triangular``).

Both are a ``kry_precond`` (csrc/precond.hip): a short fixed sequence of
``TriangularOperator`` solves and row scales on the solve's n x k device
vectors, in the caller's numbering.

* SSOR: ``M r = (D/w + U)^-1 [D (2 - w)/w] (D/w + L)^-1 r``: lower solve, row
  scale, upper solve (the factor (2 - w)/w is folded into the scale vector).
* ILU(0): ``M r = U^-1 L^-1 r`` with L, U factorised on the device
  (``kry_ilu0_factor``), bitwise the sequential loop over A's pattern.

A solve with one of them runs in the caller's numbering, so an operator the
device renumbered at upload is refused (``KRY_RENUMBER=0`` keeps the caller's
numbering), as are more than 64 right-hand-side columns and the multi-GPU
drivers.

``ordering="multicolor"`` eliminates colour by colour instead of row by row:
the object is ``M = P^T M_B P`` for ``B = P A P^T`` with P the permutation of
``multicolor_ordering(A)``, so every dependency level of the two solves is a
whole colour (two levels on a 5-point or 15-point stencil instead of hundreds
of thin ones). The vectors stay in the caller's numbering; the apply is bitwise
the natural-order object built on B, applied to the permuted vector. Such an
object also folds the row scale into the following solve and fuses the level
the two solves share into one launch (``KRY_PRECOND_FUSE=0`` turns that off).
"""
import ctypes
import time

import numpy as np
import scipy.sparse

from . import _lib
from ._lib import check, lib
from .device import DeviceVector, get_context
from .sparse import CsrOperator, _next_pow2
from .triangular import MAX_COLS, TriangularOperator


def _canonical(A, name, dtype):
    """A as a canonical square real CSR of the preconditioner's dtype."""
    if isinstance(A, CsrOperator):
        raise TypeError(
            f"{name} needs the matrix's diagonal / triangle, which a CsrOperator does not keep: pass the scipy.sparse "
            "matrix or dense array itself (its device copy is cached, so this costs no second upload)"
        )
    if not (scipy.sparse.issparse(A) or (isinstance(A, np.ndarray) and A.ndim == 2)):
        raise TypeError(f"{name} needs a scipy.sparse matrix or a dense 2-D array, not {type(A).__name__}")
    if np.iscomplexobj(A.data if scipy.sparse.issparse(A) else A):
        raise TypeError("complex matrices are outside the MI355X path (float32/float64 only)")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"{name} needs a square matrix, not {A.shape}")
    dt = np.dtype(A.dtype if dtype is None else dtype)
    if dt not in (np.float32, np.float64):
        if dtype is not None:
            raise TypeError(f"dtype must be float32 or float64, not {dt}")
        dt = np.dtype(np.float64)
    csr = scipy.sparse.csr_matrix(A, dtype=dt, copy=True)
    csr.sum_duplicates()
    csr.sort_indices()
    return csr, dt


def multicolor_ordering(A):
    """``(colors, perm)`` of the greedy first-fit colouring of A's graph (the
    stored pattern of A + A^T without the diagonal, explicit zeros included):
    ``colors[i]`` is the smallest integer >= 0 that no neighbour j < i has, and
    ``perm`` lists the rows by (colour, row), so ``A[perm][:, perm]`` has one
    diagonal block per colour. Host only (``kry_color_plan``); int32 arrays."""
    if isinstance(A, CsrOperator):
        raise TypeError("multicolor_ordering needs the matrix's pattern, which a CsrOperator does not keep: pass the "
                        "scipy.sparse matrix or dense array itself")
    if not (scipy.sparse.issparse(A) or (isinstance(A, np.ndarray) and A.ndim == 2)):
        raise TypeError(f"multicolor_ordering needs a scipy.sparse matrix or a dense 2-D array, not {type(A).__name__}")
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"multicolor_ordering needs a square matrix, not {A.shape}")
    csr = scipy.sparse.csr_matrix(A, copy=True)
    csr.sum_duplicates()
    csr.sort_indices()
    itype = np.int32 if (csr.nnz < 2**31 and csr.shape[0] < 2**31) else np.int64
    plan = _lib.color_plan(np.ascontiguousarray(csr.indptr, dtype=itype), np.ascontiguousarray(csr.indices, dtype=itype))
    return plan["color"], plan["perm"]


def _ordering(csr, ordering):
    """(colors, perm, rank, B) for ordering="multicolor": B = A[perm][:, perm]
    canonical, rank[perm[r]] = r; four times None for "natural"."""
    if ordering == "natural":
        return None, None, None, None
    if ordering != "multicolor":
        raise ValueError(f'ordering must be "natural" or "multicolor", not {ordering!r}')
    colors, perm = multicolor_ordering(csr)
    rank = np.empty(csr.shape[0], dtype=np.int32)
    rank[perm] = np.arange(csr.shape[0], dtype=np.int32)
    B = csr[perm][:, perm].tocsr()
    B.sort_indices()
    return colors, perm, rank, B


def _back(T, rank):
    """A factor in B's numbering as a matrix in the caller's: T[rank][:, rank]."""
    return T[rank][:, rank].tocsr()


def refuse_sharded(**ops):
    """The multi-GPU drivers take matrix preconditioners only."""
    for name, op in ops.items():
        for o in op if isinstance(op, (list, tuple)) else [op]:
            if getattr(o, "factored", False):
                raise NotImplementedError(
                    f"{name}: a factorised preconditioner ({type(o).__name__}) runs on one device; "
                    "krylov_amd.distributed.* and devices=[...] take matrix preconditioners only"
                )


class _Factored:
    """What the drivers use on a preconditioner: shape, dtype, ctx, handle,
    matvec_device / matvec_op, ``@``."""

    factored = True
    renumbered = False

    def _setup(self, n, dt, ctx, stages, ordering="natural", colors=None, perm=None):
        self.ordering = ordering
        self.colors = colors  # per row (None in natural order)
        self.perm = perm  # rows by (colour, row): B = A[perm][:, perm]
        self.shape = (n, n)
        self.n = n
        self.dtype = dt
        self.ctx = ctx
        self._stages = stages  # TriangularOperators and (n,) DeviceVectors, kept alive with the handle
        h = ctypes.c_void_p()
        check(lib.kry_precond_create(ctx.handle, n, _lib.dtype_code(dt), ctypes.byref(h)))
        self.handle = h
        self._fin = _lib.own(self, lib.kry_precond_destroy, h)
        for s in stages:
            if isinstance(s, TriangularOperator):
                check(lib.kry_precond_add_tri(h, s.handle))
            else:
                check(lib.kry_precond_add_scale(h, s.handle))
        if ordering == "multicolor":
            check(lib.kry_precond_fuse(h))  # a no-op under KRY_PRECOND_FUSE=0

    @property
    def device(self):
        return self.ctx.device

    def layout(self):
        """{"stages": one entry per stage, a triangular solve's plan (levels,
        launches, ...; TriangularOperator.layout) or {"scale": n}; "ordering";
        "colors" and "color_sizes" (the number of colours and the rows of each;
        None in natural order); "launches": kernel launches per apply;
        "fused": whether the apply folds the scale into the following solve and
        fuses matching level boundaries (kry_precond_info)}."""
        info = np.zeros(5, dtype=np.int64)
        check(lib.kry_precond_info(self.handle, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        sizes = None if self.colors is None else [int(c) for c in np.bincount(self.colors)]
        return {"stages": [s.layout() if isinstance(s, TriangularOperator) else {"scale": self.n}
                           for s in self._stages],
                "ordering": self.ordering, "colors": None if sizes is None else len(sizes), "color_sizes": sizes,
                "launches": int(info[0]), "fused": bool(info[1])}

    def matvec_device(self, x, y):
        """y = P x for DeviceVectors (n x k, k a power of two <= 64, this
        preconditioner's dtype) in the caller's numbering; y may be x."""
        check(lib.kry_precond_apply(self.ctx.handle, self.handle, x.handle, y.handle))

    matvec_op = matvec_device  # never renumbered

    def solve(self, y):
        """P y for a host array of shape (n,) or (n, k)."""
        y = np.asarray(y)
        if y.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        y2 = np.ascontiguousarray(y.reshape(self.n, -1), dtype=self.dtype)
        k = y2.shape[1]
        kp = _next_pow2(k)
        if kp > MAX_COLS:
            raise NotImplementedError("at most 64 right-hand-side columns on a factorised preconditioner")
        if kp != k:
            y2 = np.concatenate([y2, np.zeros((self.n, kp - k), dtype=self.dtype)], axis=1)
        yv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        yv.upload(y2)
        xv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        self.matvec_device(yv, xv)
        return np.ascontiguousarray(xv.to_host()[:, :k]).reshape(y.shape)

    __matmul__ = solve

    def close(self):
        self._fin()

    def __repr__(self):
        return f"{type(self).__name__}(n={self.n}, dtype={self.dtype}, device={self.device})"


class SsorPreconditioner(_Factored):
    """``M = (2 - omega)/omega (D/omega + U)^-1 D (D/omega + L)^-1`` for
    A = L + D + U (the update of the reference's ssor, stationary.py:64-94, as
    a preconditioner). ``A``: scipy.sparse matrix or dense array; ``dtype``:
    the dtype of the vectors it will precondition (default A's).
    ``ordering="multicolor"``: L and U split the off-diagonal entries by the
    multicolour elimination order instead of by index (the module's notes)."""

    def __init__(self, A, omega=1.0, dtype=None, device=None, ordering="natural"):
        csr, dt = _canonical(A, "SsorPreconditioner", dtype)
        colors, perm, rank, B = _ordering(csr, ordering)
        n = csr.shape[0]
        d = csr.diagonal()
        if n and np.any(d == 0):
            raise np.linalg.LinAlgError(f"A has a zero or missing diagonal entry (row {int(np.argmax(d == 0))})")
        self.omega = float(omega)
        if B is not None:
            csr, d = B, B.diagonal()
        dw = (d / dt.type(omega)).astype(dt)
        diag = scipy.sparse.diags(dw, format="csr", dtype=dt)
        self._lower = (scipy.sparse.tril(csr, -1) + diag).tocsr().astype(dt)
        self._upper = (scipy.sparse.triu(csr, 1) + diag).tocsr().astype(dt)
        self._scale = (d * dt.type((2 - omega) / omega)).astype(dt)
        ctx = get_context(device)
        if B is None:
            lo, up, scale = self._lower, self._upper, self._scale
        else:  # the same factors in the caller's numbering, solved in the order perm lists the rows in
            lo, up, scale = _back(self._lower, rank), _back(self._upper, rank), self._scale[rank]
        sv = DeviceVector.from_host(ctx, scale.reshape(-1, 1), dtype=dt)
        self._setup(n, dt, ctx, [TriangularOperator(lo, lower=True, ctx=ctx, dtype=dt, order=perm), sv,
                                 TriangularOperator(up, lower=False, ctx=ctx, dtype=dt, order=perm)],
                    ordering, colors, perm)

    def factors(self):
        """(D/omega + L, D/omega + U, D (2 - omega)/omega): the two triangles
        as scipy CSR and the scale vector applied between their solves; in the
        numbering of B = A[perm][:, perm] under ordering="multicolor"."""
        return self._lower, self._upper, self._scale


class Ilu0Preconditioner(_Factored):
    """``M = U^-1 L^-1`` with the incomplete factors of A on A's own pattern,
    factorised on the device. Every row of A must store its diagonal entry;
    a pivot that comes out zero or non-finite raises ``LinAlgError`` naming the
    row. ``ordering="multicolor"``: the factors of B = A[perm][:, perm] (the
    module's notes); ``lu`` and ``factors()`` are then in B's numbering, and so
    is the row an error names."""

    def __init__(self, A, dtype=None, device=None, ordering="natural"):
        csr, dt = _canonical(A, "Ilu0Preconditioner", dtype)
        colors, perm, rank, B = _ordering(csr, ordering)
        if B is not None:
            csr = B
        n, nnz = csr.shape[0], int(csr.nnz)
        if nnz >= 2**31 - 1:
            raise NotImplementedError("the ILU(0) factorisation indexes entries in int32")
        ctx = get_context(device)
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        data = np.ascontiguousarray(csr.data, dtype=dt)
        vals = np.zeros(max(nnz, 1), dtype=dt)
        info = np.zeros(4, dtype=np.int64)
        t0 = time.perf_counter()
        check(lib.kry_ilu0_factor(ctx.handle, n, nnz, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                  _lib.dtype_code(dt), _lib.KRY_I32, _lib.ptr(vals),
                                  info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        vals = vals[:nnz]
        # analysis, upload, the factorisation kernels and the values' way back (tools/bench_precond.py)
        self.factor_seconds = time.perf_counter() - t0
        self._plan = {"levels": int(info[0]), "launches": int(info[1]), "max_level": int(info[2])}
        # the factorised values on A's pattern; L = strict lower part + I, U = the rest
        self.lu = scipy.sparse.csr_matrix((vals, indices, indptr), shape=(n, n))
        rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
        low = indices < rows
        eye = np.arange(n, dtype=np.int32)
        self._L = scipy.sparse.coo_matrix(
            (np.concatenate([vals[low], np.ones(n, dtype=dt)]),
             (np.concatenate([rows[low], eye]), np.concatenate([indices[low], eye]))), shape=(n, n)).tocsr()
        self._U = scipy.sparse.coo_matrix((vals[~low], (rows[~low], indices[~low])), shape=(n, n)).tocsr()
        self._L.sort_indices()
        self._U.sort_indices()
        lo, up = (self._L, self._U) if B is None else (_back(self._L, rank), _back(self._U, rank))
        self._setup(n, dt, ctx, [TriangularOperator(lo, lower=True, ctx=ctx, dtype=dt, order=perm),
                                 TriangularOperator(up, lower=False, ctx=ctx, dtype=dt, order=perm)],
                    ordering, colors, perm)

    def factors(self):
        """(L, U) as scipy CSR: L unit lower triangular (its diagonal stored),
        U upper triangular with the pivots; in the numbering of
        B = A[perm][:, perm] under ordering="multicolor"."""
        return self._L, self._U

    def layout(self):
        """The plans of the two solves ("stages") and the factorisation's own
        ("factor": {"levels", "launches", "max_level"})."""
        return {"factor": dict(self._plan), **super().layout()}
