"""``TriangularOperator``: a device-resident sparse triangular matrix and
``x = T^-1 y`` on it (``kry_tri``; csrc/tri.hip), the building block of the
reference's gauss_seidel / sor / ssor (scipy ``spsolve_triangular``,
stationary.py:26-94).

The rows are sorted by dependency level on the host once (``_lib.tri_plan``
shows the analysis without a device); a solve is a fixed sequence of launches
ordered by the stream alone, and every row is summed in its stored order, so
the result is bitwise repeatable and independent of the launch plan and of the
number of right-hand sides.

``order=perm`` solves over an elimination order instead of the row numbers
(``kry_tri_create_ordered``): T is triangular in the order perm lists the rows
in, the levels follow that order, and the solve is bitwise the solve of the
explicitly permuted ``T[perm][:, perm]``, while T and the vectors stay in the
caller's numbering.
"""
import ctypes

import numpy as np
import scipy.sparse

from . import _lib
from ._lib import check, lib
from .device import DeviceVector, get_context
from .sparse import _next_pow2

MAX_COLS = 64  # the chain's limit (kry_prog)


def rank_of(order, n):
    """rank[i] = the position of row i in the elimination order ``order`` (a
    permutation of 0..n-1), int32."""
    perm = np.asarray(order)
    if perm.shape != (n,) or not np.issubdtype(perm.dtype, np.integer):
        raise ValueError(f"order must be a permutation of 0..{n - 1} as an integer array of shape ({n},)")
    if n and not np.array_equal(np.sort(perm), np.arange(n)):
        raise ValueError(f"order must be a permutation of 0..{n - 1}")
    rank = np.empty(n, dtype=np.int32)
    rank[perm] = np.arange(n, dtype=np.int32)
    return rank


def canonical_triangle(T, lower=True, rank=None):
    """T as a canonical CSR (sorted rows, duplicates summed) after the checks
    that need no device: square, real, triangular on the stated side (in the
    elimination order ``rank`` when given), a full non-zero diagonal
    (``numpy.linalg.LinAlgError`` otherwise, as scipy)."""
    if scipy.sparse.issparse(T):
        csr = scipy.sparse.csr_matrix(T, copy=True)
    elif isinstance(T, np.ndarray) and T.ndim == 2:
        csr = scipy.sparse.csr_matrix(T)
    else:
        raise TypeError(f"cannot place {type(T).__name__} on the device: pass a scipy.sparse matrix or a 2-D ndarray")
    if csr.shape[0] != csr.shape[1]:
        raise ValueError("T must be square")
    if np.iscomplexobj(csr.data):
        raise TypeError("complex matrices are outside the MI355X path (float32/float64 only)")
    csr.sum_duplicates()
    csr.sort_indices()
    if rank is not None:
        if rank.shape[0] != csr.shape[0]:
            raise ValueError("order must have one entry per row")
        rows = np.repeat(np.arange(csr.shape[0]), np.diff(csr.indptr))
        wrong = rank[csr.indices] > rank[rows] if lower else rank[csr.indices] < rank[rows]
        if np.any(csr.data[wrong] != 0):
            raise ValueError(f"T is not {'lower' if lower else 'upper'} triangular in the given order")
        if np.any(wrong):  # stored zeros on the other side
            csr = scipy.sparse.csr_matrix((csr.data[~wrong], (rows[~wrong], csr.indices[~wrong])), shape=csr.shape)
            csr.sort_indices()
    else:
        other = scipy.sparse.triu(csr, 1) if lower else scipy.sparse.tril(csr, -1)
        if other.count_nonzero():
            raise ValueError(f"T is not {'lower' if lower else 'upper'} triangular")
        if other.nnz:  # stored zeros on the other side
            csr = (scipy.sparse.tril(csr) if lower else scipy.sparse.triu(csr)).tocsr()
            csr.sort_indices()
    d = csr.diagonal()  # 0 for a stored zero and for a missing entry alike
    if csr.shape[0] and np.any(d == 0):
        raise np.linalg.LinAlgError(f"T is singular: zero entry on diagonal (row {int(np.argmax(d == 0))})")
    return csr


class TriangularOperator:
    """A sparse triangular matrix on the device. ``T``: scipy.sparse matrix
    or dense array, triangular on the side ``lower`` says, in the caller's
    numbering. ``dtype``: the dtype of the vectors it will solve for (its
    values are stored in it; default T's own, float32 or float64). ``order``:
    an elimination order (a permutation listing the rows first to last, e.g.
    ``multicolor_ordering(A)[1]``) in which T is triangular; default the row
    numbers."""

    def __init__(self, T, lower=True, device=None, ctx=None, dtype=None, order=None):
        n = T.shape[0] if hasattr(T, "shape") and len(T.shape) == 2 else 0
        rank = None if order is None else rank_of(order, n)
        self.order = None if order is None else np.array(order, dtype=np.int32)
        csr = canonical_triangle(T, lower, rank)
        dt = np.dtype(csr.dtype if dtype is None else dtype)
        if dt not in (np.float32, np.float64):
            dt = np.dtype(np.float64)
        self.lower = bool(lower)
        self.shape = csr.shape
        self.n = csr.shape[0]
        self.nnz = int(csr.nnz)
        self.dtype = dt
        self.ctx = get_context(device) if ctx is None else ctx
        itype = np.int32 if (self.nnz < 2**31 and self.n < 2**31) else np.int64
        indptr = np.ascontiguousarray(csr.indptr, dtype=itype)
        indices = np.ascontiguousarray(csr.indices, dtype=itype)
        data = np.ascontiguousarray(csr.data, dtype=dt)
        h = ctypes.c_void_p()
        head = (self.ctx.handle, self.n, self.nnz, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                _lib.dtype_code(dt), _lib.itype_code(itype), 1 if lower else 0)
        if rank is None:
            check(lib.kry_tri_create(*head, ctypes.byref(h)))
        else:
            check(lib.kry_tri_create_ordered(*head, _lib.ptr(rank), ctypes.byref(h)))
        self.handle = h
        self._fin = _lib.own(self, lib.kry_tri_destroy, h)

    @property
    def device(self):
        return self.ctx.device

    def layout(self):
        """The plan: {"levels", "launches", "slices", "slots", "max_level",
        "bytes"} (kry_tri_info)."""
        info = np.zeros(6, dtype=np.int64)
        check(lib.kry_tri_info(self.handle, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        keys = ("levels", "launches", "slices", "slots", "max_level", "bytes")
        return {k: int(v) for k, v in zip(keys, info)}

    def solve_device(self, y, x):
        """x = T^-1 y for DeviceVectors (n x k, k a power of two <= 64, this
        operator's dtype) in the caller's numbering; x may be y."""
        check(lib.kry_tri_solve(self.ctx.handle, self.handle, y.handle, x.handle))

    def solve(self, y):
        """T^-1 y for a host array of shape (n,) or (n, k)."""
        y = np.asarray(y)
        if y.shape[0] != self.n:
            raise ValueError("dimension mismatch")
        y2 = np.ascontiguousarray(y.reshape(self.n, -1), dtype=self.dtype)
        k = y2.shape[1]
        kp = _next_pow2(k)
        if kp > MAX_COLS:
            raise NotImplementedError("at most 64 right-hand-side columns on the triangular solve")
        if kp != k:
            y2 = np.concatenate([y2, np.zeros((self.n, kp - k), dtype=self.dtype)], axis=1)
        yv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        yv.upload(y2)
        xv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        self.solve_device(yv, xv)
        return np.ascontiguousarray(xv.to_host()[:, :k]).reshape(y.shape)

    def close(self):
        self._fin()

    def __repr__(self):
        side = "lower" if self.lower else "upper"
        return f"TriangularOperator(n={self.n}, nnz={self.nnz}, {side}, dtype={self.dtype}, device={self.device})"
