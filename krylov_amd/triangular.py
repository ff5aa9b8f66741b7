"""``TriangularOperator``: a device-resident sparse triangular matrix and
``x = T^-1 y`` on it (``kry_tri``; csrc/tri.hip), the building block of the
reference's gauss_seidel / sor / ssor (scipy ``spsolve_triangular``,
stationary.py:26-94).

The rows are sorted by dependency level on the host once (``_lib.tri_plan``
shows the analysis without a device); a solve is a fixed sequence of launches
ordered by the stream alone, and every row is summed in its stored order, so
the result is bitwise repeatable and independent of the launch plan and of the
number of right-hand sides.
"""
import ctypes

import numpy as np
import scipy.sparse

from . import _lib
from ._lib import check, lib
from .device import DeviceVector, get_context
from .sparse import _next_pow2

MAX_COLS = 64  # the chain's limit (kry_prog)


def canonical_triangle(T, lower=True):
    """T as a canonical CSR (sorted rows, duplicates summed) after the checks
    that need no device: square, real, triangular on the stated side, a full
    non-zero diagonal (``numpy.linalg.LinAlgError`` otherwise, as scipy)."""
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
    values are stored in it; default T's own, float32 or float64)."""

    def __init__(self, T, lower=True, device=None, ctx=None, dtype=None):
        csr = canonical_triangle(T, lower)
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
        check(lib.kry_tri_create(self.ctx.handle, self.n, self.nnz, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                 _lib.dtype_code(dt), _lib.itype_code(itype), 1 if lower else 0, ctypes.byref(h)))
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
