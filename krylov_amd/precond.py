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

``solve="isai"`` replaces each triangular solve by a product with the
incomplete sparse approximate inverse of its factor (Anzt, Huckle, Braeckle,
Dongarra): W on the factor T's own pattern with (W T) = I on that pattern
(``isai``, ``kry_isai_lower``), so a solve is one SpMV, and ``sweeps``
relaxation steps ``x = x + W (y - T x)`` win back the exact solve's quality.
The upper factor takes ``W_U = isai(U^T)^T``, the right inverse, so that
``W_U = W_L^T`` bitwise when ``U = L^T`` and an SSOR object of a symmetric A
stays symmetric. An apply is ``2 + 4 sweeps`` SpMV launches (SSOR's row scale
goes into the store of the lower stage's last product) and takes up to 256
columns; W and T are device matrices that are never renumbered.

``BlockJacobiPreconditioner`` is the one object that is a single launch by
construction: ``M = blockdiag(A_11, ..., A_mm)^-1`` over a partition of the
rows into blocks of 1 to 32, the blocks inverted once on the device
(``kry_bjacobi_create``: Gauss-Jordan with row pivoting, bitwise the
sequential loop), an apply one batched dense block product for up to 256
columns. It pays on systems with several unknowns per node
(``problems.multidof``).
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


def _isai_lower(csr, dt, ctx):
    """W's values and {"longest", "kernel_seconds"} for a canonical lower
    triangular CSR (kry_isai_lower)."""
    n, nnz = csr.shape[0], int(csr.nnz)
    if nnz >= 2**31 - 1 or n >= 2**31 - 1:
        raise NotImplementedError("the approximate inverse indexes entries in int32")
    indptr = np.ascontiguousarray(csr.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
    data = np.ascontiguousarray(csr.data, dtype=dt)
    vals = np.zeros(max(nnz, 1), dtype=dt)
    info = np.zeros(3, dtype=np.int64)
    check(lib.kry_isai_lower(ctx.handle, n, nnz, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                             _lib.dtype_code(dt), _lib.KRY_I32, _lib.ptr(vals),
                             info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    W = scipy.sparse.csr_matrix((vals[:nnz], indices, indptr), shape=(n, n))
    return W, {"longest": int(info[1]), "kernel_seconds": float(info[2]) * 1e-6}


def isai(T, lower=True, dtype=None, device=None, stats=None):
    """The incomplete sparse approximate inverse W of a sparse triangular T
    (scipy.sparse matrix or dense array, on the host) as scipy CSR: W has T's
    pattern and (W T) = I on it. Row i with pattern J (ending in i) is the
    back substitution ``T(J, J)^T w = e_last``, computed on the device bitwise
    as the sequential loop in stored order (``kry_isai_lower``). ``lower=False``:
    ``isai(T^T)^T``, the right inverse with (T W) = I on T's pattern. Every
    row of the triangle must store its diagonal; a zero or non-finite diagonal
    raises ``LinAlgError`` naming the smallest such row, a row of more than
    1024 entries ``NotImplementedError``, an entry on the wrong side of the
    diagonal ``ValueError``. ``stats``: a dict that receives "longest" (row)
    and "kernel_seconds"."""
    csr, dt = _canonical(T, "isai", dtype)
    low = csr if lower else csr.T.tocsr()
    low.sort_indices()
    W, st = _isai_lower(low, dt, get_context(device))
    if stats is not None:
        stats.update(st)
    if not lower:
        W = W.T.tocsr()
        W.sort_indices()
    return W


def _check_solve(solve, sweeps):
    if solve not in ("exact", "isai"):
        raise ValueError(f'solve must be "exact" or "isai", not {solve!r}')
    if int(sweeps) != sweeps or sweeps < 0:
        raise ValueError(f"sweeps must be an integer >= 0, not {sweeps!r}")
    if sweeps > 0 and solve == "exact":
        raise ValueError('sweeps > 0 goes with solve="isai": an exact solve has nothing to relax')
    return solve, int(sweeps)


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
    solve_kind = "exact"
    sweeps = 0
    max_cols = MAX_COLS  # 256 with solve="isai"

    def _setup_isai(self, n, dt, ctx, lower, upper, scale, sweeps, ordering, colors, perm, rank):
        """The two approximate-inverse stages of the factors lower / upper
        (in B's numbering under ordering="multicolor") and SSOR's scale."""
        t0 = time.perf_counter()
        st_l, st_u = {}, {}
        self._W = (isai(lower, True, dtype=dt, device=ctx.device, stats=st_l),
                   isai(upper, False, dtype=dt, device=ctx.device, stats=st_u))
        # both kernels alone, and the calls around them (checks, transposes, copies); tools/bench_precond.py
        self.isai_kernel_seconds = st_l["kernel_seconds"] + st_u["kernel_seconds"]
        self.isai_seconds = time.perf_counter() - t0
        self.solve_kind, self.sweeps, self.max_cols = "isai", sweeps, 256
        t0 = time.perf_counter()

        def image(M):  # in the caller's numbering, which the device keeps
            M = (M if rank is None else _back(M, rank)).astype(dt)
            M.sort_indices()
            return CsrOperator(M, ctx=ctx, renumber=False)

        ws = [image(W) for W in self._W]
        ts = [image(T) for T in (lower, upper)] if sweeps else [None, None]
        sv = None if scale is None else DeviceVector.from_host(
            ctx, (scale if rank is None else scale[rank]).reshape(-1, 1), dtype=dt)
        self.image_seconds = time.perf_counter() - t0
        self._begin(n, dt, ctx, ws + ts + [sv], ordering, colors, perm)
        for W, T, s in ((ws[0], ts[0], sv), (ws[1], ts[1], None)):
            check(lib.kry_precond_add_isai(self.handle, W.handle, None if T is None else T.handle, sweeps,
                                           None if s is None else s.handle))
        self._isai_images = list(zip(ws, ts))

    def _begin(self, n, dt, ctx, stages, ordering, colors, perm):
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

    def _setup(self, n, dt, ctx, stages, ordering="natural", colors=None, perm=None):
        self._begin(n, dt, ctx, stages, ordering, colors, perm)
        h = self.handle
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
        fuses matching level boundaries (kry_precond_info); "solve" ("exact" or
        "isai") and "sweeps"}. With solve="isai" a stage is {"isai": W's device
        image (CsrOperator.layout), "triangle": T's (None without sweeps),
        "sweeps", "scale": whether the row scale rides on its last store}, and
        "launches" counts the SpMVs: 2 + 4 sweeps."""
        info = np.zeros(5, dtype=np.int64)
        check(lib.kry_precond_info(self.handle, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        sizes = None if self.colors is None else [int(c) for c in np.bincount(self.colors)]
        if self.solve_kind == "isai":
            stages = [{"isai": W.layout(), "triangle": None if T is None else T.layout(), "sweeps": self.sweeps,
                       "scale": i == 0 and self._stages[-1] is not None}
                      for i, (W, T) in enumerate(self._isai_images)]
        else:
            stages = [s.layout() if isinstance(s, TriangularOperator) else {"scale": self.n} for s in self._stages]
        return {"stages": stages, "solve": self.solve_kind, "sweeps": self.sweeps,
                "ordering": self.ordering, "colors": None if sizes is None else len(sizes), "color_sizes": sizes,
                "launches": int(info[0]), "fused": bool(info[1])}

    def matvec_device(self, x, y):
        """y = P x for DeviceVectors (n x k, k a power of two <= 64, 256 with
        solve="isai", this preconditioner's dtype) in the caller's numbering;
        y may be x."""
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
        if kp > self.max_cols:
            raise NotImplementedError(
                f"at most {self.max_cols} right-hand-side columns on a factorised preconditioner"
                + ("" if self.max_cols > MAX_COLS else ' (256 with solve="isai")'))
        if kp != k:
            y2 = np.concatenate([y2, np.zeros((self.n, kp - k), dtype=self.dtype)], axis=1)
        yv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        yv.upload(y2)
        xv = DeviceVector(self.ctx, self.n, kp, self.dtype)
        self.matvec_device(yv, xv)
        return np.ascontiguousarray(xv.to_host()[:, :k]).reshape(y.shape)

    __matmul__ = solve

    def inverses(self):
        """(W_L, W_U) as scipy CSR with solve="isai": the approximate inverses
        of the two factors on the factors' patterns, (W_L L) = I on L's and
        (U W_U) = I on U's, in the numbering of ``factors()``."""
        if self.solve_kind != "isai":
            raise ValueError('inverses() goes with solve="isai": this object solves its factors exactly')
        return self._W

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
    multicolour elimination order instead of by index (the module's notes).
    ``solve="isai"``: each solve is a product with the factor's approximate
    inverse and ``sweeps`` relaxation steps (the module's notes)."""

    def __init__(self, A, omega=1.0, dtype=None, device=None, ordering="natural", solve="exact", sweeps=0):
        solve, sweeps = _check_solve(solve, sweeps)
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
        if solve == "isai":
            self._setup_isai(n, dt, ctx, self._lower, self._upper, self._scale, sweeps, ordering, colors, perm, rank)
            return
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
    is the row an error names. ``solve="isai"``: each solve is a product with
    the factor's approximate inverse and ``sweeps`` relaxation steps (the
    module's notes)."""

    def __init__(self, A, dtype=None, device=None, ordering="natural", solve="exact", sweeps=0):
        solve, sweeps = _check_solve(solve, sweeps)
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
        if solve == "isai":
            self._setup_isai(n, dt, ctx, self._L, self._U, None, sweeps, ordering, colors, perm, rank)
            return
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


class BlockJacobiPreconditioner(_Factored):
    """``M = blockdiag(A_11, ..., A_mm)^-1``: the diagonal blocks of A over a
    partition of its rows, inverted once on the device; an apply is one
    launch, a batched dense block product, for up to 256 columns.

    ``block_size=b``: blocks of b consecutive rows (the last may be smaller);
    ``blocks=starts``: block i is rows [starts[i], starts[i + 1]), with
    starts[0] = 0, strictly increasing, every start below n, and n closing
    the last block. Exactly one of the two; a block holds 1 to 32 rows
    (``NotImplementedError`` naming the block above that). Block i is the
    dense array of A's stored entries inside it; its inverse is in-place
    Gauss-Jordan with row pivoting in ``dtype`` scalars, and the apply sums
    ``X[r, j] * x[j]`` over j ascending: both bitwise the sequential loops
    (include/krylov_hip.h). A block with a zero or non-finite pivot raises
    ``LinAlgError`` naming the smallest such block and its first row.
    ``A``: scipy.sparse matrix or dense array; ``dtype``: the dtype of the
    vectors it will precondition (default A's)."""

    max_cols = 256

    def __init__(self, A, block_size=None, blocks=None, dtype=None, device=None):
        if (block_size is None) == (blocks is None):
            raise ValueError("BlockJacobiPreconditioner takes exactly one of block_size= and blocks=")
        csr, dt = _canonical(A, "BlockJacobiPreconditioner", dtype)
        n, nnz = csr.shape[0], int(csr.nnz)
        if nnz >= 2**31 - 1 or n >= 2**31 - 1:
            raise NotImplementedError("block-Jacobi indexes entries in int32")
        if block_size is not None:
            if int(block_size) != block_size or block_size < 1:
                raise ValueError(f"block_size must be an integer >= 1, not {block_size!r}")
            if block_size > 32:
                raise NotImplementedError(f"block_size={int(block_size)}: block-Jacobi takes blocks of at most 32 rows")
            starts = np.arange(0, n, int(block_size), dtype=np.int32)
        else:
            raw = np.asarray(blocks)
            if raw.ndim != 1 or (raw.size and not np.issubdtype(raw.dtype, np.integer)):
                raise ValueError("blocks must be a 1-D array of integer row indices (the first row of every block)")
            if raw.size and (raw.min() < 0 or raw.max() >= 2**31):
                raise ValueError("blocks must hold row indices in [0, n)")
            starts = np.ascontiguousarray(raw, dtype=np.int32)
        ctx = get_context(device)
        indptr = np.ascontiguousarray(csr.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(csr.indices, dtype=np.int32)
        data = np.ascontiguousarray(csr.data, dtype=dt)
        info = np.zeros(3, dtype=np.int64)
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        check(lib.kry_bjacobi_create(ctx.handle, n, nnz, _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                     _lib.dtype_code(dt), _lib.KRY_I32, starts.shape[0], _lib.ptr(starts),
                                     info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(h)))
        # plan, uploads, the factor kernels and the wait for them (tools/bench_precond.py)
        self.factor_seconds = time.perf_counter() - t0
        self.factor_kernel_seconds = float(info[2]) * 1e-6
        self._bj = h
        self._bj_fin = _lib.own(self, lib.kry_bjacobi_destroy, h)
        self.blocks = np.concatenate([starts, np.array([n], dtype=np.int32)])
        self._begin(n, dt, ctx, [], "natural", None, None)
        check(lib.kry_precond_add_bjacobi(self.handle, h))

    def inverse_blocks(self):
        """The inverses as the device holds them: a list of (b_i, b_i) arrays."""
        sizes = np.diff(self.blocks).astype(np.int64)
        flat = np.zeros(max(int(np.sum(sizes * sizes)), 1), dtype=self.dtype)
        check(lib.kry_bjacobi_get(self._bj, _lib.ptr(flat)))
        offs = np.concatenate([[0], np.cumsum(sizes * sizes)])
        return [flat[offs[i]:offs[i + 1]].reshape(int(b), int(b)).copy() for i, b in enumerate(sizes)]

    def layout(self):
        """{"blocks" (count), "block_sizes": (min, max), "value_bytes" (the
        inverses), "map_bytes" (the row-to-block map and the block tables),
        "launches": 1, "factor_kernel_seconds", "solve": "exact", "fused":
        False, "ordering": "natural"}."""
        info = np.zeros(6, dtype=np.int64)
        check(lib.kry_bjacobi_info(self._bj, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        pin = np.zeros(5, dtype=np.int64)
        check(lib.kry_precond_info(self.handle, pin.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return {"blocks": int(info[0]), "block_sizes": (int(info[1]), int(info[2])), "value_bytes": int(info[3]),
                "map_bytes": int(info[4]), "launches": int(pin[0]), "factor_kernel_seconds": float(info[5]) * 1e-6,
                "solve": self.solve_kind, "sweeps": 0, "fused": bool(pin[1]), "ordering": "natural", "colors": None}

    def close(self):
        self._fin()
        self._bj_fin()
