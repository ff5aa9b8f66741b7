"""Descriptor classes of the SELL-128/DIA image on the MI355X.

A slice's descriptor block (its width and, per slot column, the offset, both
lane masks, the uniform flag and the uniform value's bits) depends only on
where the grid's boundaries fall inside its 128 rows, so the slices of a
stencil or a band share a few distinct blocks. The image groups byte-equal
blocks into classes, numbered by first occurrence, and the single-RHS kernel
reads a slice's class word and the class's columns from a table of the
distinct blocks instead of the slice's own copy. The image takes classes only
when the table is smaller than the per-slice descriptors and within 1 MiB;
KRY_DIA_CLASSES=0 and KRY_DIA_CLASS_MAX_BYTES (read at an operator's first
use) keep the per-slice arrays. The descriptors a wave reads are the same
bytes either way, so is everything after them: the SpMV, its fused epilogues
and whole solves are compared bit for bit, and against SciPy bitwise with NaN
for NaN (tests/test_gpu_dia_uniform.py).

The class counts are those of the host builder (an exact map over the block
bytes; tests/test_dia_classes_host.py asserts them without a device)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

from tests.test_gpu_dia_uniform import _band, _bits_equal, _bits_equal_scipy, _mixed, _wide_x

pytestmark = pytest.mark.gpu

NAMES = ["stencil15_5", "stencil15_8", "stencil15_12", "stencil15_16", "stencil15_24", "poisson2d_61", "poisson2d_64",
         "band21_uniform", "band15_third_random"]
# no classes: one slice; grid rows of 61 against slices of 128, so the +-1 columns' masks differ in every slice
UNSHARED = ("stencil15_5", "poisson2d_61")
# (classes, class-table columns) of the 15-point stencils
COUNTS = {"stencil15_8": (3, 45), "stencil15_12": (13, 185), "stencil15_16": (6, 70), "stencil15_24": (16, 200)}


def _matrices():
    from krylov_amd import problems

    return {
        "stencil15_5": lambda: problems.stencil15_3d(5),  # one ragged slice: one class, nothing shared
        "stencil15_8": lambda: problems.stencil15_3d(8),  # 4 slices, 3 classes
        "stencil15_12": lambda: problems.stencil15_3d(12),  # 14 slices, 13 classes, ragged last slice
        "stencil15_16": lambda: problems.stencil15_3d(16),  # 32 slices, 6 classes
        "stencil15_24": lambda: problems.stencil15_3d(24),  # 108 slices, 16 classes
        "poisson2d_61": lambda: problems.poisson2d(61),  # at most 8 slot columns per slice; nothing shared
        "poisson2d_64": lambda: problems.poisson2d(64),  # the same kernel (8 per round), two grid rows per slice: shared
        # 21 columns: the last class's second round is partial and reads on into the table's padding
        "band21_uniform": lambda: _band(1001, list(range(-10, 11)), 10**9, 0),
        "band15_third_random": lambda: _mixed()["band15_third_random"],  # UNI = 1: values streamed, descriptors shared
    }


def _csr(A, dtype):
    A = scipy.sparse.csr_matrix(A, dtype=dtype)
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def _random_holes(n=1500, seed=11):
    """A 9-diagonal band whose rows each lose random entries: no two slices
    have the same masks, so every slice is a class of its own."""
    rng = np.random.default_rng(seed)
    A = _band(n, list(range(-4, 5)), 10**9, 0).tocoo()
    keep = (rng.random(A.nnz) > 0.3) | (A.row == A.col)
    return _csr(scipy.sparse.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), shape=A.shape), np.float64)


def _compare(a, b):
    from krylov_amd import _lib

    out = np.zeros(2, dtype=np.int64)
    _lib.check(_lib.lib.kry_csr_compare(a.handle, b.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return int(out[0]), int(out[1])


def _op(A, monkeypatch, classes=True, uniform=True, lean=True, max_bytes=None):
    """An operator with the given switches; layout() makes it choose its
    kernel while they are set."""
    import krylov_amd

    env = {"KRY_DIA_CLASSES": None if classes else "0", "KRY_DIA_UNIFORM": None if uniform else "0",
           "KRY_DIA_LEAN": None if lean else "0", "KRY_DIA_CLASS_MAX_BYTES": max_bytes}
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    op = krylov_amd.CsrOperator(A)
    lay = op.layout()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    assert lay["dia"] and lay["dia_lean"] == lean
    return op, lay


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("name", sorted(COUNTS))
def test_class_counts(name, uniform, monkeypatch):
    """The counts of the issue's table, with and without uniform detection,
    on the device-built image, and 0 / 0 with classes switched off."""
    A = _csr(_matrices()[name](), np.float64)
    _, lay = _op(A, monkeypatch, uniform=uniform)
    assert (lay["dia_classes"], lay["dia_class_cols"]) == COUNTS[name]
    assert lay["dia_class_cols"] < lay["dia_slots"] // 128
    _, lay0 = _op(A, monkeypatch, classes=False, uniform=uniform)
    assert (lay0["dia_classes"], lay0["dia_class_cols"]) == (0, 0)


@pytest.mark.parametrize("types", ["f64", "f32", "f64_over_f32"])
@pytest.mark.parametrize("name", NAMES)
def test_classes_spmv_bitwise(name, types, monkeypatch):
    """op @ x with classes against SciPy and against the class-free operator,
    for uniform detection on and off and the lean and the per-lane kernel. x
    from _wide_x: a hole's partner value that must not leak is there."""
    mdt = np.float64 if types == "f64" else np.float32
    xdt = np.float32 if types == "f32" else np.float64
    A = _csr(_matrices()[name](), mdt)
    x = _wide_x(A.shape[0], xdt)
    ref = A @ x
    for uniform in (True, False):
        for lean in (True, False):
            on, lay = _op(A, monkeypatch, uniform=uniform, lean=lean)
            off, lay0 = _op(A, monkeypatch, classes=False, uniform=uniform, lean=lean)
            assert lay0["dia_classes"] == 0
            if name in UNSHARED:
                assert lay["dia_classes"] == 0
            else:
                assert 0 < lay["dia_class_cols"] < lay["dia_slots"] // 128
            if name in COUNTS:
                assert (lay["dia_classes"], lay["dia_class_cols"]) == COUNTS[name]
            y = on @ x
            assert y.dtype == xdt
            _bits_equal(y, off @ x)
            _bits_equal_scipy(y, ref)


def test_no_shared_blocks_no_classes(monkeypatch):
    """Random holes per row: every slice is its own class, the table would
    not be smaller, the image records none and runs as before."""
    A = _random_holes()
    x = _wide_x(A.shape[0], np.float64)
    on, lay = _op(A, monkeypatch)
    off, _ = _op(A, monkeypatch, classes=False)
    assert (lay["dia_classes"], lay["dia_class_cols"]) == (0, 0)
    y = on @ x
    _bits_equal(y, off @ x)
    _bits_equal_scipy(y, A @ x)


def test_class_table_size_limit(monkeypatch):
    """stencil15_3d(24): 200 table columns of 32 bytes. With the limit one
    byte below, the operator keeps the per-slice arrays; at the table's size
    it takes the classes. The same bits each way."""
    from krylov_amd import problems

    A = _csr(problems.stencil15_3d(24), np.float64)
    x = _wide_x(A.shape[0], np.float64)
    small, lay_s = _op(A, monkeypatch, max_bytes=200 * 32 - 1)
    fits, lay_f = _op(A, monkeypatch, max_bytes=200 * 32)
    off, _ = _op(A, monkeypatch, classes=False)
    assert (lay_s["dia_classes"], lay_s["dia_class_cols"]) == (0, 0)
    assert (lay_f["dia_classes"], lay_f["dia_class_cols"]) == (16, 200)
    y = small @ x
    _bits_equal(y, off @ x)
    _bits_equal(y, fits @ x)
    _bits_equal_scipy(y, A @ x)


@pytest.mark.parametrize("name", NAMES + ["random_holes"])
def test_class_builders_agree(name, monkeypatch):
    """The device build's class words and table against the host builder's,
    byte for byte (kry_csr_compare, whose list now ends with them), and both
    against the host plan's counts."""
    import krylov_amd
    from krylov_amd import _lib

    A = _random_holes() if name == "random_holes" else _csr(_matrices()[name](), np.float64)
    for v in ("KRY_DIA_CLASSES", "KRY_DIA_UNIFORM", "KRY_DIA_LEAN", "KRY_DIA_CLASS_MAX_BYTES"):
        monkeypatch.delenv(v, raising=False)
    dev = krylov_amd.CsrOperator(A)
    monkeypatch.setenv("KRY_DEVICE_BUILD", "0")
    host = krylov_amd.CsrOperator(A)
    lay = dev.layout()
    assert lay["dia"] and lay == host.layout()
    assert _compare(dev, host) == (0, 0)
    plan = _lib.dia_class_plan(A.indptr, A.indices, A.data)
    assert (lay["dia_classes"], lay["dia_class_cols"]) == (plan["classes"], plan["class_cols"])
    if name in COUNTS:
        assert (plan["classes"], plan["class_cols"]) == COUNTS[name]


@pytest.mark.parametrize("solver", ["cg", "gmres", "minres"])
def test_classes_through_the_solvers(solver, monkeypatch):
    """50 CG steps at tol 0 (one launch per step: the Ap / <p, Ap> epilogue)
    and one GMRES(30) cycle (the scaled source) on the 15-point stencil 24^3,
    30 MINRES steps (the Lanczos epilogue) on a 12^3 row-scaled Laplacian in
    its weighted inner product: iterates and every residual norm bit for bit
    between classes on and off. The grid does not depend on the classes."""
    import krylov_amd
    from krylov_amd import problems

    monkeypatch.setenv("KRY_CG_PERSIST", "0")
    kw = {}
    if solver == "minres":
        A, w = problems.shifted_lap3d_weighted(12)
        b = np.random.default_rng(4).standard_normal(A.shape[0]).astype(np.float32)
        kw["inner"] = krylov_amd.WeightedInner(w)
        steps = 30
    else:
        A = problems.stencil15_3d(24)
        b = np.random.default_rng(4).standard_normal(A.shape[0])
        steps = 50 if solver == "cg" else 30
    A = _csr(A, A.dtype)
    res = []
    for classes in (True, False):
        op, lay = _op(A, monkeypatch, classes=classes)
        assert (lay["dia_classes"] > 0) == classes
        _, info = getattr(krylov_amd, solver)(op, b, tol=0.0, atol=0.0, maxiter=steps, **kw)
        assert info.numsteps == steps
        res.append(info)
    _bits_equal(np.asarray(res[0].resnorms), np.asarray(res[1].resnorms))
    _bits_equal(res[0].xk, res[1].xk)
    assert np.all(np.isfinite(res[0].xk)) and res[0].resnorms[-1] < res[0].resnorms[0]
