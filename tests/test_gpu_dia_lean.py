"""The lean single-RHS kernel of the SELL-128/DIA image on the MI355X.

By default the kernel takes a slot column's two 64-bit lane masks as the
select masks of its accumulator updates, and loads x through a bounds-checked
buffer descriptor over x[-1, n + 1) at a 32-bit byte offset, so a masked-off
lane forms no address of its own: where its run of x lies outside the
descriptor it reads 0 without touching memory, elsewhere it reads an element
of x that the select then drops. KRY_DIA_LEAN=0 keeps the kernel that tests
the mask bit per lane and steers a masked-off lane to x[0]; an operator whose
vectors do not fit a 32-bit byte offset takes that kernel too
(KRY_DIA_LEAN_MAX_BYTES lowers the limit). Present lanes load the same pairs
and run the same products, adds and selects, so the two kernels give the same
bits: in one SpMV, through every fused epilogue and through whole solves.

Against SciPy the comparison is bitwise wherever the result is not a NaN and
NaN for NaN elsewhere (tests/test_gpu_dia_uniform.py); between the two
kernels every bit is compared."""
import numpy as np
import pytest
import scipy.sparse

from tests.test_gpu_dia_uniform import _band, _bits_equal, _bits_equal_scipy, _mixed, _wide_x

pytestmark = pytest.mark.gpu


NAMES = ["stencil15_5", "stencil15_8", "stencil15_23", "stencil15_24", "poisson2d_61", "band21_uniform",
         "band15_third_random"]


def _matrices():
    from krylov_amd import problems

    return {
        "stencil15_5": lambda: problems.stencil15_3d(5),  # n = 125: one ragged slice, odd n (single-row tail)
        "stencil15_8": lambda: problems.stencil15_3d(8),  # 4 slices, holes on all three boundaries in each
        "stencil15_23": lambda: problems.stencil15_3d(23),  # odd plane offsets, ragged last slice
        "stencil15_24": lambda: problems.stencil15_3d(24),  # slices 1 to 4: runs that start before x
        "poisson2d_61": lambda: problems.poisson2d(61),  # at most 8 slot columns per slice
        "band21_uniform": lambda: _band(1001, list(range(-10, 11)), 10**9, 0),  # two rounds, the second partial
        "band15_third_random": lambda: _mixed()["band15_third_random"],  # uniform and streamed columns: UNI = 1
    }


def _csr(A, dtype):
    A = scipy.sparse.csr_matrix(A, dtype=dtype)
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def _pair(A, monkeypatch, uniform=True):
    """(operator on the lean kernel, operator on the per-lane kernel); the
    choice is made at an operator's first use, here by layout()."""
    import krylov_amd

    if uniform:
        monkeypatch.delenv("KRY_DIA_UNIFORM", raising=False)
    else:
        monkeypatch.setenv("KRY_DIA_UNIFORM", "0")
    monkeypatch.delenv("KRY_DIA_LEAN", raising=False)
    monkeypatch.delenv("KRY_DIA_LEAN_MAX_BYTES", raising=False)
    lean = krylov_amd.CsrOperator(A)
    assert lean.layout()["dia"] and lean.layout()["dia_lean"]
    monkeypatch.setenv("KRY_DIA_LEAN", "0")
    old = krylov_amd.CsrOperator(A)
    assert old.layout()["dia"] and not old.layout()["dia_lean"]
    monkeypatch.delenv("KRY_DIA_LEAN")
    monkeypatch.delenv("KRY_DIA_UNIFORM", raising=False)
    return lean, old


@pytest.mark.parametrize("types", ["f64", "f32", "f64_over_f32"])
@pytest.mark.parametrize("name", NAMES)
def test_lean_spmv_bitwise(name, types, monkeypatch):
    """op @ x against SciPy and against the per-lane kernel, with uniform
    slot columns detected (UNI = 2, or 1 on the mixed band) and with detection
    off (UNI = 0)."""
    mdt = np.float64 if types == "f64" else np.float32
    xdt = np.float32 if types == "f32" else np.float64
    A = _csr(_matrices()[name](), mdt)
    x = _wide_x(A.shape[0], xdt)
    ref = A @ x
    for uniform in (True, False):
        lean, old = _pair(A, monkeypatch, uniform)
        cols = lean.layout()["dia_slots"] // 128
        want = 0 if not uniform else None if name == "band15_third_random" else cols
        if want is None:
            assert 0 < lean.layout()["dia_uniform_cols"] < cols
        else:
            assert lean.layout()["dia_uniform_cols"] == want
        y = lean @ x
        assert y.dtype == xdt
        _bits_equal(y, old @ x)
        _bits_equal_scipy(y, ref)


def _touching(A, cols):
    P = A.copy()
    P.data[:] = 1.0
    return np.asarray(P[:, cols].sum(axis=1)).ravel() > 0


@pytest.mark.parametrize("uniform", [True, False])
def test_lean_masked_and_out_of_range_lanes_leak_nothing(uniform, monkeypatch):
    """NaN at both ends of x and inside, and an inf: every lane now loads its
    pair wherever the slot column's offset puts it, so masked-off lanes read
    these values (or 0 past the descriptor) and must drop them. Rows whose
    stencil does not touch them are finite and bitwise SciPy; rows that touch
    a NaN are NaN; the rest (inf) are SciPy's."""
    from krylov_amd import problems

    A = _csr(problems.stencil15_3d(8), np.float64)
    n = A.shape[0]
    x = np.random.default_rng(2).standard_normal(n)
    nans, infs = [0, n - 1, 201], [330]
    x[nans] = np.nan
    x[infs] = np.inf
    lean, old = _pair(A, monkeypatch, uniform)
    y, ref = lean @ x, A @ x
    clean = ~_touching(A, nans + infs)
    assert 0 < clean.sum() < n and np.all(np.isfinite(ref[clean]))
    assert np.all(np.isfinite(y[clean]))
    _bits_equal(y[clean], ref[clean])
    assert np.all(np.isnan(y[_touching(A, nans)]))
    _bits_equal_scipy(y, ref)
    _bits_equal(y, old @ x)


def test_lean_holes_are_never_read(monkeypatch):
    """tests/test_gpu_dia.py::test_dia_holes_are_never_read on the lean
    kernel: (5, 4) is a hole of the -1 slot column and x[4] = NaN, so y[5]
    stays finite; the explicit zero at (8, 9) meets x[9] = inf: NaN."""
    n = 200
    rows, cols, vals = [], [], []
    for r in range(n):
        for off, v in ((-1, -1.0), (0, 4.0), (1, -2.0)):
            c = r + off
            if 0 <= c < n and not (r == 5 and off == -1):
                rows.append(r)
                cols.append(c)
                vals.append(0.0 if (r == 8 and off == 1) else v)
    indptr = np.searchsorted(np.asarray(rows), np.arange(n + 1)).astype(np.int32)
    A = scipy.sparse.csr_matrix((np.asarray(vals), np.asarray(cols, dtype=np.int32), indptr), shape=(n, n))
    assert A.nnz == len(vals) and A.has_sorted_indices
    x = np.arange(1.0, n + 1.0)
    x[4] = np.nan
    x[9] = np.inf
    ref = A @ x
    for uniform in (True, False):
        lean, old = _pair(A, monkeypatch, uniform)
        y = lean @ x
        assert np.isfinite(y[5]) and np.isnan(y[3]) and np.isnan(y[4]) and np.isnan(y[8])
        _bits_equal_scipy(y, ref)
        _bits_equal(y, old @ x)


@pytest.mark.parametrize("solver", ["cg", "minres", "gmres"])
def test_lean_epilogues_bitwise(solver, monkeypatch):
    """20 CG steps (one launch per step: KRY_CG_PERSIST=0, the Ap / <p, Ap>
    epilogue), 20 MINRES steps (Lanczos epilogue) and one GMRES(20) cycle (the
    scaled source, the basis store) on the 15-point stencil 16^3: histories
    and iterates bit for bit between the two kernels. KRY_DIA_GRID pins the
    grid cap, so both sum the same block partials (the library reads it once
    per process; the cap does not depend on the kernel either way: 32 slices
    run as 8 blocks)."""
    import krylov_amd
    from krylov_amd import problems

    monkeypatch.setenv("KRY_CG_PERSIST", "0")
    monkeypatch.setenv("KRY_DIA_GRID", "5120")
    A = problems.stencil15_3d(16)
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    res = []
    for op in _pair(A, monkeypatch):
        _, info = getattr(krylov_amd, solver)(op, b, tol=0.0, atol=0.0, maxiter=20)
        assert info.numsteps == 20
        res.append(info)
    _bits_equal(np.asarray(res[0].resnorms), np.asarray(res[1].resnorms))
    _bits_equal(res[0].xk, res[1].xk)
    assert np.all(np.isfinite(res[0].xk)) and res[0].resnorms[-1] < res[0].resnorms[0]


def test_lean_size_fallback(monkeypatch):
    """With the byte limit below the vector's size the operator takes the
    per-lane kernel, as layout() reports, and gives the same bits."""
    import krylov_amd
    from krylov_amd import problems

    A = _csr(problems.stencil15_3d(8), np.float64)
    x = _wide_x(A.shape[0], np.float64)
    lean, old = _pair(A, monkeypatch)
    monkeypatch.setenv("KRY_DIA_LEAN_MAX_BYTES", str(A.shape[0] * 8 // 2))
    small = krylov_amd.CsrOperator(A)
    assert small.layout()["dia"] and not small.layout()["dia_lean"]
    monkeypatch.setenv("KRY_DIA_LEAN_MAX_BYTES", str((A.shape[0] + 2) * 8))
    fits = krylov_amd.CsrOperator(A)
    assert fits.layout()["dia_lean"]
    y = small @ x
    _bits_equal(y, old @ x)
    _bits_equal(y, lean @ x)
    _bits_equal(y, fits @ x)
    _bits_equal_scipy(y, A @ x)
