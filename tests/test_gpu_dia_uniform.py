"""Uniform slot columns of the SELL-128/DIA image on the MI355X.

Where every present row of a slot column stores one bit pattern (the
diagonals of a constant-coefficient stencil), the single-RHS SpMV takes the
value from the slot column's descriptor and does not read its 128 stored
values. The products, their order and the hole handling are unchanged, so an
operator built with detection off (KRY_DIA_UNIFORM=0) and one built by default
give the same bits, in one SpMV and through whole solves, and both builders
(device kernels, host threads) flag the same columns.

Against SciPy the comparison is bitwise wherever the result is not a NaN and
NaN for NaN elsewhere: IEEE 754 leaves the payload and the sign of a produced
NaN to the implementation, so x86 and the GPU may differ there; between the
two operators, which run the same instructions on the same operands, every
bit is compared, NaNs included."""
import ctypes

import numpy as np
import pytest
import scipy.sparse

from tests import dia_uniform_cases as UC

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def _bits_equal_scipy(y, ref):
    y, ref = np.asarray(y), np.asarray(ref)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(y), nan)
    _bits_equal(y[~nan], ref[~nan])


def _compare(a, b):
    from krylov_amd import _lib

    out = np.zeros(2, dtype=np.int64)
    _lib.check(_lib.lib.kry_csr_compare(a.handle, b.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return int(out[0]), int(out[1])


def _band(n, offsets, random_every, seed, dtype=np.float64):
    """Full band: diagonal t of `offsets` is random when t % random_every ==
    random_every - 1, else the constant t + 1.5."""
    rng = np.random.default_rng(seed)
    diags = []
    for t, o in enumerate(offsets):
        m = n - abs(o)
        diags.append(rng.uniform(1.0, 2.0, m) if t % random_every == random_every - 1 else np.full(m, t + 1.5))
    A = scipy.sparse.diags(diags, offsets, shape=(n, n), format="csr", dtype=dtype)
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    assert A.nnz == sum(n - abs(o) for o in offsets)
    return A


def _mixed():
    from krylov_amd import problems

    P = problems.poisson2d(40).tocsr().copy()  # n = 1,600; offsets -40, -1, 0, 1, 40
    rng = np.random.default_rng(5)
    diag = P.indices == np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    P.data[diag] = rng.uniform(4.0, 5.0, P.shape[0])
    return {
        "poisson40_random_diag": P,  # uniform and streamed slot columns in one round of UNR = 8
        "band15_third_random": _band(600, list(range(-7, 8)), 3, 6),  # 15 offsets: the UNR = 16 kernel
        "band21_two_rounds": _band(600, list(range(-10, 11)), 4, 7),  # more than 16 offsets: two rounds per slice
    }


def _all_matrices():
    from krylov_amd import problems

    m = dict(UC.plan_matrices())
    m["stencil15_12"] = problems.stencil15_3d(12)
    m.update(_mixed())
    return m


NAMES = ["stencil15_7", "poisson2d_61", "tridiag_special", "shifted_lap3d_f32", "stencil15_12",
         "poisson40_random_diag", "band15_third_random", "band21_two_rounds"]
CONSTANT = ("stencil15_7", "poisson2d_61", "stencil15_12")


def _wide_x(n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    spread = 20 if np.dtype(dtype) == np.float64 else 8
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-spread, spread, n)).astype(dtype)


def _pair(A, monkeypatch):
    """(operator built by default, operator built with detection off)"""
    import krylov_amd

    monkeypatch.delenv("KRY_DIA_UNIFORM", raising=False)
    on = krylov_amd.CsrOperator(A)
    monkeypatch.setenv("KRY_DIA_UNIFORM", "0")
    off = krylov_amd.CsrOperator(A)
    monkeypatch.delenv("KRY_DIA_UNIFORM")
    return on, off


def _check_spmv(name, xdt, monkeypatch):
    from krylov_amd import _lib

    A = _all_matrices()[name]
    xdt = A.dtype if xdt is None else xdt
    on, off = _pair(A, monkeypatch)
    lay, lay0 = on.layout(), off.layout()
    assert lay["dia"] and lay0["dia"]
    cols = lay["dia_slots"] // 128
    assert lay0["dia_uniform_cols"] == 0
    assert lay0["dia_value_bytes"] == lay["dia_slots"] * A.dtype.itemsize
    assert lay["dia_value_bytes"] == (cols - lay["dia_uniform_cols"]) * 128 * A.dtype.itemsize
    up = _lib.dia_uniform_plan(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)
    assert lay["dia_uniform_cols"] == up["uniform"] and cols == up["cols"]
    if name in CONSTANT:
        assert lay["dia_uniform_cols"] == cols
    if name == "tridiag_special":
        assert lay["dia_uniform_cols"] == sum(UC.TRIDIAG_FLAGS)
    if name in _mixed():
        assert 0 < lay["dia_uniform_cols"] < cols
    x = _wide_x(A.shape[0], xdt)
    y, y0 = on @ x, off @ x
    assert y.dtype == np.result_type(A.dtype, xdt)
    _bits_equal(y, y0)
    _bits_equal_scipy(y, A @ x)


@pytest.mark.parametrize("name", NAMES)
def test_uniform_spmv_bitwise(name, monkeypatch):
    _check_spmv(name, None, monkeypatch)


def test_uniform_spmv_f64_vector_over_f32_matrix(monkeypatch):
    assert _all_matrices()["shifted_lap3d_f32"].dtype == np.float32
    _check_spmv("shifted_lap3d_f32", np.float64, monkeypatch)


@pytest.mark.parametrize("name", ["poisson40_random_diag", "band15_third_random", "band21_two_rounds"])
def test_mixed_slices(name, monkeypatch):
    """Uniform and streamed slot columns inside one round of the kernel, in
    the 8-wide and the 16-wide instantiation and over two rounds."""
    from krylov_amd import _lib

    A = _mixed()[name]
    plan = _lib.dia_plan(A.indptr, A.indices)
    up = _lib.dia_uniform_plan(A.indptr, A.indices, A.data)
    want_w = {"poisson40_random_diag": 5, "band15_third_random": 15, "band21_two_rounds": 21}[name]
    assert plan["max_width"] == want_w
    unr = 16 if want_w > 8 else 8
    f = up["flags"][:want_w]  # the first slice: every round holds both kinds
    for r0 in range(0, want_w, unr):
        assert 0 < f[r0:r0 + unr].sum() < len(f[r0:r0 + unr])
    on, off = _pair(A, monkeypatch)
    assert on.layout()["dia_uniform_cols"] == up["uniform"]
    x = _wide_x(A.shape[0], A.dtype, seed=3)
    y = on @ x
    _bits_equal(y, off @ x)
    _bits_equal_scipy(y, A @ x)


def test_uniform_holes_are_never_read(monkeypatch):
    """tests/test_gpu_dia.py::test_dia_holes_are_never_read with uniform
    off-diagonals: row 5 lacks the -1 offset its (uniform) slot column holds;
    x[4] = NaN reaches rows 3 and 4 only, y[5] stays finite."""
    n = 200
    ent = []
    for r in range(n):
        for o, v in ((-1, -1.0), (0, 4.0), (1, -2.0)):
            c = r + o
            if 0 <= c < n and not (r == 5 and o == -1):
                ent.append((r, c, v))
    A = UC.csr_from_rows(n, ent)
    on, off = _pair(A, monkeypatch)
    assert on.layout()["dia"] and on.layout()["dia_uniform_cols"] == on.layout()["dia_slots"] // 128 == 6
    x = np.arange(1.0, n + 1.0)
    x[4] = np.nan
    y, ref = on @ x, A @ x
    assert np.isfinite(y[5]) and np.isnan(y[3]) and np.isnan(y[4])
    _bits_equal(y, off @ x)
    _bits_equal_scipy(y, ref)


def test_uniform_explicit_zero_column_meets_inf(monkeypatch):
    """A uniform slot column whose value is an explicit 0.0 is still
    multiplied: 0 * inf = NaN in row 8, as SciPy's csr_matvec gives."""
    n = 200
    ent = []
    for r in range(n):
        for o, v in ((-1, -1.0), (0, 4.0), (1, 0.0)):
            if 0 <= r + o < n:
                ent.append((r, r + o, v))
    A = UC.csr_from_rows(n, ent)
    assert A.nnz == 3 * n - 2
    on, off = _pair(A, monkeypatch)
    assert on.layout()["dia_uniform_cols"] == 6
    x = np.arange(1.0, n + 1.0)
    x[9] = np.inf
    y, ref = on @ x, A @ x
    assert np.isnan(ref[8]) and np.isnan(y[8]) and np.isinf(y[9]) and np.isinf(y[10])
    assert np.count_nonzero(np.isnan(y)) == 1
    _bits_equal(y, off @ x)
    _bits_equal_scipy(y, ref)


@pytest.mark.parametrize("solver", ["cg", "minres", "gmres"])
def test_uniform_solvers_bitwise(solver, monkeypatch):
    """20 CG steps (one launch per step: KRY_CG_PERSIST=0, the EpiApDot
    epilogue), 20 MINRES steps and one GMRES(30) cycle on the 15-point stencil
    16^3: histories and iterates bit for bit with detection on and off."""
    import krylov_amd
    from krylov_amd import problems

    monkeypatch.setenv("KRY_CG_PERSIST", "0")
    A = problems.stencil15_3d(16)
    on, off = _pair(A, monkeypatch)
    assert on.layout()["dia_uniform_cols"] == on.layout()["dia_slots"] // 128 and off.layout()["dia_uniform_cols"] == 0
    b = np.random.default_rng(4).standard_normal(A.shape[0])
    steps = 30 if solver == "gmres" else 20
    res = []
    for op in (on, off):
        _, info = getattr(krylov_amd, solver)(op, b, tol=0.0, atol=0.0, maxiter=steps)
        assert info.numsteps == steps
        res.append(info)
    _bits_equal(np.asarray(res[0].resnorms), np.asarray(res[1].resnorms))
    _bits_equal(res[0].xk, res[1].xk)
    assert np.all(np.isfinite(res[0].xk)) and res[0].resnorms[-1] < res[0].resnorms[0]


@pytest.mark.parametrize("name", NAMES)
def test_uniform_builders_agree(name, monkeypatch):
    """The device build and the host builders flag the same slot columns with
    the same values (kry_csr_compare: no differing item, the new bits
    included), and both match the host plan."""
    import krylov_amd
    from krylov_amd import _lib

    A = _all_matrices()[name]
    monkeypatch.delenv("KRY_DIA_UNIFORM", raising=False)
    dev = krylov_amd.CsrOperator(A)
    monkeypatch.setenv("KRY_DEVICE_BUILD", "0")
    host = krylov_amd.CsrOperator(A)
    assert dev.layout() == host.layout()
    assert _compare(dev, host) == (0, 0)
    up = _lib.dia_uniform_plan(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)
    assert dev.layout()["dia_uniform_cols"] == up["uniform"]
    # the comparison sees the new arrays: detection off differs in them alone
    monkeypatch.setenv("KRY_DIA_UNIFORM", "0")
    plain = krylov_amd.CsrOperator(A)
    nd, mask = _compare(host, plain)
    assert (nd > 0) == (up["uniform"] > 0) and mask & ~(0b111 << 23) == 0
