"""The SpMV, the solvers and the small dense kernels at 32 to 256
right-hand-side columns (inputs and the comparison rule:
tests/wide_block_cases.py; their host checks: tests/test_wide_block_cases.py).

SpMV: bitwise SciPy csr_matvecs, which at k = 128 and 256 runs
spmv_sell_kernel with k / 8 column groups (the wave to slice-range mapping,
the grid rounded to a multiple of 8, the grid cap). Solvers: step count,
success, history and iterate against oracle/krylov_ref.py on the same block;
every GMRES case names the MGS path it ran on."""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse

from tests import precond_factored_cases as PC
from tests import wide_block_cases as WB

pytestmark = pytest.mark.gpu


def _assert_bitwise(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def _golden_csr(d, key):
    """The fixture's matrix as stored: unsorted rows and duplicates kept."""
    n = d[f"{key}_indptr"].shape[0] - 1
    A = scipy.sparse.csr_matrix((d[f"{key}_data"], d[f"{key}_indices"], d[f"{key}_indptr"]), shape=(n, n))
    A.indices = d[f"{key}_indices"]
    A.indptr = d[f"{key}_indptr"]
    return A


# ------------------------------------------------------------------- SpMV
@pytest.mark.parametrize("k", WB.WIDE)
@pytest.mark.parametrize("compact", ["1", "0"])
@pytest.mark.parametrize("key", ["f64_i32", "f32_i32"])
def test_spmv_wide_adversarial(golden, key, compact, k, monkeypatch):
    """Unsorted rows, duplicates, explicit zeros, empty rows and the 3000-entry
    irregular slice under 128 and 256 columns at magnitudes 1e+-20 (1e+-8 in
    float32), with int32 and with compact uint16 column indices."""
    import krylov_amd

    monkeypatch.setenv("KRY_SELL_COMPACT", compact)
    A = _golden_csr(golden["spmv"], key)
    op = krylov_amd.CsrOperator(A)
    assert op.layout()["compact"] == (compact == "1") and op.layout()["irregular"] >= 1
    X = WB.wide_x(A.shape[0], k, A.dtype, k)
    _assert_bitwise(op @ X, A @ X)


@pytest.mark.parametrize("k", WB.WIDE)
def test_spmv_wide_int64_image_through_abi(golden, k):
    """The same matrix with int64 indices handed to kry_csr_create (an int64
    image, never compact)."""
    from krylov_amd import _lib
    from krylov_amd.device import DeviceVector, get_context

    d = golden["spmv"]
    key = "f64_i64"
    A = _golden_csr(d, key)
    ctx = get_context()
    ip, ix = d[f"{key}_indptr"].astype(np.int64), d[f"{key}_indices"].astype(np.int64)
    dv = np.ascontiguousarray(d[f"{key}_data"])
    n = ip.shape[0] - 1
    X = WB.wide_x(n, k, dv.dtype, 3 * k)
    h = ctypes.c_void_p()
    _lib.check(_lib.lib.kry_csr_create(ctx.handle, n, ix.shape[0], _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv),
                                       _lib.dtype_code(dv.dtype), _lib.KRY_I64, ctypes.byref(h)))
    try:
        info = np.zeros(7, dtype=np.int64)
        _lib.check(_lib.lib.kry_csr_info_n(h, info.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 7))
        assert info[3] == 0
        x = DeviceVector.from_host(ctx, X)
        y = DeviceVector(ctx, n, k, dv.dtype)
        _lib.check(_lib.lib.kry_spmv(ctx.handle, h, x.handle, y.handle))
        _assert_bitwise(y.to_host(), A @ X)
    finally:
        _lib.lib.kry_csr_destroy(h)


def test_spmv_wide_f32_matrix_f64_block(golden):
    """The float32 matrix under a float64 block of 128 columns (the values
    are upcast exactly, as SciPy upcasts them)."""
    import krylov_amd

    A = _golden_csr(golden["spmv"], "f32_i32")
    X = WB.wide_x(A.shape[0], 128, np.float64, 17)
    got = krylov_amd.CsrOperator(A) @ X
    assert got.dtype == np.float64
    _assert_bitwise(got, A @ X)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", WB.WIDE)
@pytest.mark.parametrize("n", WB.BANDED_ROWS)
def test_spmv_wide_grid_rounding_and_empty_ranges(n, k, dtype):
    """1, 2, 37 and 38 slices: fewer slices than waves per column group, and
    grids that the multiple-of-8 rule extends by blocks without a slice
    (test_wide_block_cases.py shows which shape does which)."""
    import krylov_amd

    A = WB.banded(n, 7, dtype)
    op = krylov_amd.CsrOperator(A)
    assert op.layout()["slices"] == WB.sell_geometry(n, k)["nslices"]
    X = WB.wide_x(n, k, dtype, n + k)
    _assert_bitwise(op @ X, A @ X)


@pytest.mark.parametrize("n,k,dtype", WB.GRID_CAP_SHAPES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_spmv_wide_grid_cap(n, k, dtype):
    """More slice-and-column-group pairs than 4 x 8192 waves: the grid is
    capped and waves walk two slices. (The two large shapes of this file.)"""
    import krylov_amd

    A = WB.banded(n, 11, dtype)
    op = krylov_amd.CsrOperator(A)
    assert op.layout()["slices"] == WB.sell_geometry(n, k)["nslices"] and WB.sell_geometry(n, k)["capped"]
    X = np.random.default_rng(n).standard_normal((n, k)).astype(dtype)
    _assert_bitwise(op @ X, A @ X)


@pytest.fixture(scope="module")
def structured():
    return {name: WB.structured(name) for name in WB.STRUCTURED}


@pytest.mark.parametrize("k", WB.STRUCTURED_WIDTHS)
@pytest.mark.parametrize("name", WB.STRUCTURED)
def test_spmv_wide_structured(structured, name, k):
    """A 15-point and a 5-point stencil (diagonal-offset images, whose block
    kernel stops at k = 8) on the lane-group kernel (16 to 64) and on the
    column-group kernel (128, 256)."""
    import krylov_amd

    A = structured[name]
    op = krylov_amd.CsrOperator(A)
    assert op.layout()["dia"]
    X = np.random.default_rng(k).standard_normal((A.shape[0], k))
    _assert_bitwise(op @ X, A @ X)


@pytest.mark.parametrize("k", WB.ODD_WIDTHS)
def test_spmv_wide_odd_widths(golden, structured, k):
    """33 and 129 columns run as 64 and 256: the result has the caller's
    columns only, each bitwise."""
    import krylov_amd

    for A in (_golden_csr(golden["spmv"], "f64_i32"), structured["poisson2d_61"], WB.banded(64 * 36 + 5, 7)):
        X = WB.wide_x(A.shape[0], k, np.float64, k)
        got = krylov_amd.CsrOperator(A) @ X
        assert got.shape == (A.shape[0], k)
        _assert_bitwise(got, A @ X)


# ---------------------------------------------------------------- solvers
def _gmres_path(A, B, kw):
    """(persistent, fallbacks) of a GMRES state on this problem after four
    steps (the kernel is chosen at the first)."""
    from krylov_amd import _helpers
    from krylov_amd.gmres import _GmresState, _sweeps

    prob = _helpers.Problem(A, B, None, kw.get("inner"), M=kw.get("M"), Ml=kw.get("Ml"), Mr=kw.get("Mr"))
    st = _GmresState(prob, kw["maxiter"], _sweeps(kw.get("ortho", "mgs"), kw.get("inner"), kw.get("M"), B))
    st.start()
    st.set_criterion(np.zeros(prob.kpad))
    hist, _ = st.run(4)
    assert len(hist) == 4
    return st.path()


def _compare_with_oracle(cid, got, ref):
    """The rule of wide_block_cases on a device run; prints and returns the
    largest strict-class deviation as a fraction of the tolerance."""
    want = WB.history(ref)
    WB.assert_cap(want)
    assert got.numsteps == ref.numsteps, (got.numsteps, ref.numsteps)
    assert got.success == ref.success
    worst = WB.history_deviation(WB.history(got), want)
    print(f"{cid}: steps {got.numsteps}, largest history deviation {worst:.3e} of the tolerance")
    WB.assert_final_and_x(got, ref)
    return worst


@pytest.mark.parametrize("cid", [c[0] for c in WB.CASES])
def test_wide_block_solve_matches_oracle(cid, monkeypatch):
    import krylov_amd
    from oracle import krylov_ref

    c = WB.case(cid)
    solver, A, B, kw = WB.build(c, krylov_amd.WeightedInner)
    _, _, _, ref_kw = WB.build(c, WB.host_inner)
    _, ref = getattr(krylov_ref, solver)(A, B, **ref_kw)
    WB.assert_cap(WB.history(ref))
    assert B.shape[1] == c[3]
    if solver == "gmres":
        # without preconditioner and weights the MGS passes of a step run as
        # one persistent launch; the streamed kernel is the one left when the
        # register-resident ones are the only candidates and none fits
        persistent = cid in WB.PERSISTENT
        assert _gmres_path(A, B, kw) == (persistent, 0)
        if persistent:
            monkeypatch.setenv("KRY_MGS_PERSIST", "1")
            assert _gmres_path(A, B, kw) == (cid not in WB.STREAMED, 0)
            monkeypatch.delenv("KRY_MGS_PERSIST")
    _, got = getattr(krylov_amd, solver)(A, B, **kw)
    assert np.asarray(got.xk).shape == B.shape and WB.history(got).shape[1] == c[3]
    _compare_with_oracle(cid, got, ref)
    if cid in WB.PERSISTENT:
        monkeypatch.setenv("KRY_MGS_PERSIST", "0")
        assert _gmres_path(A, B, kw) == (False, 0)
        _, lpp = getattr(krylov_amd, solver)(A, B, **kw)
        assert lpp.numsteps == got.numsteps
        g, l = WB.history(got), WB.history(lpp)
        # (the floor class, rounding noise on both paths, is held to its size)
        strict, _ = WB.classes(WB.history(ref))
        np.testing.assert_allclose(g[:-1][strict], l[:-1][strict], rtol=1e-12)
        WB.history_deviation(l, WB.history(ref))
        scale = np.abs(lpp.xk).max(axis=0)
        assert np.all(np.abs(got.xk - lpp.xk) <= 1e-11 * scale), float(
            np.max(np.abs(got.xk - lpp.xk) / np.maximum(scale, 1e-300)))
        print(f"{cid}: persistent vs launch per pass, history "
              f"{np.max(np.abs(g[:-1][strict] - l[:-1][strict]) / l[:-1][strict]):.3e}")


@pytest.mark.parametrize("cid,spec", WB.FACTORED_CASES, ids=[c[0] for c in WB.FACTORED_CASES])
def test_wide_block_factored_preconditioners(cid, spec):
    """CG with SSOR and ILU(0) at 64 columns, the most a factorised
    preconditioner takes; the oracle applies the device object's own factors
    through SciPy triangular solves."""
    import krylov_amd
    from oracle import krylov_ref

    A, _ = WB.matrix("poisson12")
    n = A.shape[0]
    B = WB.block("poisson12", 64)
    P = PC.device_precond(krylov_amd, A, spec, np.float64)
    f = P.factors()
    stages = [("tri", f[0], True)] + ([("scale", f[2])] if spec[0] == "ssor" else []) + [("tri", f[1], False)]
    _, ref = krylov_ref.cg(A, B, M=PC.HostPrecond(n, np.float64, stages), tol=1e-8)
    _, got = krylov_amd.cg(A, B, M=P, tol=1e-8)
    _compare_with_oracle(cid, got, ref)


def test_wide_block_every_column_invariant_at_once():
    """A = diag(1..40) and 32 columns, each a multiple of another unit
    vector: every column's Krylov space is invariant at step 1. GMRES ends as
    the oracle does: the same exception, or the same step count, success and
    history."""
    import krylov_amd
    from oracle import krylov_ref

    A, _ = WB.matrix("diag40")
    B = WB.unit_block()

    def outcome(fn, invariant_error):
        try:
            return fn(A, B, tol=1e-12)[1]
        except invariant_error as e:
            return type(e)

    ref = outcome(krylov_ref.gmres, krylov_ref.InvariantError)
    got = outcome(krylov_amd.gmres, krylov_amd.ArgumentError)
    if ref is krylov_ref.InvariantError:
        assert got is krylov_amd.ArgumentError
        return
    assert got is not krylov_amd.ArgumentError
    assert (got.numsteps, got.success) == (ref.numsteps, ref.success) == (1, True)
    g, w = WB.history(got), WB.history(ref)
    assert g.shape == w.shape == (2, 32)
    assert np.all(np.abs(g[0] - w[0]) <= WB.RTOL * w[0])
    assert np.all(np.abs(g[-1] - w[-1]) <= 1e-12 * w[0])
    np.testing.assert_allclose(got.xk, ref.xk, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m", [64, 65])
def test_wide_multi_solve_triangular(m, dtype):
    """256 systems on either side of the m = 64 switch between gm_trsv_kernel
    (one wave per column) and gm_trsv_big_kernel, against
    scipy.linalg.solve_triangular per column."""
    import krylov_amd

    k = 256
    rng = np.random.default_rng(m * 10 + k)
    R = np.triu(rng.standard_normal((m, m, k)).transpose(2, 0, 1)).transpose(1, 2, 0).astype(dtype)
    dg = np.arange(m)
    for c in range(k):
        R[dg, dg, c] += np.sign(R[dg, dg, c]) * 3.0
    y = rng.standard_normal((m, k)).astype(dtype)
    y[:, 1] = 0.0
    got = krylov_amd.multi_solve_triangular(R, y)
    ref = np.array([np.zeros(m) if np.all(y[:, c] == 0) else scipy.linalg.solve_triangular(R[:, :, c], y[:, c])
                    for c in range(k)]).T
    assert got.shape == ref.shape and got.dtype == ref.dtype
    tol = 1e-12 if dtype == np.float64 else 1e-4  # test_multi_solve_triangular's
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())
    assert np.all(got[:, 1] == 0.0)
