"""Host-only checks of tests/wide_block_cases.py: the conditions that keep the
device tests of tests/test_gpu_wide_blocks.py from passing vacuously. No
kernel is launched here; the solver cases run on the oracle."""
import numpy as np
import pytest

from oracle import krylov_ref as K
from tests import wide_block_cases as WB


@pytest.fixture(scope="module")
def oracle_runs():
    """Every solver case's oracle run, made once."""
    out = {}
    for c in WB.CASES:
        solver, A, B, kw = WB.build(c, WB.host_inner)
        out[c[0]] = getattr(K, solver)(A, B, **kw)[1]
    return out


# ------------------------------------------------------------------- SpMV
def test_banded_shapes_reach_the_rounding_and_empty_ranges():
    """Among the banded shapes at k = 128 and 256: a grid that the
    multiple-of-8 rule changes, at one slice and at an odd slice count above
    one; fewer slices than waves per column group (empty ranges); ranges of
    one and of two slices side by side; and none at the cap."""
    geo = {(n, k): WB.sell_geometry(n, k) for n in WB.BANDED_ROWS for k in WB.WIDE}
    assert sorted({g["nslices"] for g in geo.values()}) == [1, 2, 37, 38]
    assert {g["nch"] for g in geo.values()} == {16, 32}
    assert not any(g["capped"] for g in geo.values())
    rounded = [key for key, g in geo.items() if g["rounded"]]
    assert (1, 128) in rounded and (64 * 36 + 5, 128) in rounded
    for key in rounded:
        assert geo[key]["empty"] > 0  # the added blocks' waves own no slice
    assert geo[(1, 128)]["per_group"] == 2 and geo[(1, 128)]["empty"] == 1
    assert geo[(1, 256)]["per_group"] == 1 and geo[(1, 256)]["empty"] == 0
    assert geo[(64 * 36 + 5, 128)]["per_group"] == 38 and geo[(64 * 36 + 5, 128)]["empty"] == 1
    assert all(g["widest"] == 1 for g in geo.values())  # below the cap a wave owns one slice at most


def test_grid_cap_shapes_are_the_first_past_the_cap():
    for n, k, dtype in WB.GRID_CAP_SHAPES:
        g = WB.sell_geometry(n, k)
        assert g["capped"] and g["grid"] == WB.MAX_GRID and not g["rounded"]
        assert g["nslices"] * g["nch"] > 4 * WB.MAX_GRID
        assert g["empty"] == 0 and g["widest"] == 2  # some waves walk two slices
        assert n % 64 != 0  # a partial last slice
        assert n * k * np.dtype(dtype).itemsize <= 150e6
    assert {k for _, k, _ in WB.GRID_CAP_SHAPES} == set(WB.WIDE)
    # the largest uncapped banded shape is far below: nothing between is needed
    # to see the cap's arithmetic, which only changes `widest`
    assert not WB.sell_geometry(64 * 37 + 5, 256)["capped"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_banded_matrix_has_its_named_slices(dtype):
    A = WB.banded(64 * 37 + 5, 7, dtype)
    assert A.dtype == dtype and A.has_sorted_indices and A.indices.dtype == np.int32
    lens = np.diff(A.indptr)
    assert np.all(lens[64:128] == 0)
    # slice 2 keeps every offset that stays inside the matrix (the 16 draws of
    # banded(), repeated here)
    offs = np.sort(np.random.default_rng(7).choice(np.arange(-400, 401), 16, replace=False))
    inside = (np.arange(128, 192)[:, None] + offs[None, :] >= 0).sum(axis=1)
    np.testing.assert_array_equal(lens[128:192], inside)
    assert inside.min() >= 8
    assert lens.min() == 0 and lens.max() == 16 and 0 < np.count_nonzero(lens[192:]) < lens.shape[0] - 192
    rows = np.repeat(np.arange(A.shape[0]), lens)
    assert np.all(np.abs(A.indices - rows) <= 400)
    for i in range(A.shape[0]):  # distinct within the row
        r = A.indices[A.indptr[i]:A.indptr[i + 1]]
        assert np.all(np.diff(r) > 0)
    assert WB.banded(1, 7, dtype).shape == (1, 1)


@pytest.mark.parametrize("dtype,e", [(np.float64, 20), (np.float32, 8)])
def test_wide_x_spans_its_magnitudes(dtype, e):
    X = WB.wide_x(2000, 128, dtype, 5)
    assert X.dtype == dtype and X.shape == (2000, 128) and np.all(np.isfinite(X))
    mag = np.log10(np.abs(X[X != 0]))
    assert mag.max() > e - 1 and mag.min() < 1 - e


# ---------------------------------------------------------------- the block
def test_blocks_are_rebuilt_identically_from_the_seed():
    for name, k in (("poisson29", 129), ("R", 32), ("poisson29_shift_w", 128)):
        B1 = WB.block(name, k)
        WB.matrix.cache_clear()
        B2 = WB.block(name, k)
        assert B1 is not B2
        np.testing.assert_array_equal(B1.view(np.uint8), B2.view(np.uint8))
        assert not np.array_equal(B1[:, 4:], WB.block(name, k, seed=1)[:, 4:])
    np.testing.assert_array_equal(WB.unit_block(), WB.unit_block())
    np.testing.assert_array_equal(WB.wide_x(65, 128, np.float32, 3), WB.wide_x(65, 128, np.float32, 3))
    a, b = WB.banded(65, 9), WB.banded(65, 9)
    np.testing.assert_array_equal(a.indices, b.indices)
    np.testing.assert_array_equal(a.data, b.data)


@pytest.mark.parametrize("name", ["poisson29", "poisson100", "poisson29_shift_w", "Pvar", "R"])
def test_column_0_is_an_eigenvector(name):
    A, v = WB.matrix(name)
    lam = (v @ (A @ v)) / (v @ v)
    res = np.linalg.norm(A @ v - lam * v) / (np.abs(lam) * np.linalg.norm(v))
    print(name, "eigenvalue", lam, "relative residual", res)
    assert res < 1e-12
    B = WB.block(name, 32)
    np.testing.assert_array_equal(B[:, 0], v)
    assert np.all(B[:, 1] == 0.0)
    n = A.shape[0]
    assert 0.5e-12 < np.linalg.norm(B[:, 2]) / np.sqrt(n) < 2e-12
    assert 0.5e12 < np.linalg.norm(B[:, 3]) / np.sqrt(n) < 2e12
    assert 0.5 < np.linalg.norm(B[:, 4:]) / np.sqrt(n * 28) < 2.0


def test_case_list_is_the_one_the_device_tests_expect():
    ids = [c[0] for c in WB.CASES]
    assert len(ids) == len(set(ids)) == 26
    for s in ("cg", "minres"):
        assert sorted(c[3] for c in WB.CASES if c[1] == s and c[2] == "poisson29") == [32, 33, 64, 128, 129, 256]
    assert set(WB.PERSISTENT) == {f"gmres_{o}_R_k{k}" for o in ("mgs", "mgs2") for k in (32, 128, 256)} | {
        "gmres_poisson100_k256", "gmres_poisson29_k32_m70"}
    assert set(WB.STREAMED) < set(WB.PERSISTENT)
    A, _ = WB.matrix("poisson29")
    assert A.shape[0] == 841 and A.shape[0] % 64 != 0
    # n k of the streamed case is past 512 threads x 16 doubles x 256 blocks
    A100, _ = WB.matrix("poisson100")
    assert A100.shape[0] * 256 > 512 * 16 * 256
    # the QR kernel's LDS tile holds 2048 / k rotations: 30 steps cross it from k = 128 on
    assert 2048 // 128 < 30 and 2048 // 256 < 30 and 2048 // 32 >= 30 and 2048 // 32 < 70
    A, _ = WB.matrix("poisson29_shift_w")
    w = WB.weights(841)
    S = (A.T.multiply(w)).T.tocsr()  # W A: symmetric, so A is self-adjoint in <., .>_w
    assert abs(S - S.T).max() < 1e-15


# ------------------------------------------------------------------ the rule
@pytest.mark.parametrize("cid", [c[0] for c in WB.CASES])
def test_cap_on_the_floor_class(oracle_runs, cid):
    """On the oracle's history of every case: at least 90 % of the ordinary
    columns' entries are compared relatively, column 0 starts there, and the
    zero column is zero."""
    ref = oracle_runs[cid]
    want = WB.history(ref)
    c = WB.case(cid)
    assert want.shape == (ref.numsteps + 1, c[3])
    share = WB.assert_cap(want)
    strict, floor = WB.classes(want)
    print(cid, "steps", ref.numsteps, "success", ref.success, "strict share", share,
          "column 0 strict entries", int(strict[:, 0].sum()))
    if c[2] in ("poisson29", "poisson100", "poisson29_shift_w", "R") and not set(c[4]) & {"M", "Ml", "Mr"}:
        # the eigenvector column is done at step 1 and stays in the floor class
        assert int(strict[:, 0].sum()) == 1 and np.all(want[1:-1, 0] < 1e-12 * want[0, 0])
    if "maxiter" in c[4]:
        assert ref.numsteps == c[4]["maxiter"] and not ref.success
    else:
        assert ref.success and ref.numsteps < A_rows(c)
    np.testing.assert_array_equal(np.asarray(ref.xk)[:, 1], 0.0)


@pytest.mark.parametrize("cid,spec", WB.FACTORED_CASES, ids=[c[0] for c in WB.FACTORED_CASES])
def test_cap_on_the_floor_class_factored(cid, spec):
    """The same for CG at 64 columns under SSOR and ILU(0), with the host
    models of the factors (the device test takes the device object's own)."""
    from tests import precond_factored_cases as PC

    A, _ = WB.matrix("poisson12")
    B = WB.block("poisson12", 64)
    assert B.shape == (144, 64)
    _, ref = K.cg(A, B, M=PC.host_precond(A, spec, np.float64), tol=1e-8)
    share = WB.assert_cap(WB.history(ref))
    print(cid, "steps", ref.numsteps, "strict share", share)
    assert ref.success


def A_rows(c):
    return WB.matrix(c[2])[0].shape[0]


def test_rule_rejects_what_it_should():
    """history_deviation on a made-up history: passes on itself, fails on a
    relative error of 2e-10 in one strict entry, on a floor entry that is too
    large, and on a nonzero in the zero column."""
    steps, k = 12, 8
    want = np.outer(10.0 ** (-1.1 * np.arange(steps + 1)), np.ones(k))  # 10^-7.7 strict, 10^-8.8 floor
    want[:, 1] = 0.0
    want[1:, 0] = 1e-15
    want[:, 3] *= 1e12
    assert WB.history_deviation(want.copy(), want) == 0.0
    strict, floor = WB.classes(want)
    assert strict[:8, 2:].all() and floor[8:, 2:].all() and floor[1:, 0].all() and strict[0, 0]
    bad = want.copy()
    bad[5, 3] *= 1 + 2e-10
    with pytest.raises(AssertionError):
        WB.history_deviation(bad, want)
    ok = want.copy()
    ok[5, 3] *= 1 + 0.5e-10
    assert 0.49 < WB.history_deviation(ok, want) < 0.51
    bad = want.copy()
    bad[10, 4] = 3e-8
    with pytest.raises(AssertionError):
        WB.history_deviation(bad, want)
    ok = want.copy()
    ok[10, 4] = 1.9e-8
    WB.history_deviation(ok, want)
    for v in (1e-300, np.nan):
        bad = want.copy()
        bad[4, 1] = v
        with pytest.raises(AssertionError):
            WB.history_deviation(bad, want)
    bad = want.copy()
    bad[3, 0] = np.inf
    with pytest.raises(AssertionError):
        WB.history_deviation(bad, want)
    assert WB.assert_cap(want[:9]) == 1.0
    with pytest.raises(AssertionError):
        WB.assert_cap(want[:10])  # 8 of 9 compared entries in the strict class


def test_oracle_noise_behind_the_tolerance(oracle_runs):
    """The oracle's block run against its own single-column runs of four
    ordinary columns, for the k = 128 cases: only the summation grouping
    differs (einsum over the block against np.dot). The largest relative
    difference over the strict class is printed and must stay below 1e-11,
    a tenth of the tolerance the device is held to."""
    worst_all = 0.0
    for c in WB.CASES:
        if c[3] != 128:
            continue
        solver, A, B, kw = WB.build(c, WB.host_inner)
        want = WB.history(oracle_runs[c[0]])
        strict, _ = WB.classes(want)
        worst = 0.0
        for col in (4, 5, 77, 127):
            try:
                _, one = getattr(K, solver)(A, B[:, col], **kw)
            except K.InvariantError:
                continue
            h = WB.history(one)
            m = min(h.shape[0], want.shape[0]) - 1  # a single column may stop at another step
            s = strict[:m, col]
            worst = max(worst, float(np.max(np.abs(h[:m][s] - want[:m, col][s]) / want[:m, col][s])))
        print(f"{c[0]}: block vs single-column history, max relative difference {worst:.3e}")
        assert worst > 0.0
        worst_all = max(worst_all, worst)
    print(f"oracle noise, largest over the k = 128 cases: {worst_all:.3e}")
    assert worst_all < WB.NOISE_BOUND
    assert WB.NOISE_BOUND * 10 <= WB.RTOL
