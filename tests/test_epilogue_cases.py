"""The exact-integer epilogue cases on the host (tests/epilogue_cases.py):
every configuration meets the magnitude condition that makes the device
comparison of tests/test_gpu_epilogue_images.py exact, the start residual's
squared norm is a power of 4, and the integer reference agrees with SciPy
where SciPy is exact."""
import numpy as np
import pytest

from tests import epilogue_cases as EC


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    EC.clear_caches()


def test_four_squares():
    for r in range(0, 200):
        q = EC.four_squares(r)
        assert sum(v * v for v in q) == r and all(v >= 0 for v in q)


@pytest.mark.parametrize("name", sorted(EC.MATRICES))
def test_matrix_features(name):
    A = EC.matrix(name)
    n = A.shape[0]
    assert A.data.dtype == np.int64 and np.abs(A.data).max() <= 4
    if not name.startswith("dia_uniform"):  # every diagonal constant there: an explicit zero would be a zero diagonal
        assert (A.data == 0).any()
    lens = np.diff(A.indptr)
    assert lens.min() != lens.max()  # rows of differing length
    assert n % 128 != 0  # a partial last slice
    if name != "dia_uniform_12":  # 12^3 = 13.5 slices of 128, taken for its descriptor classes
        assert n % 64 != 0
        assert n % 2 == 1 or name == "sell_irregular"
    if name in ("pair_general", "rs_general", "sell_irregular"):
        assert not A.has_sorted_indices
        rows = np.repeat(np.arange(n), lens)
        key = rows * n + A.indices.astype(np.int64)
        assert np.unique(key).shape[0] < key.shape[0]  # duplicates, kept
    if name in ("pair_general", "cb_scattered", "sell_regular", "dia_narrow_mixed", "dia_wide_plain",
                "dia_uniform_deferred"):
        width = 128 if name != "sell_regular" else 64
        pad = np.concatenate([lens, np.zeros(-n % width, dtype=lens.dtype)])
        empty = pad.reshape(-1, width).sum(axis=1) == 0
        assert empty.any()  # an empty slice
        if name.startswith("dia_"):
            assert not empty[0] and not empty[-1]  # ... in the interior
    if name in ("rs_general", "sell_irregular"):
        assert (lens == 0).any()


@pytest.mark.parametrize("name", sorted(EC.MATRICES))
def test_int_spmv_against_scipy(name):
    """The entry-walking integer SpMV against SciPy's float64 product, which
    is exact here (integers far below 2^53), also for unsorted rows and
    duplicates."""
    A = EC.matrix(name)
    rng = np.random.default_rng(3)
    X = rng.integers(-5, 6, (A.shape[0], 2))
    got = EC.int_spmv(A, X)
    ref = EC.as_float(A, np.float64) @ X.astype(np.float64)
    assert np.abs(ref).max() < 2**53
    np.testing.assert_array_equal(got, ref.astype(np.int64))
    np.testing.assert_array_equal(ref, got.astype(np.float64))
    assert np.all(EC.int_spmv(A, X, absolute=True) >= np.abs(got))


@pytest.mark.parametrize("cfg", EC.CONFIGS, ids=repr)
def test_config_is_exact(cfg):
    A, b, x0, w, ref = cfg.problem()
    n = A.shape[0]
    assert b.shape == x0.shape == ((n,) if cfg.k == 1 else (n, cfg.k))
    assert np.abs(x0).max() <= 3 and w.min() >= 1 and w.max() <= 3
    assert (w.max() > 1) == cfg.weighted
    # <r0, r0>_w is 4^m in every column, so sqrt and r0 / 2^m are exact
    for rho, m in zip(ref.rho0, ref.m):
        assert rho == 4**m and m >= 1
    assert np.abs(ref.r0).max() <= 5
    assert (ref.r0[-3:] != 0).any()  # the tail rows of the last slice carry dot terms
    assert all(p != 0 for p in ref.pAp)  # alpha = rho0 / pAp is a plain quotient, no guard taken
    # the exactness condition, per case, in the type the device works in
    print(f"{cfg.id}: max vector element / row partial {ref.max_vector}, max |dot| {ref.max_dot}, "
          f"sum of |dot terms| {ref.max_dot_abs}, limit 2^{int(np.log2(EC.LIMIT[cfg.vdtype]))}")
    assert ref.exact_in(cfg.vdtype)
    assert np.abs(A.data).max() <= 4 and A.dtype == cfg.mdtype
    # the reference against SciPy where SciPy is exact
    A64 = EC.as_float(EC.matrix(cfg.matrix), np.float64)
    x2 = x0.reshape(n, -1).astype(np.float64)
    np.testing.assert_array_equal(A64 @ x2, ref.Ax0.astype(np.float64))
    np.testing.assert_array_equal(A64 @ ref.r0.astype(np.float64), ref.Ar.astype(np.float64))
    v0 = ref.v0(cfg.vdtype)
    assert v0.dtype == cfg.vdtype
    for c, m in enumerate(ref.m):
        np.testing.assert_array_equal(v0.reshape(n, -1)[:, c].astype(np.float64) * 2.0**m, ref.r0[:, c])


@pytest.mark.parametrize("cfg", [c for c in EC.CONFIGS if c.form is not None], ids=repr)
def test_dia_form(cfg):
    """The host plans give the kernel form the configuration is listed for."""
    A = cfg.problem()[0]
    assert EC.dia_form(A) == cfg.form
    assert EC.dia_waves_walk_two(A) == cfg.expect.get("two_slice_waves", False)


@pytest.mark.parametrize("a,m", EC.PRECOND_PAIRS)
def test_precond_pairs_are_exact(a, m):
    """Ml r0, M Ml r0 and <Ml r0, M Ml r0>_w stay exact in float64."""
    A, M = EC.matrix(a), EC.matrix(m)
    assert A.shape == M.shape
    b, x0, w = EC.rhs(A, 1, True, seed=5)
    ref = EC.Reference(A, b, x0, w)
    mlr = EC.int_spmv(M, ref.r0)
    z = EC.int_spmv(M, mlr)
    amr = EC.int_spmv(A, mlr)  # A Mr r0 of the right-preconditioned GMRES step
    big = max(int(EC.int_spmv(M, ref.r0, absolute=True).max()), int(EC.int_spmv(M, mlr, absolute=True).max()),
              int(EC.int_spmv(A, mlr, absolute=True).max()))
    assert big < 2**53
    assert int((w[:, None] * np.abs(mlr) * np.abs(z)).sum()) < 2**53
    assert int((w[:, None] * mlr * mlr).sum()) < 2**53
    assert int((w[:, None] * np.abs(ref.r0) * np.abs(amr)).sum()) < 2**53
