"""The host-only analysis of the ILU(0) factorisation (kry_ilu0_plan,
csrc/host_image.cpp): its levels are those of the triangular-solve plan on
tril(A)'s pattern, every diagonal position is right, and malformed inputs are
refused. No device needed."""
import numpy as np
import pytest
import scipy.sparse

from krylov_amd import _lib, problems
from tests import precond_factored_cases as PC


def _matrices():
    return {
        "poisson12": problems.poisson2d(12),
        "random3000": problems.random_nonsym(3000, 6, 2.0),
        "arrow300": PC.arrow(300),
    }


@pytest.fixture(scope="module")
def matrices():
    return _matrices()


@pytest.mark.parametrize("name", ["poisson12", "random3000", "arrow300"])
@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_levels_are_the_lower_triangle_plan(matrices, name, itype):
    A = PC.canonical(matrices[name])
    ip, ix = A.indptr.astype(itype), A.indices.astype(itype)
    got = _lib.ilu0_plan(ip, ix)
    T = scipy.sparse.tril(A).tocsr()
    T.sort_indices()
    want = _lib.tri_plan(T.indptr.astype(itype), T.indices.astype(itype), lower=True)
    assert got["levels"] == want["levels"]
    assert got["launches"] == want["launches"]
    assert got["max_level"] == want["max_level"]
    np.testing.assert_array_equal(got["level"], want["level"])
    np.testing.assert_array_equal(got["order"], want["order"])
    np.testing.assert_array_equal(got["launch"], want["launch"])


@pytest.mark.parametrize("name", ["poisson12", "random3000", "arrow300"])
def test_diagonal_positions(matrices, name):
    A = PC.canonical(matrices[name])
    got = _lib.ilu0_plan(A.indptr, A.indices)["diag"]
    n = A.shape[0]
    assert got.shape == (n,)
    assert np.all(got >= A.indptr[:-1]) and np.all(got < A.indptr[1:])
    np.testing.assert_array_equal(A.indices[got], np.arange(n))


def test_small_shapes():
    one = _lib.ilu0_plan(np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32))
    assert one["levels"] == 1 and one["launches"] == 1 and list(one["diag"]) == [0]
    # a diagonal matrix: one level, nothing to eliminate
    n = 70
    d = _lib.ilu0_plan(np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32))
    assert d["levels"] == 1 and d["max_level"] == n
    np.testing.assert_array_equal(d["diag"], np.arange(n))


def test_missing_diagonal_is_singular():
    # row 1 stores (1, 0) only
    ip = np.array([0, 1, 2, 3], dtype=np.int32)
    ix = np.array([0, 0, 2], dtype=np.int32)
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        _lib.ilu0_plan(ip, ix)


def test_unsorted_row_is_refused():
    ip = np.array([0, 1, 3], dtype=np.int32)
    ix = np.array([0, 1, 0], dtype=np.int32)
    with pytest.raises(ValueError, match="sorted"):
        _lib.ilu0_plan(ip, ix)
    # a duplicate column is not canonical either
    with pytest.raises(ValueError, match="sorted"):
        _lib.ilu0_plan(ip, np.array([0, 1, 1], dtype=np.int32))
