"""The device ILU(0) factorisation (kry_ilu0_factor, csrc/precond.hip) is
bitwise the sequential loop in the same dtype (tests/precond_factored_cases.py
ilu0_loop: dtype scalars, the product rounded before the subtraction),
whatever launch plan the matrix takes: many thin levels in one workgroup, fat
levels grouped under 1024 rows, a level over 1024 rows on its own grid, and a
300-entry row through the strided loop."""
import numpy as np
import pytest
import scipy.sparse

from krylov_amd import problems
from tests import precond_factored_cases as PC

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_factors(P, A, dtype):
    want = PC.ilu0_loop(A, dtype)
    assert P.lu.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(P.lu.indptr, want.indptr)
    np.testing.assert_array_equal(P.lu.indices, want.indices)
    np.testing.assert_array_equal(_bits(P.lu.data), _bits(want.data))
    L, U = P.factors()
    Lw, Uw = PC.split_lu(want)
    for got, ref in ((L, Lw), (U, Uw)):
        assert got.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(got.indptr, ref.indptr)
        np.testing.assert_array_equal(got.indices, ref.indices)
        np.testing.assert_array_equal(_bits(got.data), _bits(ref.data))
    np.testing.assert_array_equal(L.diagonal(), np.ones(A.shape[0], dtype=dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_poisson_thin_levels(dtype):
    import krylov_amd

    A = problems.poisson2d(12)
    P = krylov_amd.Ilu0Preconditioner(A, dtype=dtype)
    lay = P.layout()["factor"]
    assert lay["levels"] == 23 and lay["launches"] == 1  # anti-diagonals of the grid, one workgroup
    _assert_factors(P, A, dtype)


def test_random_fat_levels_grouped():
    import krylov_amd

    A = problems.random_nonsym(3000, 6, 2.0)
    P = krylov_amd.Ilu0Preconditioner(A)
    lay = P.layout()["factor"]
    assert lay["max_level"] <= 1024 and lay["levels"] > 1
    _assert_factors(P, A, np.float64)


def test_random_level_on_its_own_grid():
    import krylov_amd

    A = problems.random_nonsym(20000, 4, 2.0)
    P = krylov_amd.Ilu0Preconditioner(A)
    assert P.layout()["factor"]["max_level"] > 1024  # the multi-workgroup launch runs
    _assert_factors(P, A, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_arrow_long_row(dtype):
    import krylov_amd

    A = PC.arrow(300)
    assert A.indptr[-1] - A.indptr[-2] == 300
    d = np.abs(A.diagonal())
    assert np.all(np.asarray(abs(A).sum(axis=1)).ravel() - d < d)  # diagonally dominant
    P = krylov_amd.Ilu0Preconditioner(A, dtype=dtype)
    _assert_factors(P, A, dtype)


def test_one_by_one():
    import krylov_amd

    A = scipy.sparse.csr_matrix(np.array([[3.0]]))
    P = krylov_amd.Ilu0Preconditioner(A)
    _assert_factors(P, A, np.float64)
    np.testing.assert_array_equal(P @ np.array([6.0]), [2.0])


def test_diagonal_matrix():
    import krylov_amd

    d = np.linspace(1.0, 3.0, 130)
    A = scipy.sparse.diags(d, format="csr")
    P = krylov_amd.Ilu0Preconditioner(A)
    _assert_factors(P, A, np.float64)
    y = np.arange(1.0, 131.0)
    np.testing.assert_array_equal(P @ y, y / d)


def test_zero_pivot_names_the_row():
    import krylov_amd

    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        krylov_amd.Ilu0Preconditioner(np.array([[1.0, 1.0], [1.0, 1.0]]))


def test_repeatable():
    import krylov_amd

    A = problems.random_nonsym(3000, 6, 2.0)
    a = krylov_amd.Ilu0Preconditioner(A).lu.data
    b = krylov_amd.Ilu0Preconditioner(A).lu.data
    np.testing.assert_array_equal(_bits(a), _bits(b))
