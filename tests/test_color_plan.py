"""The host side of the multicolour ordering: kry_color_plan against a Python
model of the greedy first-fit rule, the colouring's validity, and the ordered
triangular plan (kry_tri_plan_ordered) against kry_tri_plan on the explicitly
permuted triangle. No kernel is launched here."""
import numpy as np
import pytest
import scipy.sparse as sp

from krylov_amd import problems
from tests import multicolor_cases as MC
from tests import tri_cases as TC

NAMES = list(MC.COLOR_SIZES)


@pytest.fixture(scope="module")
def models():
    """name -> (A, colors, perm) of the Python model, computed once."""
    out = {}
    for name in NAMES:
        A = MC.matrix(problems, name)
        out[name] = (A,) + MC.color_py(A)
    return out


@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("name", NAMES)
def test_color_plan_equals_the_model(models, name, itype):
    from krylov_amd import _lib

    A, colors, perm = models[name]
    got = _lib.color_plan(A.indptr.astype(itype), A.indices.astype(itype))
    np.testing.assert_array_equal(got["color"], colors)
    np.testing.assert_array_equal(got["perm"], perm)
    sizes = np.bincount(colors).tolist()
    assert sizes == MC.COLOR_SIZES[name]
    assert got["colors"] == len(sizes) and got["max_color"] == max(sizes)


@pytest.mark.parametrize("name", NAMES)
def test_no_entry_joins_two_rows_of_one_colour(name):
    import krylov_amd

    A = MC.matrix(problems, name)
    colors, perm = krylov_amd.multicolor_ordering(A)
    assert colors.dtype == np.int32 and perm.dtype == np.int32
    C = A.tocoo()
    off = C.row != C.col
    assert not np.any(colors[C.row[off]] == colors[C.col[off]])
    np.testing.assert_array_equal(np.sort(perm), np.arange(A.shape[0]))
    key = colors[perm].astype(np.int64) * A.shape[0] + perm  # sorted by (colour, row)
    assert np.all(np.diff(key) > 0)


def test_special_patterns():
    """Rows with only a diagonal entry get colour 0; explicit zeros are
    edges; a nonsymmetric pattern is symmetrised; n = 0 and n = 1."""
    import krylov_amd
    from krylov_amd import _lib

    # rows 1 and 3 hold nothing but their diagonal
    A = sp.csr_matrix(np.array([[2.0, 0, 1, 0, 0], [0, 2, 0, 0, 0], [1, 0, 2, 0, 1], [0, 0, 0, 2, 0], [0, 0, 1, 0, 2]]))
    colors, perm = krylov_amd.multicolor_ordering(A)
    np.testing.assert_array_equal(colors, [0, 0, 1, 0, 0])
    np.testing.assert_array_equal(perm, [0, 1, 3, 4, 2])
    np.testing.assert_array_equal(colors, MC.color_py(A)[0])
    # (0, 1) stored only above the diagonal, (2, 1) only below, (2, 0) as an explicit zero
    ip = np.array([0, 2, 3, 6], dtype=np.int32)
    ix = np.array([0, 1, 1, 0, 1, 2], dtype=np.int32)
    got = _lib.color_plan(ip, ix)
    np.testing.assert_array_equal(got["color"], [0, 1, 2])
    Z = sp.csr_matrix((np.array([1.0, 1, 1, 0, 1, 1]), ix, ip), shape=(3, 3))
    np.testing.assert_array_equal(MC.color_py(Z)[0], [0, 1, 2])
    np.testing.assert_array_equal(krylov_amd.multicolor_ordering(Z)[0], [0, 1, 2])
    empty = _lib.color_plan(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert empty["colors"] == 0 and empty["max_color"] == 0 and empty["perm"].shape == (0,)
    one = _lib.color_plan(np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int64))
    assert one["colors"] == 1 and one["max_color"] == 1
    with pytest.raises(ValueError):  # a column index out of range
        _lib.color_plan(np.array([0, 1], dtype=np.int32), np.array([3], dtype=np.int32))
    with pytest.raises(ValueError, match="square"):
        krylov_amd.multicolor_ordering(np.ones((2, 3)))
    with pytest.raises(TypeError, match="CsrOperator does not keep"):
        krylov_amd.multicolor_ordering(object.__new__(krylov_amd.CsrOperator))
    assert "multicolor_ordering" in krylov_amd.__all__


@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("name", NAMES)
def test_ordered_plan_is_the_permuted_triangles_plan(models, name, itype):
    """Over the multicolour order the lower triangle's levels are the colours
    (level = colour + 1: first-fit gives every row of colour c a neighbour of
    colour c - 1 before it), and both triangles' plans are kry_tri_plan's on
    the explicitly permuted triangle, mapped through perm."""
    from krylov_amd import _lib

    A, colors, perm = models[name]
    rank = MC.rank_of(perm)
    B = MC.permuted(A, perm)
    for lower in (True, False):
        T = MC.split_by_rank(A, rank, lower)
        got = _lib.tri_plan(T.indptr.astype(itype), T.indices.astype(itype), lower, rank=rank)
        TB = TC.triangle(B, lower)
        want = _lib.tri_plan(TB.indptr.astype(itype), TB.indices.astype(itype), lower)
        for key in ("levels", "launches", "slices", "slots", "max_level"):
            assert got[key] == want[key], key
        np.testing.assert_array_equal(got["level"][perm], want["level"])
        np.testing.assert_array_equal(got["order"], perm[want["order"]])
        np.testing.assert_array_equal(got["launch"], want["launch"])
        np.testing.assert_array_equal(got["widths"], want["widths"])
    # the coloured graph's own lower triangle (A + A^T: a row depends on every neighbour of a lower colour)
    G = (abs(A) + abs(A).T).tocsr()
    G.data[:] = 1.0
    T = MC.split_by_rank(G, rank, True)
    got = _lib.tri_plan(T.indptr.astype(itype), T.indices.astype(itype), True, rank=rank)
    np.testing.assert_array_equal(got["level"], colors + 1)
    assert got["levels"] == len(MC.COLOR_SIZES[name]) and got["max_level"] == max(MC.COLOR_SIZES[name])
    np.testing.assert_array_equal(got["order"], perm)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", ["poisson40", "arrow3000", "level65"])
def test_identity_and_null_rank_equal_tri_plan(name, lower):
    from krylov_amd import _lib

    T = TC.triangle(TC.pattern(name), lower)
    want = _lib.tri_plan(T.indptr, T.indices, lower)
    info = np.zeros(5, dtype=np.int64)
    arrays = [np.zeros(T.shape[0], dtype=np.int32), np.zeros(T.shape[0], dtype=np.int32),
              np.zeros(want["launches"] + 1, dtype=np.int32), np.zeros(want["slices"], dtype=np.int32)]
    _lib.check(_lib.lib.kry_tri_plan_ordered(T.shape[0], T.nnz, _lib.ptr(T.indptr), _lib.ptr(T.indices),
                                             _lib.itype_code(T.indptr.dtype), int(lower), None,
                                             info.ctypes.data_as(_lib._ip64), *[_lib.ptr(a) for a in arrays]))
    ident = _lib.tri_plan(T.indptr, T.indices, lower, rank=np.arange(T.shape[0], dtype=np.int32))
    for key, arr in zip(("level", "order", "launch", "widths"), arrays):
        np.testing.assert_array_equal(arr, want[key], err_msg=key)
        np.testing.assert_array_equal(ident[key], want[key], err_msg=key)
    assert info.tolist() == [want[k] for k in ("levels", "launches", "slices", "slots", "max_level")]


def test_ordered_plan_rejects_wrong_side_entries_and_bad_ranks(models):
    from krylov_amd import _lib

    A, colors, perm = models["poisson12"]
    rank = MC.rank_of(perm)
    L = MC.split_by_rank(A, rank, True)
    _lib.tri_plan(L.indptr, L.indices, True, rank=rank)
    with pytest.raises(ValueError, match="wrong side"):  # lower in the order is not upper in it
        _lib.tri_plan(L.indptr, L.indices, False, rank=rank)
    with pytest.raises(ValueError, match="wrong side"):  # nor lower by index
        _lib.tri_plan(L.indptr, L.indices, True)
    with pytest.raises(ValueError, match="wrong side"):  # the whole matrix
        _lib.tri_plan(A.indptr, A.indices, True, rank=rank)
    bad = rank.copy()
    bad[0] = bad[1]
    with pytest.raises(ValueError, match="permutation"):
        _lib.tri_plan(L.indptr, L.indices, True, rank=bad)
    bad[0] = A.shape[0]
    with pytest.raises(ValueError, match="permutation"):
        _lib.tri_plan(L.indptr, L.indices, True, rank=bad)


def test_argument_checks_need_no_device():
    import krylov_amd
    from krylov_amd.triangular import canonical_triangle, rank_of

    A = MC.matrix(problems, "poisson12")
    colors, perm = krylov_amd.multicolor_ordering(A)
    rank = rank_of(perm, A.shape[0])
    np.testing.assert_array_equal(rank, MC.rank_of(perm))
    L = MC.split_by_rank(A, rank, True)
    assert canonical_triangle(L, True, rank).nnz == L.nnz
    with pytest.raises(ValueError, match="in the given order"):
        canonical_triangle(L, False, rank)
    with pytest.raises(ValueError, match="permutation"):
        rank_of(np.zeros(A.shape[0], dtype=np.int32), A.shape[0])
    with pytest.raises(ValueError, match="permutation"):
        rank_of(perm[:-1], A.shape[0])
    for cls in (krylov_amd.SsorPreconditioner, krylov_amd.Ilu0Preconditioner):
        with pytest.raises(ValueError, match="ordering must be"):
            cls(A, ordering="redblack")
