"""The sequential ISAI loop of tests/isai_cases.py against the properties that
define it (no device): (W T) = I on T's pattern, the transposed form of the
upper factor, and exactness where the inverse has the factor's pattern."""
import numpy as np
import pytest
import scipy.sparse

from krylov_amd import problems
from tests import isai_cases as IC
from tests import precond_factored_cases as PC


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_pattern(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)


def _assert_identity_on_pattern(W, T, lower, dtype):
    """|(W T - I)_ij| <= 4 m eps (|W| |T|)_ij on T's pattern (T W for an
    upper T), m the longest row of the lower form; the products in float64."""
    eps = float(np.finfo(dtype).eps)
    W64, T64 = W.astype(np.float64), T.astype(np.float64)
    prod, mag = (W64 @ T64, abs(W64) @ abs(T64)) if lower else (T64 @ W64, abs(T64) @ abs(W64))
    m = int(np.diff((T if lower else IC.transposed(T)).indptr).max())
    rows = np.repeat(np.arange(T.shape[0]), np.diff(T.indptr))
    cols = T.indices
    resid = np.abs(np.asarray(prod[rows, cols]).ravel() - (rows == cols))
    bound = 4 * m * eps * np.asarray(mag[rows, cols]).ravel()
    assert np.all(resid <= bound), float(np.max(resid / np.maximum(bound, 1e-300)))


@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def loops(request):
    """name -> (T, lower, W) for every triangle of the suite, W by the loop."""
    dtype = request.param
    out = {}
    for name, (L, U) in IC.factor_pairs(problems, dtype).items():
        out[name + "_L"] = (L, True, IC.isai_loop(L, True, dtype))
        out[name + "_U"] = (U, False, IC.isai_loop(U, False, dtype))
    for name, T in IC.hand_triangles(dtype).items():
        out[name] = (T, True, IC.isai_loop(T, True, dtype))
    return dtype, out


def test_w_times_t_is_the_identity_on_the_pattern(loops):
    dtype, cases = loops
    for name, (T, lower, W) in cases.items():
        assert W.dtype == dtype and _same_pattern(W, PC.canonical(T, dtype)), name
        assert np.all(np.isfinite(W.data)), name
        _assert_identity_on_pattern(W, PC.canonical(T, dtype), lower, dtype)


def test_hand_triangles_hold_the_row_lengths():
    T = IC.hand_triangles(np.float64)
    assert {1, 2, 63, 64, 65} <= set(int(m) for m in IC.row_lengths(T["mixed"]))
    assert T["n1"].shape == (1, 1) and T["n65"].shape == (65, 65)
    assert list(IC.row_lengths(T["n65"])) == list(range(1, 66))
    assert np.all(T["unit"].diagonal() == 1.0)
    W1 = IC.isai_loop(T["n1"], True, np.float64)
    assert W1.data[0] == 1.0 / 3.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_upper_of_a_symmetric_ssor_is_the_transposed_lower(dtype):
    lo, up, _ = PC.ssor_factors(problems.poisson2d(12), 1.2, dtype)
    lt = IC.transposed(lo)
    assert _same_pattern(lt, up) and np.array_equal(_bits(lt.data), _bits(up.data))
    WL = IC.isai_loop(lo, True, dtype)
    WU = IC.isai_loop(up, False, dtype)
    WLt = IC.transposed(WL)
    assert _same_pattern(WU, WLt)
    np.testing.assert_array_equal(_bits(WU.data), _bits(WLt.data))


def red_black(nx):
    """(perm, rank) of the two-colour order of poisson2d(nx): what the greedy
    first-fit colouring gives on the 5-point stencil."""
    i = np.arange(nx * nx)
    colors = (i // nx + i % nx) % 2
    perm = np.argsort(colors, kind="stable")
    rank = np.empty_like(perm)
    rank[perm] = np.arange(perm.shape[0])
    return perm, rank


@pytest.mark.parametrize("spec", [("ssor", 1.2), ("ilu0",)], ids=["ssor", "ilu0"])
def test_two_colour_poisson_has_the_exact_inverse(spec):
    """Under the two-colour order a factor is [[D1, 0], [E, D2]]: its inverse
    has its pattern, so W is that inverse (entries of at most m = 5 terms:
    within 4 m eps of it, componentwise)."""
    A = problems.poisson2d(12)
    perm, _ = red_black(12)
    B = PC.canonical(A[perm][:, perm])
    WL, WU, L, U, _ = IC.isai_parts(B, spec, np.float64)
    eps = float(np.finfo(np.float64).eps)
    for W, T in ((WL, L), (WU, U)):
        inv = np.linalg.inv(T.toarray())
        mask = T.toarray() != 0
        assert np.all(np.abs(inv[~mask]) <= 1e-300)  # the inverse has the factor's pattern
        m = int(np.diff(T.indptr).max())
        assert m <= 5
        assert np.all(np.abs(W.toarray() - inv) <= 4 * m * eps * np.abs(inv))


def test_apply_bound_covers_another_summation_order():
    """apply_bound against the same chain evaluated with dense products
    (another summation order): the difference stays within the bound, and the
    bound is small against the result."""
    A = problems.poisson2d(12)
    y = np.random.default_rng(3).standard_normal((144, 3))
    for spec in (("ssor", 1.2), ("ilu0",)):
        parts = IC.isai_parts(A, spec, np.float64)
        for sweeps in (0, 1, 2):
            x, bound = IC.apply_bound(parts, y, sweeps)
            np.testing.assert_array_equal(_bits(x), _bits(IC.apply_model(parts, y, sweeps)))
            dense = tuple(p if i == 4 else scipy.sparse.csr_matrix(p).toarray() for i, p in enumerate(parts))
            xd = IC.stage(dense[1], dense[3], IC.stage(dense[0], dense[2], y, sweeps, dense[4]), sweeps, None)
            assert np.all(np.abs(xd - x) <= bound)
            assert np.max(bound) <= 1e-12 * np.max(np.abs(x))
