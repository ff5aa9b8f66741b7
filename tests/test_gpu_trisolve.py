"""The device sparse triangular solve (krylov_amd.TriangularOperator over
kry_tri, csrc/tri.hip): exact integer systems solved bitwise, the textbook
componentwise backward-error bound of substitution, determinism, and the
chain form against the plain one."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import tri_cases as TC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", TC.NAMES)
def test_exact_systems_are_solved_bitwise(name):
    """Small integer off-diagonals, a diagonal in {+-1, +-2, +-4}, integer x
    and y = T x formed exactly: every intermediate is an exact integer, so any
    wrong entry, order or dependency shows as a wrong bit."""
    from krylov_amd import TriangularOperator

    A = TC.pattern(name)
    for lower in (True, False):
        for dtype in (np.float32, np.float64):
            T, _, _ = TC.exact_system(A, lower, dtype, 1)
            op = TriangularOperator(T, lower=lower)
            lay = op.layout()
            want = TC.plan_py(TC.triangle(A, lower), lower)
            assert (lay["levels"], lay["launches"], lay["slices"], lay["slots"]) == (
                want["levels"], want["launches"], want["slices"], want["slots"])
            for k in (1, 3, 8):
                T2, x, y = TC.exact_system(A, lower, dtype, k)
                assert (T2 != T).nnz == 0
                got = op.solve(y)
                assert got.dtype == dtype and got.shape == x.shape
                np.testing.assert_array_equal(got, x, err_msg=f"{name} lower={lower} {np.dtype(dtype)} k={k}")


def _backward_matrices():
    from krylov_amd import problems

    return {"poisson40": lambda: problems.poisson2d(40), "stencil15_24": lambda: problems.stencil15_3d(24),
            "rand5000": lambda: problems.random_nonsym(5000),
            "perm_poisson300": lambda: problems.permuted_sym(problems.poisson2d(300), 2)}


@pytest.mark.parametrize("name", ["poisson40", "stencil15_24", "rand5000", "perm_poisson300"])
def test_componentwise_backward_error(name):
    """|T x - y| <= gamma_m (|T| |x| + |y|) componentwise, gamma_m = m u /
    (1 - m u), m = longest row + 1, u the unit round-off of the vectors'
    dtype: the bound of substitution (Higham, Accuracy and Stability, Thm 8.5
    with the right-hand side's rounding), the residual evaluated in extended
    precision on the host."""
    from krylov_amd import TriangularOperator

    A = sp.csr_matrix(_backward_matrices()[name]())
    n = A.shape[0]
    rng = np.random.default_rng(11)
    for lower in (True, False):
        for dtype in (np.float64, np.float32):
            T = TC.triangle(A, lower).astype(dtype)
            y = rng.standard_normal((n, 3)).astype(dtype)
            x = TriangularOperator(T, lower=lower).solve(y)
            assert x.dtype == dtype and np.all(np.isfinite(x))
            coo = T.tocoo()
            tv = coo.data.astype(np.longdouble)
            res = -y.astype(np.longdouble)
            mag = np.abs(y).astype(np.longdouble)
            xl = x.astype(np.longdouble)
            for c in range(3):
                np.add.at(res[:, c], coo.row, tv * xl[coo.col, c])
                np.add.at(mag[:, c], coo.row, np.abs(tv) * np.abs(xl[coo.col, c]))
            m = int(np.diff(T.indptr).max()) + 1
            u = np.longdouble(np.finfo(dtype).eps) / 2
            gamma = m * u / (1 - m * u)
            ratio = float(np.max(np.abs(res) / (gamma * mag)))
            print(f"{name} lower={lower} {np.dtype(dtype)}: worst |res| / bound = {ratio:.3f}")
            assert ratio <= 1.0


@pytest.mark.parametrize("name", ["rand5000", "arrow3000", "poisson40"])
def test_solves_are_deterministic_and_independent_of_k(name):
    from krylov_amd import TriangularOperator

    A = TC.pattern(name)
    rng = np.random.default_rng(5)
    for lower in (True, False):
        T = TC.triangle(A, lower)
        T = T + sp.diags(np.full(T.shape[0], 3.0))  # values that round
        op = TriangularOperator(T, lower=lower)
        Y = rng.standard_normal((T.shape[0], 8))
        X1, X2 = op.solve(Y), op.solve(Y)
        np.testing.assert_array_equal(X1, X2)
        for c in (0, 5, 7):
            np.testing.assert_array_equal(op.solve(Y[:, c]), X1[:, c])
        np.testing.assert_array_equal(op.solve(Y[:, :3]), X1[:, :3])


def test_chain_form_matches_solve_and_respects_a_stopped_chunk():
    """kry_prog_trisolve is bitwise kry_tri_solve, and does nothing in a chunk
    step after the chunk was stopped, like every chain launch."""
    from krylov_amd import TriangularOperator, _helpers, extra, problems

    A = problems.poisson2d(40)
    n = A.shape[0]
    Y = np.random.default_rng(8).standard_normal((n, 4))
    prob = _helpers.Problem(A, Y, None, None)
    assert not prob.A.renumbered
    D = extra._Dev(prob)
    C = extra._Chain(D, ["n"], cap=4)
    for lower in (True, False):
        op = TriangularOperator(TC.triangle(A, lower), lower=lower, ctx=prob.ctx)
        want = op.solve(Y)
        yv, xv = D.upload(Y), D.zeros()
        C.begin()
        C.trisolve(op, yv, xv, 0)
        C.end(1)
        np.testing.assert_array_equal(xv.to_host(), want)
        # in place, through solve_device
        op.solve_device(yv, yv)
        np.testing.assert_array_equal(yv.to_host(), want)
        # a stopped chunk: the launches of step 1 leave x alone
        zv = D.zeros()
        C.set(None, np.full(4, 1.0))
        C.begin()
        C.sc(extra.SOP_SET, "n", 0, value=0.0)
        C.check("n", 0)
        C.trisolve(op, D.upload(Y), zv, 1)
        rows, _ = C.end(2)
        assert len(rows) == 1
        np.testing.assert_array_equal(zv.to_host(), np.zeros((n, 4)))
    # kry_prog_permute on an operator in the caller's numbering is a copy, and a chain step like the others
    src, a, b2 = D.upload(Y), D.zeros(), D.zeros()
    C.begin()
    C.permute(prob.A, src, a, False, 0)
    C.sc(extra.SOP_SET, "n", 0, value=0.0)
    C.check("n", 0)
    C.permute(prob.A, src, b2, True, 1)
    C.end(2)
    np.testing.assert_array_equal(a.to_host(), Y)
    np.testing.assert_array_equal(b2.to_host(), np.zeros((n, 4)))


def test_singular_and_malformed_triangles_are_refused():
    from krylov_amd import TriangularOperator, problems

    A = problems.poisson2d(8)
    with pytest.raises(ValueError):
        TriangularOperator(A, lower=True)
    L = sp.tril(A).tolil()
    L[7, 7] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        TriangularOperator(L.tocsr(), lower=True)
    op = TriangularOperator(sp.tril(A), lower=True)
    with pytest.raises(NotImplementedError):
        op.solve(np.ones((A.shape[0], 65)))
    with pytest.raises(ValueError):
        op.solve(np.ones(A.shape[0] + 1))
