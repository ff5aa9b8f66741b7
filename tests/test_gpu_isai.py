"""ISAI triangular solves on the device: the kernel kry_isai_lower against the
sequential loop of tests/isai_cases.py (bitwise), its refusals, the apply of
SsorPreconditioner / Ilu0Preconditioner(solve="isai") against the same products
done by scipy, and the solvers against the reference's results with the host
model of the same preconditioner (tests/golden/precond_isai.npz)."""
import os

import numpy as np
import pytest
import scipy.sparse

from krylov_amd import problems
from tests import gpu_helpers as H
from tests import isai_cases as IC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_same_matrix(got, want, what):
    assert got.dtype == want.dtype, what
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), what
    np.testing.assert_array_equal(_bits(got.data), _bits(want.data), err_msg=what)


# ----------------------------------------------------------------- kernel
@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def triangles(request):
    """name -> (T, lower, the loop's W), computed once per dtype."""
    dtype = request.param
    out = {}
    for name, (L, U) in IC.factor_pairs(problems, dtype).items():
        out[name + "_L"] = (L, True, IC.isai_loop(L, True, dtype))
        out[name + "_U"] = (U, False, IC.isai_loop(U, False, dtype))
    for name, T in IC.hand_triangles(dtype).items():
        out[name] = (T, True, IC.isai_loop(T, True, dtype))
    return dtype, out


def test_kernel_is_bitwise_the_loop(triangles):
    import krylov_amd

    dtype, cases = triangles
    assert max(int(IC.row_lengths(cases["ilu0_arrow300_L"][0]).max()),
               int(IC.row_lengths(IC.transposed(cases["ilu0_arrow300_U"][0])).max())) == 300
    for name, (T, lower, want) in cases.items():
        stats = {}
        got = krylov_amd.isai(T, lower=lower, stats=stats)
        _assert_same_matrix(got, want, name)
        assert stats["longest"] == int(IC.row_lengths(T if lower else IC.transposed(T)).max()), name


def test_upper_of_a_symmetric_ssor_is_the_transposed_lower():
    import krylov_amd

    P = krylov_amd.SsorPreconditioner(problems.poisson2d(12), omega=1.2, solve="isai")
    WL, WU = P.inverses()
    _assert_same_matrix(WU, IC.transposed(WL), "W_U = W_L^T")
    lo, up, _ = P.factors()
    _assert_same_matrix(WL, IC.isai_loop(lo, True, np.float64), "W_L")


def test_zero_pivots_name_the_smallest_row():
    import krylov_amd

    T = IC.hand_triangles(np.float64)["mixed"].copy()
    for i in (90, 7):
        T.data[T.indptr[i + 1] - 1] = 0.0
    with pytest.raises(np.linalg.LinAlgError, match=r"row 7\b"):
        krylov_amd.isai(T)
    T.data[T.indptr[8] - 1] = np.inf  # row 7 again, now non-finite
    with pytest.raises(np.linalg.LinAlgError, match=r"row 7\b"):
        krylov_amd.isai(T)
    with pytest.raises(np.linalg.LinAlgError, match=r"row 7\b"):
        krylov_amd.isai(IC.transposed(T), lower=False)


def test_a_row_of_1025_entries_is_refused():
    import krylov_amd

    n = 1025
    T = scipy.sparse.identity(n, format="lil")
    T[n - 1, :] = 0.001
    T[n - 1, n - 1] = 1.0
    T = T.tocsr()
    assert T.indptr[-1] - T.indptr[-2] == 1025
    with pytest.raises(NotImplementedError, match=r"row 1024\b.*1025 entries"):
        krylov_amd.isai(T)
    # 1,024 entries are taken
    S = T[:1024][:, :1024].tolil()
    S[1023, :] = 0.001
    S[1023, 1023] = 1.0
    S = S.tocsr()
    _assert_same_matrix(krylov_amd.isai(S), IC.isai_loop(S, True, np.float64), "1024-entry row")


def test_a_row_without_its_diagonal_is_refused():
    import krylov_amd

    D = np.tril(np.ones((5, 5))) + np.eye(5)
    D[3, 3] = 0.0
    with pytest.raises(ValueError, match=r"row 3\b.*diagonal"):
        krylov_amd.isai(scipy.sparse.csr_matrix(D))
    Up = np.triu(np.ones((5, 5)))  # an upper triangle handed in as a lower one
    with pytest.raises(ValueError, match="diagonal"):
        krylov_amd.isai(scipy.sparse.csr_matrix(Up))
    with pytest.raises(ValueError, match="solve must be"):
        krylov_amd.Ilu0Preconditioner(problems.poisson2d(6), solve="jacobi")
    with pytest.raises(ValueError, match="sweeps"):
        krylov_amd.SsorPreconditioner(problems.poisson2d(6), solve="isai", sweeps=-1)
    with pytest.raises(ValueError, match='goes with solve="isai"'):
        krylov_amd.SsorPreconditioner(problems.poisson2d(6), sweeps=1)
    with pytest.raises(ValueError, match='goes with solve="isai"'):
        krylov_amd.Ilu0Preconditioner(problems.poisson2d(6)).inverses()


# ------------------------------------------------------------------ apply
@pytest.fixture(scope="module")
def matrices():
    return {"poisson12": problems.poisson2d(12), "random3000": problems.random_nonsym(3000)}


def _parts(P):
    f = P.factors()
    WL, WU = P.inverses()
    return WL, WU, f[0], f[1], (f[2] if len(f) == 3 else None)


def _in_b(P, v):
    """A caller-numbered block in the numbering of P's factors."""
    return v if P.perm is None else v[P.perm]


@pytest.mark.parametrize("sweeps", [0, 1, 2])
@pytest.mark.parametrize("ordering", ["natural", "multicolor"])
@pytest.mark.parametrize("spec", [("ssor", 1.2), ("ilu0",)], ids=["ssor", "ilu0"])
def test_apply_is_the_chain_of_products(matrices, spec, ordering, sweeps):
    """P.solve(y) against scipy's products with P.inverses() and P.factors():
    within the componentwise bound of isai_cases.apply_bound, each product
    (m + 2) eps |M| |x| carried along the chain. k = 1, 3 (padded), 8, 128."""
    for name, A in matrices.items():
        n = A.shape[0]
        P = IC.device_precond(__import__("krylov_amd"), A, spec, np.float64, sweeps, ordering)
        lay = P.layout()
        assert lay["solve"] == "isai" and lay["sweeps"] == sweeps
        assert lay["launches"] == 2 + 4 * sweeps
        assert len(lay["stages"]) == 2 and lay["stages"][0]["scale"] == (spec[0] == "ssor")
        assert not any(s["isai"]["renumbered"] for s in lay["stages"])
        parts = _parts(P)
        Y = np.random.default_rng(3).standard_normal((n, 128))
        want, bound = IC.apply_bound(parts, _in_b(P, Y), sweeps)
        worst = 0.0
        for cols in (slice(0, 128), slice(0, 8), slice(0, 3), 0):
            got = P.solve(Y[:, cols])
            assert got.shape == Y[:, cols].shape and got.dtype == np.float64
            err = np.abs(_in_b(P, got) - want[:, cols])
            assert np.all(err <= bound[:, cols]), (name, cols, float(np.max(err / bound[:, cols])))
            worst = max(worst, float(np.max(err / bound[:, cols])))
        print(spec[0], ordering, sweeps, name, "worst |got - want| / bound", worst)
        assert np.max(bound) <= 1e-9 * np.max(np.abs(want))  # the bound is no escape hatch


@pytest.mark.parametrize("spec", [("ssor", 1.2), ("ilu0",)], ids=["ssor", "ilu0"])
def test_float32_apply(matrices, spec):
    A = matrices["poisson12"].astype(np.float32)
    P = IC.device_precond(__import__("krylov_amd"), A, spec, np.float32, 1)
    Y = np.random.default_rng(3).standard_normal((A.shape[0], 8)).astype(np.float32)
    want, bound = IC.apply_bound(_parts(P), Y, 1)
    got = P.solve(Y)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("spec", [("ssor", 1.2), ("ilu0",)], ids=["ssor", "ilu0"])
def test_two_colour_poisson_isai_is_the_exact_solve(matrices, spec):
    """Under the two-colour order W is the factor's inverse, so the ISAI apply
    agrees with the exact one within the chain's bound, and sweeps change
    nothing beyond theirs."""
    import krylov_amd

    A = matrices["poisson12"]
    Y = np.random.default_rng(3).standard_normal((A.shape[0], 8))
    make = ((lambda **kw: krylov_amd.SsorPreconditioner(A, omega=1.2, ordering="multicolor", **kw))
            if spec[0] == "ssor" else (lambda **kw: krylov_amd.Ilu0Preconditioner(A, ordering="multicolor", **kw)))
    exact = make()
    assert exact.layout()["colors"] == 2 and exact.layout()["solve"] == "exact"
    xe = exact.solve(Y)
    x0 = None
    for sweeps in (0, 1, 2):
        P = make(solve="isai", sweeps=sweeps)
        _, bound = IC.apply_bound(_parts(P), _in_b(P, Y), sweeps)
        got = P.solve(Y)
        err = np.abs(_in_b(P, got) - _in_b(P, xe))
        print(spec[0], sweeps, "isai against exact, worst / bound", float(np.max(err / bound)))
        assert np.all(err <= bound)
        if sweeps == 0:
            x0 = got
        else:
            assert np.all(np.abs(_in_b(P, got) - _in_b(P, x0)) <= bound)


def test_wide_blocks_go_to_isai_objects_only(matrices):
    import krylov_amd

    A = matrices["poisson12"]
    n = A.shape[0]
    B = np.random.default_rng(3).standard_normal((n, 128))
    P = krylov_amd.SsorPreconditioner(A, omega=1.2, solve="isai")
    assert P.max_cols == 256
    X, info = krylov_amd.cg(A, B, M=P, tol=1e-8)
    assert info.success
    assert np.all(np.linalg.norm(B - A @ X, axis=0) <= 1e-6 * np.linalg.norm(B, axis=0))
    _, one = krylov_amd.cg(A, B[:, 5], M=P, tol=1e-8)
    assert one.success and one.numsteps <= info.numsteps  # the block stops with its last column
    E = krylov_amd.SsorPreconditioner(A, omega=1.2)
    with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
        krylov_amd.cg(A, B, M=E)
    with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
        E @ B
    with pytest.raises(NotImplementedError, match="256 right-hand-side columns"):
        P @ np.ones((n, 257))


def test_refusals_are_unchanged(matrices):
    import krylov_amd
    import krylov_amd._helpers as helpers
    from krylov_amd import distributed
    from krylov_amd.precond import refuse_sharded

    A = problems.poisson2d(8)
    n = A.shape[0]
    P = krylov_amd.Ilu0Preconditioner(A, solve="isai", sweeps=1)
    P32 = krylov_amd.SsorPreconditioner(A, dtype=np.float32, solve="isai")
    with pytest.raises(ValueError, match="dtype="):
        krylov_amd.cg(A, np.ones(n), M=P32)
    with pytest.raises(ValueError, match="dtype="):
        krylov_amd.bicgstab(A, np.ones(n), Mr=P32)
    with pytest.raises(NotImplementedError, match="devices="):
        krylov_amd.cg(A, np.ones((n, 2)), M=P, devices=[0])
    with pytest.raises(ValueError, match="shape"):
        krylov_amd.cg(problems.poisson2d(7), np.ones(49), M=P)
    with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
        refuse_sharded(Ml=P)
    with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
        distributed._problem(A, np.ones((64, 1)), None, None, None, M=P)
    op = krylov_amd.CsrOperator(A)

    class Renumbered:
        renumbered = True

        def __getattr__(self, name):
            return getattr(op, name)

    orig = helpers.as_device_operator
    helpers.as_device_operator = lambda a, **kw: Renumbered()
    try:
        with pytest.raises(NotImplementedError, match="KRY_RENUMBER=0"):
            helpers.Problem(A, np.ones(64), None, None, M=P)
    finally:
        helpers.as_device_operator = orig
    with pytest.raises(ValueError, match="contradict"):
        krylov_amd.CsrOperator(A, like=Renumbered(), renumber=False)


def test_chain_step_is_the_direct_apply(matrices):
    """kry_prog_precond (what bicgstab's Ml= enqueues) is bitwise
    kry_precond_apply, and does nothing in a stopped chunk."""
    import krylov_amd
    from krylov_amd import _helpers, extra

    A = matrices["random3000"]
    n = A.shape[0]
    Y = np.random.default_rng(8).standard_normal((n, 4))
    for P in (krylov_amd.Ilu0Preconditioner(A, solve="isai", sweeps=1),
              krylov_amd.SsorPreconditioner(A, omega=1.2, solve="isai")):
        want = P.solve(Y)
        prob = _helpers.Problem(A, Y, None, None, Ml=P)
        assert not prob.A.renumbered
        D = extra._Dev(prob)
        C = extra._Chain(D, ["n"], cap=4)
        yv, xv = D.upload(Y), D.zeros()
        C.begin()
        assert C.apply("Ml", yv, xv, 0) is xv
        C.end(1)
        np.testing.assert_array_equal(_bits(xv.to_host()), _bits(want))
        P.matvec_device(yv, yv)  # in place: the stages never write what they still read
        np.testing.assert_array_equal(_bits(yv.to_host()), _bits(want))
        zv = D.zeros()
        C.set(None, np.full(4, 1.0))
        C.begin()
        C.sc(extra.SOP_SET, "n", 0, value=0.0)
        C.check("n", 0)
        C.apply("Ml", D.upload(Y), zv, 1)
        rows, _ = C.end(2)
        assert len(rows) == 1
        np.testing.assert_array_equal(zv.to_host(), np.zeros((n, 4)))


# ----------------------------------------------------------------- parity
@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(HERE, "golden", "precond_isai.npz"))


@pytest.mark.parametrize("case", IC.CASES, ids=lambda c: c[0])
def test_parity_with_the_reference(fixtures, case):
    """Step count and success equal; history within 1e-10 * want_k +
    2 * spread * want_0 (1e-4 * want_k for the float32 case, whose tolerance
    is 1e-4; bicgstab with the absolute floor 1e-14 ||r_0|| of
    tests/test_gpu_precond.py)."""
    import krylov_amd

    name, solver, slot, spec, sweeps, key, kw = case
    A, b = IC.problem(problems, key)
    P = IC.device_precond(krylov_amd, A, spec, A.dtype, sweeps)
    _, info = getattr(krylov_amd, solver)(A, b, **{slot: P}, **kw)
    rtol = 1e-4 if name.startswith("f32_") else 1e-10
    want = fixtures[name + "_resnorms"]
    got = np.asarray(info.resnorms, dtype=np.float64)
    print(name, "steps", info.numsteps, int(fixtures[name + "_numsteps"]), "spread", float(fixtures[name + "_spread"]))
    assert info.numsteps == int(fixtures[name + "_numsteps"])
    assert info.success and bool(fixtures[name + "_success"])
    assert got.shape == want.shape
    w0 = np.max(np.abs(want[0]))
    floor = 1e-14 * w0 if solver == "bicgstab" else 0.0
    bound = rtol * np.abs(want) + H.NOISE_FACTOR * float(fixtures[name + "_spread"]) * w0 + floor
    err = np.abs(got - want)
    print(name, "largest fraction of the bound used", float(np.max(err / bound)), "at", int(np.argmax(err / bound)))
    assert np.all(err <= bound), (float(np.max(err / bound)), int(np.argmax(err / bound)))
