"""Factorised preconditioners (SsorPreconditioner, Ilu0Preconditioner) in the
preconditioner slots of the solvers: the apply against its own stages, the
solves against the reference's results with the same preconditioners written
on scipy triangular solves (tests/golden/precond_factored.npz,
tests/precond_factored_cases.py), and the interface's refusals."""
import os

import numpy as np
import pytest
import scipy.sparse

from krylov_amd import problems
from tests import gpu_helpers as H
from tests import precond_factored_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(HERE, "golden", "precond_factored.npz"))


@pytest.fixture(scope="module")
def matrices():
    return {"poisson12": problems.poisson2d(12), "random3000": problems.random_nonsym(3000, 6, 2.0, 0)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("kind", ["ssor", "ilu0"])
@pytest.mark.parametrize("name", ["poisson12", "random3000"])
def test_apply_is_the_composition_of_its_stages(matrices, kind, name):
    import krylov_amd

    A = matrices[name]
    n = A.shape[0]
    P = krylov_amd.SsorPreconditioner(A, omega=1.2) if kind == "ssor" else krylov_amd.Ilu0Preconditioner(A)
    Y = np.random.default_rng(3).standard_normal((n, 8))
    f = P.factors()
    lo = krylov_amd.TriangularOperator(f[0], lower=True)
    up = krylov_amd.TriangularOperator(f[1], lower=False)

    def compose(y):
        t = lo.solve(y)
        if kind == "ssor":
            t = (t.T * f[2]).T
        return up.solve(t)

    got8 = P @ Y
    assert got8.shape == (n, 8) and got8.dtype == np.float64
    np.testing.assert_array_equal(_bits(got8), _bits(compose(Y)))
    got1 = P.solve(Y[:, 0])
    assert got1.shape == (n,)
    np.testing.assert_array_equal(_bits(got1), _bits(compose(Y[:, 0])))
    np.testing.assert_array_equal(_bits(got8[:, 0]), _bits(got1))  # independent of k
    got3 = P @ Y[:, :3]  # padded to 4 columns
    assert got3.shape == (n, 3)
    np.testing.assert_array_equal(_bits(got3), _bits(got8[:, :3]))
    stages = P.layout()["stages"]
    assert len(stages) == (3 if kind == "ssor" else 2)
    assert stages[0]["levels"] >= 1 and stages[-1]["launches"] >= 1


# ----------------------------------------------------------------- parity
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c[0])
def test_parity_with_the_reference(fixtures, case):
    """Step count, success and num_operations equal; history within
    rtol * want_k + NOISE_FACTOR * spread * want_0 (rtol 1e-10, 1e-4 for the
    float32 case; bicgstab / cgs with the absolute floor 1e-14 ||r_0|| of
    tests/test_gpu_precond.py); xk within 1e-9 (1e-4) of max |x|."""
    import krylov_amd

    name, solver, slot, spec, key, kw = case
    A, b = PC.problem(problems, key)
    P = PC.device_precond(krylov_amd, A, spec, A.dtype)
    eigs = fixtures[name + "_eigs"] if solver == "chebyshev" else None
    _, info = PC.call(krylov_amd, solver, A, b, slot, P, kw, eigs=eigs)
    f32 = name.startswith("f32_")
    rtol, xtol = (1e-4, 1e-4) if f32 else (1e-10, 1e-9)
    want = fixtures[name + "_resnorms"]
    got = np.asarray(info.resnorms, dtype=np.float64)
    print(name, "steps", info.numsteps, int(fixtures[name + "_numsteps"]), "spread", float(fixtures[name + "_spread"]))
    assert info.numsteps == int(fixtures[name + "_numsteps"])
    assert info.success == bool(fixtures[name + "_success"])
    assert got.shape == want.shape
    w0 = np.max(np.abs(want[0]))
    floor = 1e-14 * w0 if solver in ("bicgstab", "cgs") else 0.0
    bound = rtol * np.abs(want) + H.NOISE_FACTOR * float(fixtures[name + "_spread"]) * w0 + floor
    err = np.abs(got - want)
    print(name, "worst |got - want| / bound", float(np.max(err / bound)), "at", int(np.argmax(err / bound)))
    assert np.all(err <= bound), (float(np.max(err / bound)), int(np.argmax(err / bound)))
    xr = fixtures[name + "_xk"]
    xerr = float(np.max(np.abs(np.asarray(info.xk) - xr)) / np.max(np.abs(xr)))
    print(name, "x error / max|x|", xerr)
    assert xerr <= xtol
    ops = info.num_operations
    if ops is None:
        assert np.all(np.isnan(fixtures[name + "_ops"]))
    else:
        np.testing.assert_array_equal([ops[k] for k in ("A", "M", "Ml", "Mr", "inner", "axpy")],
                                      fixtures[name + "_ops"])


# -------------------------------------------------------------- interface
def test_callback_sees_every_iterate(fixtures):
    import krylov_amd

    A, b = PC.problem(problems, "p40")
    P = krylov_amd.SsorPreconditioner(A, omega=1.2)
    seen = []
    _, info = krylov_amd.cg(A, b, M=P, tol=1e-8, callback=lambda x, r: seen.append(x.shape))
    assert info.numsteps == int(fixtures["cg_p40_ssor_numsteps"])
    assert len(seen) == info.numsteps + 1


def test_a_setter_replaces_the_slot_and_needs_a_new_start(matrices):
    """One CG state over poisson2d(12): a factorised M, then
    kry_cg_set_preconditioners with a matrix M (which clears the factorised
    one), then the factorised M again through kry_cg_set_precond. After each
    setter a run is refused until the next start, and the history then equals,
    bitwise, a fresh solver's that was given only that M."""
    import krylov_amd
    from krylov_amd import _helpers
    from krylov_amd._lib import check, lib
    from krylov_amd.cg import _CGState

    S = matrices["poisson12"]
    A = krylov_amd.CsrOperator(S)
    b = np.random.default_rng(5).standard_normal(S.shape[0])
    fac = krylov_amd.SsorPreconditioner(S, omega=1.2)
    jac = scipy.sparse.diags(1.0 / S.diagonal(), format="csr")
    steps = 10

    def fresh(M):
        st = _CGState(_helpers.Problem(A, b, None, None, M=M))
        st.start()
        st.set_criterion(np.zeros(1))
        return st

    def restarted(st):
        with pytest.raises(ValueError, match="kry_cg_start has not been called"):
            st.run(steps)
        st.start()
        st.set_criterion(np.zeros(1))
        return st.run(steps)

    only_jac = fresh(jac)
    want_jac = only_jac.run(steps)
    want_fac = fresh(fac).run(steps)
    assert want_jac.shape == want_fac.shape == (steps, 1)
    assert not np.array_equal(_bits(want_jac), _bits(want_fac))

    st = fresh(fac)
    np.testing.assert_array_equal(_bits(st.run(steps)), _bits(want_fac))
    check(lib.kry_cg_set_preconditioners(st.h, only_jac.prob.ops["M"].handle, None))
    np.testing.assert_array_equal(_bits(restarted(st)), _bits(want_jac))
    check(lib.kry_cg_set_precond(st.h, 0, fac.handle))
    np.testing.assert_array_equal(_bits(restarted(st)), _bits(want_fac))


def test_gmres_restarted_with_ml(matrices):
    import krylov_amd

    A = matrices["random3000"]
    b = np.ones(A.shape[0])
    P = krylov_amd.Ilu0Preconditioner(A)
    x, infos = krylov_amd.gmres_restarted(A, b, Ml=P, tol=1e-8, restart=10, max_cycles=10)
    assert infos[-1].success
    assert np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b)


def test_constructor_errors():
    import krylov_amd

    A = problems.poisson2d(6)
    for cls in (krylov_amd.SsorPreconditioner, krylov_amd.Ilu0Preconditioner):
        with pytest.raises(TypeError, match="CsrOperator does not keep"):
            cls(krylov_amd.CsrOperator(A))
        with pytest.raises(TypeError, match="complex"):
            cls(A.astype(np.complex128))
        with pytest.raises(ValueError, match="square"):
            cls(np.ones((3, 4)))
        with pytest.raises(TypeError, match="scipy.sparse matrix or a dense"):
            cls([[1.0]])
    Z = A.tolil()
    Z[3, 3] = 0.0
    with pytest.raises(np.linalg.LinAlgError, match="row 3"):
        krylov_amd.SsorPreconditioner(Z.tocsr())
    nodiag = scipy.sparse.csr_matrix(np.array([[1.0, 2.0], [3.0, 0.0]]))
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        krylov_amd.Ilu0Preconditioner(nodiag)
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        krylov_amd.SsorPreconditioner(nodiag)


def test_solve_refusals():
    import krylov_amd

    A = problems.poisson2d(8)
    n = A.shape[0]
    P = krylov_amd.SsorPreconditioner(A)
    with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
        krylov_amd.cg(A, np.ones((n, 65)), M=P)
    with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
        P @ np.ones((n, 65))
    P32 = krylov_amd.SsorPreconditioner(A, dtype=np.float32)
    with pytest.raises(ValueError, match="dtype="):
        krylov_amd.cg(A, np.ones(n), M=P32)
    with pytest.raises(ValueError, match="dtype="):
        krylov_amd.bicgstab(A, np.ones(n), Mr=P32)
    with pytest.raises(NotImplementedError, match="devices="):
        krylov_amd.cg(A, np.ones((n, 2)), M=P, devices=[0])
    with pytest.raises(ValueError, match="shape"):
        krylov_amd.cg(problems.poisson2d(7), np.ones(49), M=P)


def test_sharded_drivers_refuse():
    from krylov_amd import distributed
    from krylov_amd.precond import refuse_sharded

    import krylov_amd

    A = problems.poisson2d(8)
    P = krylov_amd.Ilu0Preconditioner(A)
    refuse_sharded(M=A, Ml=None, Mr=[A, A])  # matrices pass
    for kw in ({"M": P}, {"Ml": P}, {"Mr": [P]}):
        with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
            refuse_sharded(**kw)
    with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
        distributed._problem(A, np.ones((64, 1)), None, None, None, M=P)


def test_renumbered_operator_is_refused():
    """The refusal Problem raises for an operator renumbered at upload,
    through a stand-in operator that says it was (a real one needs x over
    8 MB)."""
    import krylov_amd
    from krylov_amd._helpers import Problem

    A = problems.poisson2d(8)
    P = krylov_amd.SsorPreconditioner(A)
    op = krylov_amd.CsrOperator(A)

    class Renumbered:
        renumbered = True

        def __getattr__(self, name):
            return getattr(op, name)

    import krylov_amd._helpers as helpers

    orig = helpers.as_device_operator
    helpers.as_device_operator = lambda a, **kw: Renumbered()
    try:
        with pytest.raises(NotImplementedError, match="KRY_RENUMBER=0"):
            Problem(A, np.ones(64), None, None, M=P)
    finally:
        helpers.as_device_operator = orig
