"""richardson / jacobi / gauss_seidel / sor / ssor / chebyshev on the device
(krylov_amd/stationary.py, chebyshev.py) against the reference's own runs
(tests/golden/stationary.npz, made by tests/golden/make_stationary.py; the
cases are listed in tests/stationary_cases.py).

History bound: |got_k - want_k| <= rtol * want_k + 2 * spread * want_0, with
rtol = 1e-10 (the project's parity contract; 1e-4 for float32, its float32
contract) and spread the case's own spread recorded in the fixture: how far the
reference's history moves when only its inner product's summation order or its
sparse / dense branch changes (r = b - A x cancels, so late entries are
compared absolutely)."""
import os

import numpy as np
import pytest

from tests import gpu_helpers as H
from tests import stationary_cases as SC

pytestmark = pytest.mark.gpu

BITWISE_X = {"richardson_p40", "jacobi_rand", "jacobi_p40_block", "cheb_p40", "cheb_p40_block", "cheb_p40_weighted"}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "stationary.npz"))


def _cases():
    from krylov_amd import problems

    return {name: (solver, make) for name, solver, make in SC.big_cases(problems)}


def _run(name, callback=None, force_callback=False):
    import krylov_amd

    solver, make = _cases()[name]
    A, b, kw = make()
    if force_callback:
        kw = dict(kw, use_callback=True)
    sol, info = SC.call(krylov_amd, solver, A, b, kw, krylov_amd.WeightedInner, callback=callback)
    return A, b, sol, info


def _check_history(name, info, d):
    want = d[f"{name}_resnorms"]
    got = np.asarray(info.resnorms, dtype=np.float64)
    assert got.shape == want.shape
    rtol = 1e-4 if name.startswith("f32") else 1e-10
    bound = rtol * want + 2.0 * float(d[f"{name}_spread"]) * want[0]
    excess = np.abs(got - want) - bound
    worst = int(np.argmax(excess))
    print(f"{name}: worst |got - want| - bound = {excess.ravel()[worst]:.3e} at entry {worst} "
          f"(max |got - want| / want_0 = {np.max(np.abs(got - want)) / max(np.max(want[0]), 1e-300):.3e})")
    assert np.all(excess <= 0.0)


BIG = ["richardson_p40", "jacobi_rand", "jacobi_p40_block", "gs_rand_lower", "gs_rand_upper", "gs_p40",
       "sor_p40_lower", "sor_p40_upper", "sor_p40_block", "sor_p157", "ssor_p40", "ssor_rand", "ssor_perm",
       "f32_jacobi", "f32_sor", "cheb_p40", "cheb_p40_M", "cheb_p40_block", "cheb_p40_weighted"]


@pytest.mark.parametrize("name", BIG)
def test_matches_reference_fixture(name, fixture):
    d = fixture
    seen = []
    A, b, sol, info = _run(name, callback=lambda x, r: seen.append(1))
    assert info.numsteps == int(d[f"{name}_numsteps"])
    assert info.success == bool(d[f"{name}_success"])
    if info.success:
        assert sol is info.xk
    else:
        assert sol is None
    if seen:  # the case with a callback
        assert len(seen) == info.numsteps + 1
    # the n = 90,000 permuted matrix stays in the caller's order on the device: renumbering starts where x
    # outgrows 8 MB, and there the triangular solvers refuse the operator (NotImplementedError)
    if name == "ssor_perm":
        assert info.renumbered is False
    if name.startswith("f32"):
        assert info.xk.dtype == np.float32 and np.asarray(info.resnorms).dtype == np.float32
    _check_history(name, info, d)
    if f"{name}_x" in d.files:
        xr, xg = d[f"{name}_x"], info.xk
    else:
        xr, xg = d[f"{name}_xs"], info.xk[SC.sample_index(info.xk.shape[0])]
    xtol = 1e-4 if name.startswith("f32") else 1e-9
    assert np.max(np.abs(xg - xr)) <= xtol * np.max(np.abs(xr))
    if name in BITWISE_X:
        # every line is elementwise and the SpMV is bitwise csr_matvec
        np.testing.assert_array_equal(xg, xr)


@pytest.mark.parametrize("name", ["richardson_p40", "jacobi_rand", "gs_rand_upper", "sor_p40_lower", "ssor_p40",
                                  "ssor_perm", "cheb_p40_M", "f32_sor"])
def test_chunking_is_invisible(name):
    """Chunks of 32 iterations against one iteration per chunk (a callback):
    bitwise the same history and iterate; the callback sees every iterate."""
    _, _, _, fast = _run(name)
    seen = []
    _, _, _, slow = _run(name, callback=lambda x, r: seen.append((x.shape, r.shape)), force_callback=True)
    assert fast.numsteps == slow.numsteps and fast.success == slow.success
    np.testing.assert_array_equal(np.asarray(fast.resnorms), np.asarray(slow.resnorms))
    np.testing.assert_array_equal(fast.xk, slow.xk)
    assert len(seen) == slow.numsteps + 1
    assert all(s == (fast.xk.shape, fast.xk.shape) for s in seen)


@pytest.mark.parametrize("solver", SC.STATIONARY + ("chebyshev",))
def test_reference_small_cases(solver, fixture):
    """tests/test_richardson.py ... test_gauss_seidel.py / test_chebyshev.py
    of the reference, restated: the callback is called numsteps + 1 times and
    helpers.assert_consistent holds; step counts and success as the reference's."""
    import krylov_amd

    d = fixture
    mine = [c for c in SC.small_cases(H) if c[1] == solver]
    assert len(mine) == (6 if solver == "chebyshev" else 8)
    for name, _, make in mine:
        A, b, kw = make()
        count = []
        sol, info = SC.call(krylov_amd, solver, A, b, dict(kw, use_callback=True), None,
                            callback=lambda x, r: count.append(1))
        assert len(count) == info.numsteps + 1, name
        assert info.numsteps == int(d[f"{name}_numsteps"]), name
        assert info.success == bool(d[f"{name}_success"]), name
        assert (sol is info.xk) if info.success else (sol is None), name
        H.assert_consistent(A, b, info, sol, kw["tol"])


def test_divergence_is_survived():
    """sor with omega = 1.8 on the random nonsymmetric matrix diverges (the
    reference overflows to inf): the call returns after maxiter steps without
    raising."""
    import krylov_amd
    from krylov_amd import problems

    A = problems.random_nonsym(5000)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    with np.errstate(all="ignore"):
        sol, info = krylov_amd.sor(A, b, omega=1.8, maxiter=40)
    assert info.numsteps == 40 and info.success is False and sol is None
    assert len(info.resnorms) == 41


def test_x0_is_copied_and_operators_are_accepted_where_possible():
    import krylov_amd
    from krylov_amd import problems

    A = problems.poisson2d(40)
    b = np.random.default_rng(3).standard_normal(A.shape[0])
    x0 = np.ones(A.shape[0])
    keep = x0.copy()
    _, info = krylov_amd.gauss_seidel(A, b, x0=x0, tol=0.0, maxiter=5)
    np.testing.assert_array_equal(x0, keep)
    assert info.xk is not x0 and info.numsteps == 5
    op = krylov_amd.CsrOperator(A)
    _, a = krylov_amd.richardson(op, b, omega=0.2, tol=0.0, maxiter=7)
    _, c = krylov_amd.richardson(A, b, omega=0.2, tol=0.0, maxiter=7)
    np.testing.assert_array_equal(a.xk, c.xk)
    _, a = krylov_amd.chebyshev(op, b, (0.01, 8.0), tol=0.0, maxiter=7)
    _, c = krylov_amd.chebyshev(A, b, (0.01, 8.0), tol=0.0, maxiter=7)
    np.testing.assert_array_equal(a.xk, c.xk)
