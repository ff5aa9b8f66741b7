"""Multicolour SSOR and ILU(0) preconditioners (ordering="multicolor") and the
ordered triangular solve on the device: bitwise against the natural-order
objects built on the explicitly permuted matrix B = A[perm][:, perm], the
ILU(0) values against the sequential loop on B, the fused apply against the
unfused one with the launch counts of both, the solves against the reference's
results with the host model of the same preconditioner
(tests/golden/precond_multicolor.npz, tests/golden/make_precond_multicolor.py),
the level structure, and the interface's refusals."""
import os

import numpy as np
import pytest

from krylov_amd import problems
from tests import gpu_helpers as H
from tests import multicolor_cases as MC
from tests import precond_factored_cases as PC
from tests import tri_cases as TC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["poisson12", "poisson64", "random3000", "random20000", "arrow300"]
SPECS = {"ssor": ("ssor", 1.2), "ilu0": ("ilu0",)}


@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(HERE, "golden", "precond_multicolor.npz"))


@pytest.fixture(scope="module")
def ordered():
    """name -> (A, perm, B, Y): the matrix, its multicolour permutation from
    the Python model, B = A[perm][:, perm] and an (n, 8) right-hand side."""
    out = {}
    for name in NAMES:
        A = MC.matrix(problems, name)
        _, perm = MC.color_py(A)
        out[name] = (A, perm, MC.permuted(A, perm), np.random.default_rng(7).standard_normal((A.shape[0], 8)))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _device(A, spec, dtype, ordering):
    import krylov_amd

    if spec[0] == "ssor":
        return krylov_amd.SsorPreconditioner(A, omega=spec[1], dtype=dtype, ordering=ordering)
    return krylov_amd.Ilu0Preconditioner(A, dtype=dtype, ordering=ordering)


# ---------------------------------------------------- bitwise, existing path
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["ssor", "ilu0"])
@pytest.mark.parametrize("name", NAMES)
def test_apply_is_the_natural_apply_on_the_permuted_matrix(ordered, name, kind, dtype):
    A, perm, B, Y = ordered[name]
    P = _device(A, SPECS[kind], dtype, "multicolor")
    Q = _device(B, SPECS[kind], dtype, "natural")
    np.testing.assert_array_equal(P.perm, perm)
    Y = Y.astype(dtype)
    for k in (1, 3, 8):
        y = Y[:, 0] if k == 1 else Y[:, :k]
        got = P.solve(y)
        want = np.empty_like(got)
        want[perm] = Q.solve(y[perm])
        assert got.dtype == np.dtype(dtype) and got.shape == y.shape
        assert np.all(np.isfinite(got))
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"k={k}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_ordered_triangular_solve_is_the_permuted_triangles(ordered, name, lower, dtype):
    import krylov_amd

    A, perm, B, Y = ordered[name]
    rank = MC.rank_of(perm)
    T = krylov_amd.TriangularOperator(MC.split_by_rank(A, rank, lower), lower=lower, dtype=dtype, order=perm)
    TB = krylov_amd.TriangularOperator(TC.triangle(B, lower), lower=lower, dtype=dtype)
    assert T.layout()["levels"] == TB.layout()["levels"] and T.layout()["launches"] == TB.layout()["launches"]
    Y = Y.astype(dtype)
    for k in (1, 3, 8):
        y = Y[:, 0] if k == 1 else Y[:, :k]
        got = T.solve(y)
        want = np.empty_like(got)
        want[perm] = TB.solve(y[perm])
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"k={k}")
    with pytest.raises(ValueError, match="in the given order"):
        krylov_amd.TriangularOperator(MC.split_by_rank(A, rank, lower), lower=not lower, dtype=dtype, order=perm)


# ------------------------------------------------------------ ILU(0) values
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["poisson12", "random3000", "arrow300"])
def test_ilu0_values_are_the_sequential_loop_on_b(ordered, name, dtype):
    import krylov_amd

    A, perm, B, _ = ordered[name]
    P = krylov_amd.Ilu0Preconditioner(A, dtype=dtype, ordering="multicolor")
    want = PC.ilu0_loop(B, dtype)
    np.testing.assert_array_equal(P.lu.indptr, want.indptr)
    np.testing.assert_array_equal(P.lu.indices, want.indices)
    assert P.lu.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(_bits(P.lu.data), _bits(want.data))
    L, U = P.factors()
    Lw, Uw = PC.split_lu(want)
    np.testing.assert_array_equal(_bits(L.toarray()), _bits(Lw.toarray()))
    np.testing.assert_array_equal(_bits(U.toarray()), _bits(Uw.toarray()))


# ------------------------------------------------------------------- fusion
def _pair(monkeypatch, A, spec, dtype=np.float64):
    """(fused, unfused): the switch is read when the object is created."""
    monkeypatch.delenv("KRY_PRECOND_FUSE", raising=False)
    fused = _device(A, spec, dtype, "multicolor")
    monkeypatch.setenv("KRY_PRECOND_FUSE", "0")
    unfused = _device(A, spec, dtype, "multicolor")
    monkeypatch.delenv("KRY_PRECOND_FUSE")
    return fused, unfused


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["ssor", "ilu0"])
@pytest.mark.parametrize("name", NAMES)
def test_fused_apply_is_the_unfused_apply(monkeypatch, ordered, name, kind, dtype):
    A, perm, B, Y = ordered[name]
    fused, unfused = _pair(monkeypatch, A, SPECS[kind], dtype)
    assert fused.layout()["fused"] and not unfused.layout()["fused"]
    assert fused.layout()["launches"] < unfused.layout()["launches"] or kind == "ilu0"
    Y = Y.astype(dtype)
    for y in (Y[:, 0], Y[:, :3], Y):
        np.testing.assert_array_equal(_bits(fused.solve(y)), _bits(unfused.solve(y)))


def test_launch_counts(monkeypatch, ordered):
    def stage_launches(P):
        return sum(s["launches"] if "launches" in s else 1 for s in P.layout()["stages"])

    A = ordered["poisson64"][0]
    for kind, want_unfused, want_fused in (("ssor", 5, 3), ("ilu0", 4, 3)):
        fused, unfused = _pair(monkeypatch, A, SPECS[kind])
        lay = fused.layout()
        assert lay["ordering"] == "multicolor" and lay["colors"] == 2 and lay["color_sizes"] == [2048, 2048]
        assert unfused.layout()["launches"] == want_unfused == stage_launches(unfused)
        assert lay["launches"] == want_fused
    # an irregular graph: the boundary levels hold different rows, so only the scale's launch goes
    A = ordered["random20000"][0]
    for kind, saved in (("ssor", 1), ("ilu0", 0)):
        fused, unfused = _pair(monkeypatch, A, SPECS[kind])
        assert unfused.layout()["launches"] == stage_launches(unfused)
        assert fused.layout()["launches"] == unfused.layout()["launches"] - saved
        assert fused.layout()["color_sizes"] == MC.COLOR_SIZES["random20000"]
    # everything in one grouped launch per solve: nothing to fuse at the boundary
    fused, unfused = _pair(monkeypatch, ordered["poisson12"][0], SPECS["ssor"])
    assert (fused.layout()["launches"], unfused.layout()["launches"]) == (2, 3)
    # natural order: one launch per stage launch, as before, whatever the switch says
    for name in ("poisson64", "random20000"):
        for kind in ("ssor", "ilu0"):
            P = _device(ordered[name][0], SPECS[kind], np.float64, "natural")
            lay = P.layout()
            assert lay["launches"] == stage_launches(P) and not lay["fused"]
            assert lay["ordering"] == "natural" and lay["colors"] is None and P.perm is None and P.colors is None


# ---------------------------------------------------------------- structure
def test_two_levels_per_solve_on_the_stencil(ordered):
    A = ordered["poisson64"][0]
    for kind in ("ssor", "ilu0"):
        mc = [s for s in _device(A, SPECS[kind], np.float64, "multicolor").layout()["stages"] if "levels" in s]
        nat = [s for s in _device(A, SPECS[kind], np.float64, "natural").layout()["stages"] if "levels" in s]
        assert [s["levels"] for s in mc] == [2, 2] and [s["max_level"] for s in mc] == [2048, 2048]
        assert [s["levels"] for s in nat] == [127, 127]


# ------------------------------------------------------------------- parity
def _cases():
    return [c for c in PC.CASES
            if c[1] != "chebyshev" and not any(isinstance(c[5].get(nm), tuple) for nm in ("M", "Ml", "Mr"))]


STEPS = {"cg_p40_ssor": 39, "cg_p40_ilu0": 38, "cg_p40_ssor_block": 63, "cg_p40_ml": 15, "minres_p40_ssor": 39,
         "gmres_r3k_mr": 9, "gmres_r3k_ml": 9, "gmres_r3k_m_mgs2": 20, "bicgstab_r3k_mr": 5, "cgs_r3k_m": 5,
         "f32_cg_p40_ssor": 27}


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_parity_with_the_reference(fixtures, case):
    """Step count and success equal; history within rtol * want_k +
    NOISE_FACTOR * spread * want_0 (rtol 1e-10, 1e-4 for the float32 case; the
    rule of tests/test_gpu_precond_factored.py without its absolute floor for
    bicgstab / cgs); xk within 1e-9 (1e-4) plus
    NOISE_FACTOR * spread of max |x|: an iterate moves with the summation order
    as its history does. cg_p40_ml (15 fixed steps with the nonsymmetric
    product Ml A) diverges in the reference, to 1e17 with a spread of 2e15
    between its own variants, so only its step count and success say anything."""
    import krylov_amd

    name, solver, slot, spec, key, kw = case
    A, b = PC.problem(problems, key)
    P = _device(A, spec, A.dtype, "multicolor")
    _, info = PC.call(krylov_amd, solver, A, b, slot, P, kw)
    f32 = name.startswith("f32_")
    rtol, xtol = (1e-4, 1e-4) if f32 else (1e-10, 1e-9)
    want = fixtures[name + "_resnorms"]
    got = np.asarray(info.resnorms, dtype=np.float64)
    print(name, "steps", info.numsteps, int(fixtures[name + "_numsteps"]), "spread", float(fixtures[name + "_spread"]))
    assert int(fixtures[name + "_numsteps"]) == STEPS[name]
    assert info.numsteps == int(fixtures[name + "_numsteps"])
    assert info.success == bool(fixtures[name + "_success"])
    assert got.shape == want.shape
    w0 = np.max(np.abs(want[0]))
    bound = rtol * np.abs(want) + H.NOISE_FACTOR * float(fixtures[name + "_spread"]) * w0
    err = np.abs(got - want)
    print(name, "worst |got - want| / bound", float(np.max(err / bound)), "at", int(np.argmax(err / bound)))
    assert np.all(err <= bound), (float(np.max(err / bound)), int(np.argmax(err / bound)))
    xr = fixtures[name + "_xk"]
    xerr = float(np.max(np.abs(np.asarray(info.xk) - xr)) / np.max(np.abs(xr)))
    print(name, "x error / max|x|", xerr)
    assert xerr <= xtol + H.NOISE_FACTOR * float(fixtures[name + "_spread"])


# ---------------------------------------------------------------- interface
def test_errors_and_refusals():
    import krylov_amd
    from krylov_amd import distributed
    from krylov_amd._helpers import Problem
    from krylov_amd.precond import refuse_sharded

    A = problems.poisson2d(8)
    n = A.shape[0]
    for cls in (krylov_amd.SsorPreconditioner, krylov_amd.Ilu0Preconditioner):
        with pytest.raises(ValueError, match="ordering must be"):
            cls(A, ordering="rcm")
        P = cls(A, ordering="multicolor")
        assert P.ordering == "multicolor" and P.factored and not P.renumbered
        np.testing.assert_array_equal(np.bincount(P.colors), [32, 32])
        with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
            krylov_amd.cg(A, np.ones((n, 65)), M=P)
        with pytest.raises(NotImplementedError, match="64 right-hand-side columns"):
            P @ np.ones((n, 65))
        with pytest.raises(NotImplementedError, match="devices="):
            krylov_amd.cg(A, np.ones((n, 2)), M=P, devices=[0])
        with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
            refuse_sharded(M=P)
        with pytest.raises(NotImplementedError, match="krylov_amd.distributed"):
            distributed._problem(A, np.ones((n, 1)), None, None, None, M=P)
        P32 = cls(A, dtype=np.float32, ordering="multicolor")
        with pytest.raises(ValueError, match="dtype="):
            krylov_amd.cg(A, np.ones(n), M=P32)
        with pytest.raises(ValueError, match="shape"):
            krylov_amd.cg(problems.poisson2d(7), np.ones(49), M=P)
        # an operator renumbered at upload, through a stand-in that says it was
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
                Problem(A, np.ones(n), None, None, M=P)
        finally:
            helpers.as_device_operator = orig
