"""Host checks that the float32 cases (tests/f32_cases.py) have teeth: the
variants agree with the float64 reference to a tight envelope, two wrong
inner products fail the bound on every small case, the stop-at-tolerance
cases stop where every variant stops, and the case table reaches the
geometries it is meant to. CPU only; the device side is
tests/test_gpu_f32.py."""
import numpy as np
import pytest

from tests import f32_cases as F


@pytest.mark.parametrize("cid", F.ids(F.SMALL))
def test_variants_and_mutants(cid):
    """Every variant gives a finite history with the float64 run's step
    count, the envelope stays below ENVELOPE_CAP, the default inner's result
    dtypes are the reference's (float32; MINRES keeps its QR and so its
    history in float64); a dropped tail and an inner product off by 1e-5 both
    fail the bound."""
    c, R = F.case(cid), F.reference(cid)
    ref = R["ref"]
    assert ref["numsteps"] == F.STEPS and not ref["success"]
    for name, run in R["variants"].items():
        assert run["numsteps"] == ref["numsteps"], name
        assert np.all(np.isfinite(run["resnorms"])) and np.all(np.isfinite(run["xk"])), name
        assert run["xk"].dtype == np.float32, name
        uh, ux = F.used(run, R, c)
        assert uh <= 1.0 / F.NOISE_FACTOR and ux <= 1.0 / F.NOISE_FACTOR, name
    assert R["env"].shape == (F.STEPS + 1,) and np.all(np.diff(R["env"]) >= 0.0)
    assert R["env"][-1] < F.ENVELOPE_CAP and R["xenv"] < F.ENVELOPE_CAP, (R["env"][-1], R["xenv"])
    # no column has run down to float32 round-off of its start, where the
    # recurrence would only carry noise
    h = F.hist64(ref)
    assert np.all(h[-1] > F.EPS32 * h[0])
    assert R["default"]["xk"].dtype == np.float32
    assert R["default"]["resnorms"].dtype == (np.float64 if c[1] == "minres" else np.float32)
    n = F.matrix(c[2]).shape[0]
    for kind in ("tail", "scaled"):
        m = F.run_oracle(c, np.float32, F.mutant_inner(kind, n))
        assert m["numsteps"] == ref["numsteps"]
        uh, _ = F.used(m, R, c)
        print(f"{cid} mutant {kind}: history dev/bound {uh:.3g}")
        assert uh > 1.0, (kind, uh)


@pytest.mark.parametrize("cid", F.ids(F.STOP))
def test_stop_cases_stop_together(cid):
    """tol = 1e-4: the float64 run, every variant and the default inner stop
    with success at the same step, and each history lies at least 1 % away
    from the criterion at that step and the one before."""
    c, R = F.case(cid), F.reference(cid)
    ref = R["ref"]
    assert ref["success"] and 2 <= ref["numsteps"] < c[4]["maxiter"]
    assert F.stop_margin(ref) >= F.STOP_MARGIN
    h = F.hist64(ref)
    assert h[-2] > F.STOP_TOL * h[0] >= h[-1]
    for name, run in list(R["variants"].items()) + [("default", R["default"])]:
        assert run["success"] and run["numsteps"] == ref["numsteps"], name
        assert F.stop_margin(run) >= F.STOP_MARGIN, name
        uh, ux = F.used(run, R, c)
        assert uh <= 1.0 and ux <= 1.0, (name, uh, ux)


def test_block_geometry():
    """What the case table reaches, as arithmetic: n mod 4 takes every value;
    k = 2 with odd n gives a flat length 2 n = 2 (mod 4), so a 4-wide lane
    group straddles the end of the block; a 2-column row is narrower than one
    lane's group; k = 3 runs as 4 columns; the scaled tail carries at least a
    tenth of ||b||^2 in every column (0.47 to 0.99), so dropping it is an O(1)
    error."""
    assert sorted(n % F.W for n in F.SIZES) == [0, 1, 2, 3]
    odd = [n for n in F.SIZES if n % 2]
    assert len(odd) == 2 and all((2 * n) % F.W == 2 for n in odd)
    assert 2 < F.W and 1 << (3 - 1).bit_length() == 4
    for solver, prefix in (("cg", "band"), ("minres", "band"), ("minres", "indef"), ("gmres", "nonsym")):
        got = {(F.matrix(c[2]).shape[0], c[3]) for c in F.select(solver=solver, matrix_prefix=prefix, plain=True)}
        assert got == {(n, k) for n in F.SIZES for k in F.COLUMNS}, (solver, prefix)
    for n in F.SIZES:
        for k in F.COLUMNS:
            B = F.rhs(n, k).astype(np.float64).reshape(n, k)
            share = np.sum(B[-F.TAIL:] ** 2, axis=0) / np.sum(B ** 2, axis=0)
            assert B.dtype == np.float64 and np.all(share > 0.1), (n, k, share)
    assert F.matrix("poisson63").shape[0] == 3969 and F.matrix("poisson64").shape[0] == 4096


def test_matrices_are_what_the_solvers_need():
    """float32, canonical; the band is symmetric and strictly diagonally
    dominant with a positive diagonal (SPD), the shifted one symmetric with a
    diagonal of both signs (indefinite)."""
    for n in F.SIZES:
        A = F.matrix(f"band{n}")
        assert A.dtype == np.float32 and A.has_sorted_indices and A.shape == (n, n)
        assert abs(A - A.T).nnz == 0
        d = A.diagonal().astype(np.float64)
        off = np.asarray(abs(A.astype(np.float64)).sum(axis=1)).ravel() - np.abs(d)
        assert np.all(d > off)
        offsets = np.unique(A.tocoo().col - A.tocoo().row)
        assert sorted(offsets.tolist()) == [-301, -17, -1, 0, 1, 17, 301]
        S = F.matrix(f"indef{n}")
        assert S.dtype == np.float32 and abs(S - S.T).nnz == 0
        assert S.diagonal().min() < 0.0 < S.diagonal().max()
        assert F.matrix(f"nonsym{n}").dtype == np.float32


def test_large_sizes_sit_on_the_float_kernel_bands():
    """The register-resident MGS serves 256 blocks x 512 threads x E elements,
    E up to 32 in float32 (16 in float64): m = 1449 is the first size past
    E = 16, m = 2048 the last at E = 32 with a full grid, m = 2049 the first
    streamed one with n mod 4 = 1."""
    grid = 256 * 512
    n = [m * m for m in F.LARGE_M]
    assert 1448 ** 2 <= 16 * grid < n[0] <= 32 * grid and n[0] % (512 * 32) != 0
    assert n[1] == 32 * grid
    assert n[2] > 32 * grid and n[2] % F.W == 1
    assert [c[4]["maxiter"] for c in F.LARGE] == [F.LARGE_STEPS] * 3
