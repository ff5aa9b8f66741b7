"""The streamed persistent MGS kernel (gm_mgsl_kernel): all MGS passes of an
Arnoldi step in one launch with w held in registers and the basis streamed,
for n·k beyond the register-resident kernel's ~2.1 M doubles (up to ~10.5 M:
the BASELINE metric's GMRES(30), tests/test_gpu_fullsize_golden.py).

Its passes sum the inner products in a different grouping from the
launch-per-pass kernels, so the two paths agree to rounding; both follow the
reference's iteration (oracle) to 1e-10.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poisson1800():
    from krylov_amd import problems

    return problems.poisson2d(1800)  # n = 3.24 M


def _state_path(A, b, sweeps):
    from krylov_amd import _helpers
    from krylov_amd.gmres import _GmresState

    st = _GmresState(_helpers.Problem(A, b, None, None), 30, sweeps)
    st.start()
    st.set_criterion(np.zeros(1 if b.ndim == 1 else b.shape[1]))
    hist, _ = st.run(4)
    assert len(hist) == 4
    return st.path()


@pytest.mark.parametrize("ortho", ["mgs", "mgs2"])
def test_streamed_mgs_matches_launch_per_pass_and_oracle(poisson1800, ortho, monkeypatch):
    import krylov_amd
    from oracle import krylov_ref

    P = poisson1800
    b = np.random.default_rng(11).standard_normal(P.shape[0])
    A = krylov_amd.CsrOperator(P)
    assert _state_path(A, b, 1 if ortho == "mgs" else 2) == (True, 0)
    _, got = krylov_amd.gmres(A, b, ortho=ortho, maxiter=30, tol=0.0)
    monkeypatch.setenv("KRY_MGS_PERSIST", "0")
    A0 = krylov_amd.CsrOperator(P)
    assert _state_path(A0, b, 1 if ortho == "mgs" else 2) == (False, 0)
    _, lpp = krylov_amd.gmres(A0, b, ortho=ortho, maxiter=30, tol=0.0)
    g, l = np.asarray(got.resnorms), np.asarray(lpp.resnorms)
    assert got.numsteps == lpp.numsteps == 30
    np.testing.assert_allclose(g[:-1], l[:-1], rtol=1e-12)
    np.testing.assert_allclose(got.xk, lpp.xk, rtol=0, atol=1e-11 * np.abs(lpp.xk).max())
    if ortho == "mgs":
        _, ref = krylov_ref.gmres(P, b, maxiter=30, tol=0.0)
        np.testing.assert_allclose(g[:-1], np.asarray(ref.resnorms)[:-1], rtol=1e-10)


def test_streamed_mgs_block_columns(monkeypatch):
    """k = 4 columns (n·k = 4 M): the counter-barrier exchange of the
    streamed kernel against the launch-per-pass path."""
    import krylov_amd
    from krylov_amd import problems

    P = problems.poisson2d(1000)
    B = np.random.default_rng(5).standard_normal((P.shape[0], 4))
    A = krylov_amd.CsrOperator(P)
    assert _state_path(A, B, 1) == (True, 0)
    _, got = krylov_amd.gmres(A, B, maxiter=20, tol=0.0)
    monkeypatch.setenv("KRY_MGS_PERSIST", "0")
    _, lpp = krylov_amd.gmres(krylov_amd.CsrOperator(P), B, maxiter=20, tol=0.0)
    np.testing.assert_allclose(np.asarray(got.resnorms)[:-1], np.asarray(lpp.resnorms)[:-1], rtol=1e-12)
    np.testing.assert_allclose(got.xk, lpp.xk, rtol=0, atol=1e-11 * np.abs(lpp.xk).max())


def test_streamed_mgs_timeout_falls_back(poisson1800, monkeypatch):
    """A block that never joins step 2's exchange (KRY_MGS_FAULT): the step
    is rerun launch per pass and the solve matches the clean one."""
    import krylov_amd

    P = poisson1800
    b = np.ones(P.shape[0])
    A = krylov_amd.CsrOperator(P)
    _, clean = krylov_amd.gmres(A, b, maxiter=30, tol=1e-9)
    monkeypatch.setenv("KRY_MGS_FAULT", "2")
    _, faulted = krylov_amd.gmres(A, b, maxiter=30, tol=1e-9)
    assert faulted.numsteps == clean.numsteps
    f, c = np.asarray(faulted.resnorms), np.asarray(clean.resnorms)
    np.testing.assert_allclose(f[:-1], c[:-1], rtol=1e-11)
    np.testing.assert_allclose(faulted.xk, clean.xk, rtol=0, atol=1e-10 * np.abs(clean.xk).max())
    assert _state_path(A, b, 1) == (False, 1)


def test_mgs_partner_two_passes_ahead_is_bitwise(monkeypatch):
    """gm_mgsp3_kernel (k = 1: the partner of pass p + 1 copied into LDS two
    passes ahead, buffer_load ... lds) performs gm_mgsp_kernel's passes and
    sums in the same order: the GMRES history, Hessenberg and iterate are
    bitwise those of KRY_MGS_PF2=0, for mgs and mgs2, and at a size whose
    last block is ragged (the copies' out-of-range rows read 0)."""
    import krylov_amd
    from krylov_amd import problems

    for n, ortho in ((200_000, "mgs"), (200_000, "mgs2"), (123_457, "mgs")):
        R = problems.random_nonsym(n)
        b = np.random.default_rng(3).standard_normal(n)
        monkeypatch.setenv("KRY_MGS_PF2", "1")
        A1 = krylov_amd.CsrOperator(R)
        assert _state_path(A1, b, 1 if ortho == "mgs" else 2) == (True, 0)
        _, i1 = krylov_amd.gmres(A1, b, ortho=ortho, maxiter=30, tol=0.0)
        monkeypatch.setenv("KRY_MGS_PF2", "0")
        _, i0 = krylov_amd.gmres(krylov_amd.CsrOperator(R), b, ortho=ortho, maxiter=30, tol=0.0)
        np.testing.assert_array_equal(np.asarray(i1.resnorms).view(np.uint8), np.asarray(i0.resnorms).view(np.uint8))
        np.testing.assert_array_equal(np.asarray(i1.xk).view(np.uint8), np.asarray(i0.xk).view(np.uint8))


@pytest.mark.parametrize("n", [123_457, 2_100_003])
def test_mgs_partner_two_passes_ahead_is_bitwise_float32(n, monkeypatch):
    """The same in float32 (matrix and right-hand side), where the
    register-resident kernels go up to 32 elements per thread: n = 123,457 is
    ragged at 8 per thread; n = 2,100,003 is past the 2,097,152 that 16 per
    thread cover, so it runs 32 per thread on 129 blocks, the last one holding
    2,851 of its 16,384 elements (3 entries per row keep the matrix quick to
    build)."""
    import krylov_amd
    from krylov_amd import problems

    R = problems.random_nonsym(n, per_row=3).astype(np.float32)
    b = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    monkeypatch.setenv("KRY_MGS_PF2", "1")
    A1 = krylov_amd.CsrOperator(R)
    assert _state_path(A1, b, 1) == (True, 0)
    _, i1 = krylov_amd.gmres(A1, b, maxiter=8, tol=0.0)
    monkeypatch.setenv("KRY_MGS_PF2", "0")
    A0 = krylov_amd.CsrOperator(R)
    assert _state_path(A0, b, 1) == (True, 0)
    _, i0 = krylov_amd.gmres(A0, b, maxiter=8, tol=0.0)
    assert i1.xk.dtype == np.float32 and i1.numsteps == i0.numsteps == 8
    np.testing.assert_array_equal(np.asarray(i1.resnorms).view(np.uint8), np.asarray(i0.resnorms).view(np.uint8))
    np.testing.assert_array_equal(np.asarray(i1.xk).view(np.uint8), np.asarray(i0.xk).view(np.uint8))


@pytest.mark.parametrize("m", [1024, 1025, 1448, 1449])
def test_persistent_mgs_selection_boundaries(m, monkeypatch):
    """The sizes at which the kernel choice changes (float64, one column, 256
    blocks of 512 threads at most): m = 1024, n = 1,048,576, the last size at
    8 elements per thread, a full grid; m = 1025, the first at 16; m = 1448,
    n = 2,096,704, the last register-resident size, its last block ragged;
    m = 1449, n = 2,099,601, the first streamed size (12 granules). Each
    against the launch-per-pass path, to the tolerances of
    test_streamed_mgs_matches_launch_per_pass_and_oracle."""
    import krylov_amd
    from krylov_amd import problems

    P = problems.poisson2d(m)
    assert P.shape[0] == m * m
    b = np.random.default_rng(11).standard_normal(P.shape[0])
    A = krylov_amd.CsrOperator(P)
    assert _state_path(A, b, 1) == (True, 0)
    _, got = krylov_amd.gmres(A, b, maxiter=6, tol=0.0)
    monkeypatch.setenv("KRY_MGS_PERSIST", "0")
    A0 = krylov_amd.CsrOperator(P)
    assert _state_path(A0, b, 1) == (False, 0)
    _, lpp = krylov_amd.gmres(A0, b, maxiter=6, tol=0.0)
    assert got.numsteps == lpp.numsteps == 6
    g, l = np.asarray(got.resnorms), np.asarray(lpp.resnorms)
    print(f"m={m}: max rel resnorm diff {np.max(np.abs(g - l) / np.abs(l)):.3e}, "
          f"max |dx| / max|x| {np.max(np.abs(got.xk - lpp.xk)) / np.abs(lpp.xk).max():.3e}")
    np.testing.assert_allclose(g, l, rtol=1e-12)
    np.testing.assert_allclose(got.xk, lpp.xk, rtol=0, atol=1e-11 * np.abs(lpp.xk).max())
