"""The float32 instantiations of the solver kernels against a float64
reference, ragged tails included (tests/f32_cases.py: the cases, the
reference and the bound; tests/test_f32_cases.py: that the bound has teeth).

Every solve is compared with the oracle run in float64 on the same float32
data. The allowance per history entry is twice the spread of the oracle's own
float32 runs under six valid inner-product orders, 2 eps32 at the least; the
solution is bounded the same way, the final explicit residual of a solve that
stops by 64 eps32 (||b|| + ||A||_1 ||x||). Each test prints the share of the
bound it used and asserts which device path ran."""
import importlib

import numpy as np
import pytest

from tests import f32_cases as F

pytestmark = pytest.mark.gpu

_STATE = {"cg": "_CGState", "gmres": "_GmresState", "minres": "_MinresState"}


def _solve(monkeypatch, cid, **env):
    """Run a case on the device under the given switches -> (info, the
    solver's core state, for its path probes)."""
    import krylov_amd

    solver, A, b, kw = F.build(F.case(cid))
    mod = importlib.import_module(f"krylov_amd.{solver}")
    made = []

    class Recording(getattr(mod, _STATE[solver])):
        def __init__(self, *args):
            super().__init__(*args)
            made.append(self)

    monkeypatch.setattr(mod, _STATE[solver], Recording)
    for name, val in env.items():
        monkeypatch.setenv(name, str(val))
    _, info = getattr(mod, solver)(krylov_amd.CsrOperator(A), b, **kw)
    assert len(made) == 1
    # (pop: the list must not keep the state, whose class closes over the list;
    # the state and its device memory then go when the test returns)
    return info, made.pop()


# ---------------------------------------------------------------------- CG
@pytest.mark.parametrize("cid", F.ids(F.select("cg", k=1, plain=True)))
def test_cg_persistent_loop(cid, monkeypatch):
    """cg_persist_kernel<float, float, ...> with its 32-bit exchange words."""
    info, st = _solve(monkeypatch, cid, KRY_CG_PERSIST=2)
    assert st.path() == (True, 0)
    F.check_device(info, cid)


@pytest.mark.parametrize("cid", F.ids(F.select("cg", k=1, plain=True)))
def test_cg_one_launch_update(cid, monkeypatch):
    """cg_upd_kernel<float, float, NV>: 512 NV 4 elements per block."""
    info, st = _solve(monkeypatch, cid, KRY_CG_PERSIST=0)
    assert st.path() == (False, 0) and st.update_path() == (1, 0)
    F.check_device(info, cid)


@pytest.mark.parametrize("cid", F.ids(F.select("cg", k=1, plain=True)))
def test_cg_separate_passes(cid, monkeypatch):
    """The launch-per-pass kernels with cg_alpha_kernel<float> and
    cg_rho_kernel<float>."""
    info, st = _solve(monkeypatch, cid, KRY_CG_PERSIST=0, KRY_CG_UPD=0)
    assert st.path() == (False, 0) and st.update_path() == (0, 0)
    F.check_device(info, cid)


@pytest.mark.parametrize("D", [0, 3])
@pytest.mark.parametrize("cid", F.ids(F.select("cg", k=(2, 3, 8), plain=True)))
def test_cg_blocks(cid, D, monkeypatch):
    """k = 2 (a row narrower than a lane's four elements), 3 (run as 4) and
    8, with yk updated every step and deferred 3 steps at a time."""
    info, st = _solve(monkeypatch, cid, KRY_CG_YDEFER=D)
    assert st.path() == (False, 0) and st.update_path() == (0, 0) and st.defer_info()[0] == D
    F.check_device(info, cid)


def test_cg_float32_jacobi(monkeypatch):
    info, st = _solve(monkeypatch, "cg_M_band4099_k1")
    assert st.path() == (False, 0) and st.update_path() == (0, 0)
    F.check_device(info, "cg_M_band4099_k1")


# ------------------------------------------------------------------- GMRES
@pytest.mark.parametrize("cid", F.ids(F.select("gmres", plain=True)))
def test_gmres_persistent_mgs(cid, monkeypatch):
    """gm_mgsp3_kernel<float, 8> at k = 1, gm_mgsp_kernel<float, 8> at k = 2,
    4 (k = 3) and 8."""
    info, st = _solve(monkeypatch, cid)
    assert st.path() == (True, 0)
    F.check_device(info, cid)


@pytest.mark.parametrize("cid", F.ids(F.select("gmres", k=(1, 2), plain=True)))
def test_gmres_pass_kernels(cid, monkeypatch):
    info, st = _solve(monkeypatch, cid, KRY_MGS_PERSIST=0)
    assert st.path() == (False, 0)
    F.check_device(info, cid)


@pytest.mark.parametrize("cid", [c[0] for c in F.select("gmres", plain=False) if "ortho" in c[4]])
def test_gmres_mgs2_and_householder(cid, monkeypatch):
    info, st = _solve(monkeypatch, cid)
    assert st.path() == ("mgs2" in cid, 0)
    F.check_device(info, cid)


def test_gmres_float32_right_preconditioner(monkeypatch):
    """Mr: the MGS runs launch per pass (the persistent kernel fuses the
    norm, which a preconditioned step does not take)."""
    info, st = _solve(monkeypatch, "gmres_Mr_nonsym4099_k1")
    assert st.path() == (False, 0)
    F.check_device(info, "gmres_Mr_nonsym4099_k1")


@pytest.mark.parametrize("cid", F.ids(F.LARGE))
def test_gmres_float_kernel_bands(cid, monkeypatch):
    """The sizes at which the float kernel choice changes (256 blocks x 512
    threads x E): poisson2d(1449), the first size at E = 32, the float-only
    kernel, its last block ragged; poisson2d(2048), the last at E = 32, a full
    grid; poisson2d(2049), the first on the streamed gm_mgsl_kernel<float, 12>,
    n mod 4 = 1. The envelope is of the pairwise and f64acc variants."""
    try:
        info, st = _solve(monkeypatch, cid)
        assert st.path() == (True, 0)
        F.check_device(info, cid)
    finally:
        F.release_large()


# ------------------------------------------------------------------ MINRES
@pytest.mark.parametrize("cid", F.ids(F.select("minres")))
def test_minres_float32_vectors(cid, monkeypatch):
    """Unweighted float32: every step kernel runs as <float, float>, and the
    one-launch tail, float64 only, is not taken. SPD and indefinite, k = 1, 2,
    3 and 8, the DIA image, and M."""
    info, st = _solve(monkeypatch, cid)
    assert st.update_path() == (False, 0)
    F.check_device(info, cid)


# ------------------------------------------------------- stop at tolerance
@pytest.mark.parametrize("cid", F.ids(F.STOP))
def test_stop_at_tolerance(cid, monkeypatch):
    """tol = 1e-4: numsteps and success are the oracle's (every variant of
    which stops at this step, 1 % clear of the criterion), the explicit
    residual within 64 eps32 (||b|| + ||A||_1 ||x||)."""
    info, _ = _solve(monkeypatch, cid)
    assert info.success
    F.check_device(info, cid)


# --------------------------------------------------------- single-call ops
_SHAPES = [(1, 1), (2, 1), (3, 1), (5, 1), (1023, 1), (1025, 1), (1027, 1), (1027, 2), (1027, 4), (100003, 1)]


@pytest.mark.parametrize("n,k", _SHAPES)
def test_dot_and_axpy_float32(n, k):
    """kry_dot, plain and weighted, within 2 eps32 of sum |x_i y_i| of the
    float64 einsum of the float32 data; kry_axpy bitwise NumPy's float32
    y + alpha * x."""
    from krylov_amd import _lib
    from krylov_amd.device import DeviceVector, get_context

    ctx = get_context()
    rng = np.random.default_rng([n, k])
    x = rng.standard_normal((n, k)).astype(np.float32)
    y = rng.standard_normal((n, k)).astype(np.float32)
    x[-1], y[-1] = 100.0, 100.0  # the last element carries the sum
    w = rng.uniform(1, 2, n)
    xv, yv = DeviceVector.from_host(ctx, x), DeviceVector.from_host(ctx, y)
    assert xv.dtype == np.float32
    wv = DeviceVector.from_host(ctx, w[:, None])
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    worst = 0.0
    for wdev, wy in ((None, y64), (wv, w[:, None] * y64)):
        out = np.zeros(k)
        _lib.check(_lib.lib.kry_dot(ctx.handle, xv.handle, yv.handle, wdev.handle if wdev else None, _lib.dptr(out)))
        want = np.einsum("ij,ij->j", x64, wy)
        scale = np.einsum("ij,ij->j", np.abs(x64), np.abs(wy))
        worst = max(worst, float(np.max(np.abs(out - want) / (2.0 * F.EPS32 * scale))))
    print(f"kry_dot float32 ({n}, {k}): dev/bound {worst:.3g}")
    assert worst <= 1.0
    alpha = rng.standard_normal(k).astype(np.float32)
    _lib.check(_lib.lib.kry_axpy(ctx.handle, _lib.dptr(alpha.astype(np.float64)), xv.handle, yv.handle))
    got = yv.to_host()
    want = y + alpha * x
    assert got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", [1, 10, 1027, 5000])
def test_householder_float32(n):
    """Householder(x) and H @ y for float32 x against the oracle's _House on
    the same data in float64: v within 4 eps32 of ||v||_inf, H @ y within
    4 eps32 of ||y||_inf; alpha, beta and xnorm come out in float32."""
    import krylov_amd
    from oracle import krylov_ref

    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    x[-1] = 100.0
    y = rng.standard_normal(n).astype(np.float32)
    H = krylov_amd.Householder(x)
    R = krylov_ref._House(x.astype(np.float64))
    assert H.v.dtype == np.float32 and H.v.shape == x.shape
    assert isinstance(H.alpha, np.float32) and isinstance(H.xnorm, np.float32)
    assert float(H.alpha) == float(R.alpha) and float(H.beta) == float(R.beta)
    assert (H.beta == 0 and n == 1) or isinstance(H.beta, np.float32)
    xnorm = np.linalg.norm(x.astype(np.float64))
    assert abs(float(H.xnorm) - xnorm) <= 2.0 * F.EPS32 * xnorm
    dv = float(np.max(np.abs(H.v.astype(np.float64) - R.v)) / (4.0 * F.EPS32 * np.max(np.abs(R.v))))
    got, want = H @ y, R @ y.astype(np.float64)
    assert got.dtype == np.float32
    dy = float(np.max(np.abs(got.astype(np.float64) - want)) / (4.0 * F.EPS32 * np.max(np.abs(y))))
    print(f"Householder float32 n={n}: v dev/bound {dv:.3g}, H @ y dev/bound {dy:.3g}")
    assert dv <= 1.0 and dy <= 1.0
