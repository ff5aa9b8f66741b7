"""The cases of tests/golden/stationary.npz, shared by the script that makes
the fixture from the reference (tests/golden/make_stationary.py) and the tests
that replay them on the device (tests/test_gpu_stationary.py). Inputs are
regenerated from seeds; the fixture stores outputs only.

Each case is (name, solver, make) with make() -> (A, b, kwargs); kwargs may
hold "x0", "M", "inner_weights" (a WeightedInner's weights) and
"eigenvalue_estimates" beside the solver's own keywords.
"""
import numpy as np
import scipy.sparse

STATIONARY = ("richardson", "jacobi", "gauss_seidel", "sor", "ssor")
NSAMPLE = 512       # rows of x stored for n > FULL_X
FULL_X = 1600


def _b(n, cols=None, dtype=np.float64):
    shape = (n,) if cols is None else (n, cols)
    return np.random.default_rng(3).standard_normal(shape).astype(dtype)


def _cheb_bounds():
    return (8 * np.sin(np.pi / 82) ** 2, 8 * np.cos(np.pi / 82) ** 2)


def big_cases(problems):
    P = problems

    def p40():
        return P.poisson2d(40)

    def rnd():
        return P.random_nonsym(5000)

    def case(A, cols=None, dtype=np.float64, **kw):
        def make():
            M = A() if dtype == np.float64 else A().astype(dtype)
            return M, _b(M.shape[0], cols, dtype), dict(kw)

        return make

    def sor_block():
        A = p40()
        x0 = np.random.default_rng(4).standard_normal((A.shape[0], 3))
        return A, _b(A.shape[0], 3), dict(omega=1.8, tol=1e-6, x0=x0, use_callback=True)

    def cheb_m():
        A = p40()
        lo, hi = _cheb_bounds()
        M = scipy.sparse.diags(1.0 / A.diagonal()).tocsr()
        return A, _b(A.shape[0]), dict(eigenvalue_estimates=(lo / 4, hi / 4), M=M, tol=1e-8)

    def cheb_w():
        A = p40()
        w = 10.0 / np.arange(1, A.shape[0] + 1) + 0.5
        return A, _b(A.shape[0]), dict(eigenvalue_estimates=_cheb_bounds(), inner_weights=w, tol=1e-8)

    return [
        ("richardson_p40", "richardson", case(p40, omega=0.2, tol=0.0, maxiter=60)),
        ("jacobi_rand", "jacobi", case(rnd, tol=1e-9, maxiter=400)),
        ("jacobi_p40_block", "jacobi", case(p40, 3, omega=0.9, tol=0.0, maxiter=40)),
        ("gs_rand_lower", "gauss_seidel", case(rnd, tol=1e-9, maxiter=400)),
        ("gs_rand_upper", "gauss_seidel", case(rnd, tol=1e-9, lower=False, maxiter=400)),
        ("gs_p40", "gauss_seidel", case(p40, tol=0.0, maxiter=60)),
        ("sor_p40_lower", "sor", case(p40, omega=1.8, tol=1e-6, maxiter=1000)),
        ("sor_p40_upper", "sor", case(p40, omega=1.8, tol=1e-6, lower=False, maxiter=1000)),
        ("sor_p40_block", "sor", sor_block),
        ("sor_p157", "sor", case(lambda: P.poisson2d(157), omega=1.9, tol=0.0, maxiter=30)),
        ("ssor_p40", "ssor", case(p40, omega=1.8, tol=1e-6, maxiter=1000)),
        ("ssor_rand", "ssor", case(rnd, omega=1.0, tol=1e-9, maxiter=400)),
        ("ssor_perm", "ssor", case(lambda: P.permuted_sym(P.poisson2d(300), 2), omega=1.5, tol=0.0, maxiter=20)),
        ("f32_jacobi", "jacobi", case(p40, dtype=np.float32, tol=0.0, maxiter=50)),
        ("f32_sor", "sor", case(p40, dtype=np.float32, omega=1.5, tol=0.0, maxiter=50)),
        ("cheb_p40", "chebyshev", case(p40, eigenvalue_estimates=_cheb_bounds(), tol=1e-8, maxiter=1000)),
        ("cheb_p40_M", "chebyshev", cheb_m),
        ("cheb_p40_block", "chebyshev", case(p40, 3, eigenvalue_estimates=_cheb_bounds(), tol=1e-8, maxiter=1000)),
        ("cheb_p40_weighted", "chebyshev", cheb_w),
    ]


def small_problems(H):
    """The reference's own small systems (tests/linear_problems.py, restated
    in tests/gpu_helpers.py)."""
    return [H.spd_dense((5,)), H.spd_sparse((5,)), H.spd_dense((5, 1)), H.spd_dense((5, 3)), H.spd_rhs_0((5,)),
            H.spd_rhs_0sol0(), H.symmetric_indefinite(), H.real_unsymmetric()]


def small_cases(H):
    """tests/test_gauss_seidel.py etc. (tol 1e-3, maxiter 10) and
    tests/test_chebyshev.py ((1e-2, 1.75), tol 1e-3, maxiter 100; the first six
    systems) of the reference."""
    out = []
    for solver in STATIONARY:
        for i, (A, b) in enumerate(small_problems(H)):
            out.append((f"{solver}_small{i}", solver, lambda A=A, b=b: (A, b, dict(tol=1.0e-3, maxiter=10))))
    for i, (A, b) in enumerate(small_problems(H)[:6]):
        out.append((f"chebyshev_small{i}", "chebyshev",
                    lambda A=A, b=b: (A, b, dict(eigenvalue_estimates=(1e-2, 1.75), tol=1.0e-3, maxiter=100))))
    return out


def all_cases(problems, H):
    return big_cases(problems) + small_cases(H)


def sample_index(n):
    """The rows of x the fixture stores for n > FULL_X."""
    return np.sort(np.random.default_rng(12345).choice(n, NSAMPLE, replace=False))


def call(mod, solver, A, b, kw, inner_factory=None, callback=None):
    """Call mod.<solver> on a case. inner_factory(w) builds the inner product
    of a weighted case (the reference: a plain callable; the device:
    WeightedInner)."""
    kw = dict(kw)
    w = kw.pop("inner_weights", None)
    use_cb = kw.pop("use_callback", False)
    if w is not None:
        kw["inner"] = inner_factory(w)
    if use_cb and callback is not None:
        kw["callback"] = callback
    fn = getattr(mod, solver)
    if solver == "chebyshev":
        est = kw.pop("eigenvalue_estimates")
        return fn(A, b, est, **kw)
    return fn(A, b, **kw)
