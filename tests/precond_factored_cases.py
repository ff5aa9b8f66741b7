"""Cases and host models of the factorised preconditioners (SSOR, ILU(0)),
shared by tests/golden/make_precond_factored.py (which runs the reference
with the host models) and tests/test_gpu_ilu0.py /
tests/test_gpu_precond_factored.py (which run the device objects on the same
regenerated inputs). Plain NumPy / SciPy: nothing here loads the library.
"""
import numpy as np
import scipy.linalg
import scipy.sparse
from scipy.sparse.linalg import spsolve_triangular


def canonical(A, dtype=None):
    S = scipy.sparse.csr_matrix(A, dtype=dtype, copy=True)
    S.sum_duplicates()
    S.sort_indices()
    return S


def arrow(n=300):
    """Tridiagonal plus a dense last row and last column: diagonal 4, every
    other entry -1/n (row sums of magnitudes < 4: diagonally dominant). The
    last row has n entries and each of its pivots was updated by another step
    of the same row."""
    A = scipy.sparse.lil_matrix((n, n))
    off = -1.0 / n
    for i in range(n):
        A[i, i] = 4.0
        if i > 0:
            A[i, i - 1] = off
        if i + 1 < n:
            A[i, i + 1] = off
    A[n - 1, :] = off
    A[:, n - 1] = off
    A[n - 1, n - 1] = 4.0
    return canonical(A.tocsr())


def ilu0_loop(A, dtype):
    """The sequential ILU(0) loop in `dtype` scalars, the product rounded
    before the subtraction: the factorised values on A's canonical pattern."""
    S = canonical(A, dtype)
    ip, ix = S.indptr, S.indices
    v = S.data.copy()
    n = S.shape[0]
    diag = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        for t in range(ip[i], ip[i + 1]):
            if ix[t] == i:
                diag[i] = t
    assert np.all(diag >= 0)
    with np.errstate(all="ignore"):
        for i in range(n):
            pos = {int(ix[t]): t for t in range(ip[i], ip[i + 1])}
            for t in range(ip[i], diag[i]):
                k = int(ix[t])
                lik = v[t] / v[diag[k]]  # dtype scalars: one rounding
                v[t] = lik
                for f in range(diag[k] + 1, ip[k + 1]):
                    te = pos.get(int(ix[f]))
                    if te is not None:
                        p = lik * v[f]  # rounded product
                        v[te] = v[te] - p
    return scipy.sparse.csr_matrix((v, ix.copy(), ip.copy()), shape=S.shape)


def split_lu(F):
    """(L, U) of factorised values F on A's pattern: L = strict lower part
    with a stored unit diagonal, U = the upper part with the diagonal."""
    n = F.shape[0]
    rows = np.repeat(np.arange(n), np.diff(F.indptr))
    low = F.indices < rows
    eye = np.arange(n)
    L = scipy.sparse.coo_matrix((np.concatenate([F.data[low], np.ones(n, dtype=F.dtype)]),
                                 (np.concatenate([rows[low], eye]), np.concatenate([F.indices[low], eye]))),
                                shape=F.shape).tocsr()
    U = scipy.sparse.coo_matrix((F.data[~low], (rows[~low], F.indices[~low])), shape=F.shape).tocsr()
    L.sort_indices()
    U.sort_indices()
    return L, U


def ssor_factors(A, omega, dtype):
    """(D/omega + L, D/omega + U, D (2 - omega)/omega) in `dtype`."""
    S = canonical(A, dtype)
    dt = np.dtype(dtype)
    d = S.diagonal()
    dw = scipy.sparse.diags((d / dt.type(omega)).astype(dt), format="csr", dtype=dt)
    lo = (scipy.sparse.tril(S, -1) + dw).tocsr().astype(dt)
    up = (scipy.sparse.triu(S, 1) + dw).tocsr().astype(dt)
    return lo, up, (d * dt.type((2 - omega) / omega)).astype(dt)


class HostPrecond:
    """A preconditioner as the reference's users write one: an object with
    ``@`` over scipy triangular solves. stages: ("tri", T, lower) or
    ("scale", d). dense=True solves through scipy.linalg.solve_triangular on
    the same factors (the spread variant)."""

    def __init__(self, n, dtype, stages, dense=False):
        self.shape = (n, n)
        self.dtype = np.dtype(dtype)
        self.stages = [(s[0], s[1].toarray(), s[2]) if (dense and s[0] == "tri") else s for s in stages]
        self.dense = dense

    def __matmul__(self, x):
        y = np.asarray(x)
        for s in self.stages:
            if s[0] == "scale":
                y = (y.T * s[1]).T
            elif self.dense:
                y = scipy.linalg.solve_triangular(s[1], y, lower=s[2])
            else:
                y = spsolve_triangular(s[1], y, lower=s[2])
        return y


def host_precond(A, spec, dtype, dense=False):
    n = A.shape[0]
    if spec[0] == "ssor":
        lo, up, sc = ssor_factors(A, spec[1], dtype)
        return HostPrecond(n, dtype, [("tri", lo, True), ("scale", sc), ("tri", up, False)], dense)
    L, U = split_lu(ilu0_loop(A, dtype))
    return HostPrecond(n, dtype, [("tri", L, True), ("tri", U, False)], dense)


def device_precond(krylov_amd, A, spec, dtype):
    if spec[0] == "ssor":
        return krylov_amd.SsorPreconditioner(A, omega=spec[1], dtype=dtype)
    return krylov_amd.Ilu0Preconditioner(A, dtype=dtype)


def slot_matrix(A, tag):
    """A matrix preconditioner named by a tag in a case's keyword arguments:
    ("jacobi",) = diag(1 / diag(A)), ("scaled_eye", c) = c I; scipy sparse."""
    n = A.shape[0]
    if tag[0] == "jacobi":
        return scipy.sparse.diags(1.0 / A.diagonal(), format="csr")
    if tag[0] == "scaled_eye":
        return (tag[1] * scipy.sparse.identity(n, dtype=A.dtype)).tocsr()
    raise ValueError(f"unknown matrix tag {tag!r}")


# name, solver, slot, preconditioner spec, problem, keyword arguments; a tuple
# under "M" / "Ml" / "Mr" there names a matrix for that other slot (slot_matrix)
CASES = [
    ("cg_p40_ssor", "cg", "M", ("ssor", 1.2), "p40", {"tol": 1e-8}),
    ("cg_p40_ilu0", "cg", "M", ("ilu0",), "p40", {"tol": 1e-8}),
    ("cg_p40_ssor_block", "cg", "M", ("ssor", 1.0), "p40_block", {"tol": 1e-8}),
    ("cg_p40_ml", "cg", "Ml", ("ssor", 1.0), "p40", {"tol": 0.0, "maxiter": 15}),
    ("minres_p40_ssor", "minres", "M", ("ssor", 1.2), "p40", {"tol": 1e-8}),
    ("gmres_r3k_mr", "gmres", "Mr", ("ilu0",), "r3k", {"tol": 1e-10, "maxiter": 40}),
    ("gmres_r3k_ml", "gmres", "Ml", ("ilu0",), "r3k", {"tol": 1e-10, "maxiter": 40}),
    ("gmres_r3k_m_mgs2", "gmres", "M", ("ssor", 1.0), "p40", {"tol": 0.0, "maxiter": 20, "ortho": "mgs2"}),
    ("bicgstab_r3k_mr", "bicgstab", "Mr", ("ilu0",), "r3k", {"tol": 1e-10, "maxiter": 60}),
    ("cgs_r3k_m", "cgs", "M", ("ilu0",), "r3k", {"tol": 1e-10, "maxiter": 60}),
    ("cheb_p40_ssor", "chebyshev", "M", ("ssor", 1.0), "p40", {"tol": 0.0, "maxiter": 30}),
    ("f32_cg_p40_ssor", "cg", "M", ("ssor", 1.0), "p40_f32", {"tol": 1e-4}),
    # a factorised object and a matrix in one solve
    ("gmres_r3k_ml_fac_mr_mat", "gmres", "Ml", ("ilu0",), "r3k", {"Mr": ("jacobi",), "tol": 0.0, "maxiter": 25}),
    ("gmres_p40_m_fac_mr_mat", "gmres", "M", ("ssor", 1.0), "p40", {"Mr": ("jacobi",), "tol": 0.0, "maxiter": 20}),
    ("cg_p40_m_mat_ml_fac", "cg", "Ml", ("ssor", 1.0), "p40", {"M": ("jacobi",), "tol": 0.0, "maxiter": 15}),
    ("minres_p40_m_fac_ml_mr_mat", "minres", "M", ("ssor", 1.0), "p40",
     {"Ml": ("scaled_eye", 0.5), "Mr": ("scaled_eye", 0.5), "tol": 0.0, "maxiter": 20}),
]


def problem(problems, key):
    """(A, b) of a case, regenerated from krylov_amd.problems."""
    if key == "r3k":
        A = problems.random_nonsym(3000, 6, 2.0, 0)
        return A, np.ones(A.shape[0])
    A = problems.poisson2d(40)
    n = A.shape[0]
    if key == "p40_block":
        return A, np.random.default_rng(1).standard_normal((n, 3))
    if key == "p40_f32":
        return A.astype(np.float32), np.ones(n, dtype=np.float32)
    return A, np.ones(n)


def call(mod, solver, A, b, slot, P, kw, eigs=None, **extra):
    """mod.<solver>(A, b, ..., <slot>=P, **kw), the matrix tags in kw resolved."""
    kw = dict(kw, **extra)
    for nm in ("M", "Ml", "Mr"):
        if isinstance(kw.get(nm), tuple):
            kw[nm] = slot_matrix(A, kw[nm])
    kw[slot] = P
    if solver == "chebyshev":
        return mod.chebyshev(A, b, eigs, **kw)
    return getattr(mod, solver)(A, b, **kw)
