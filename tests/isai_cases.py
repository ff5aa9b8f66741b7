"""The incomplete sparse approximate inverse (ISAI) of a triangular factor as
a sequential loop, the matrices its tests run on, and the host model of a
preconditioner that solves its factors with it. Shared by
tests/test_isai_cases.py (CPU), tests/test_gpu_isai.py (the device kernel and
the apply against these) and tests/golden/make_precond_isai.py (which runs the
reference with the host model). Plain NumPy / SciPy: nothing here loads the
library.
"""
import numpy as np
import scipy.sparse

from tests import precond_factored_cases as PC


def isai_lower_loop(T, dtype):
    """W on the pattern of the lower triangle T with (W T) = I on that pattern.
    Row i with pattern J[0..m-1], J[m-1] = i, is the back substitution on
    T(J, J)^T in `dtype` scalars, the stored terms in ascending q, the product
    rounded before the subtraction, true divisions."""
    S = PC.canonical(T, dtype)
    ip, ix, v = S.indptr, S.indices, S.data
    n = S.shape[0]
    one, zero = S.dtype.type(1), S.dtype.type(0)
    out = np.zeros_like(v)
    where = [{int(ix[t]): t for t in range(ip[r], ip[r + 1])} for r in range(n)]
    with np.errstate(all="ignore"):
        for i in range(n):
            b, m = ip[i], ip[i + 1] - ip[i]
            J = [int(c) for c in ix[b:b + m]]
            assert m >= 1 and J[-1] == i and all(J[q] < J[q + 1] for q in range(m - 1))
            w = [None] * m
            w[m - 1] = one / v[b + m - 1]
            for p in range(m - 2, -1, -1):
                s = zero
                for q in range(p + 1, m):
                    t = where[J[q]].get(J[p])
                    if t is not None:
                        prod = v[t] * w[q]  # rounded product
                        s = s - prod
                w[p] = s / v[ip[J[p] + 1] - 1]
            out[b:b + m] = w
    return scipy.sparse.csr_matrix((out, ix.copy(), ip.copy()), shape=S.shape)


def transposed(M):
    T = M.T.tocsr()
    T.sort_indices()
    return T


def isai_loop(T, lower, dtype):
    """isai_lower_loop for a lower T; for an upper one the same on T^T,
    transposed back: the right inverse, (T W) = I on T's pattern."""
    if lower:
        return isai_lower_loop(T, dtype)
    return transposed(isai_lower_loop(transposed(PC.canonical(T, dtype)), dtype))


# ---------------------------------------------------------------- matrices
def triangle(n, lengths, seed=0):
    """A lower triangle whose row i has min(i + 1, lengths[i % len(lengths)])
    entries: the diagonal (magnitude 1 to 2, either sign) and columns drawn
    from [0, i), half of them the nearest ones so that many (J[q], J[p]) are
    stored, values in [-1, 1] / row length."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        m = min(i + 1, lengths[i % len(lengths)])
        near = (m - 1 + 1) // 2
        pick = set(range(i - near, i))
        rest = [c for c in range(i - near)]
        if m - 1 - near > 0:
            pick |= set(int(c) for c in rng.choice(rest, size=m - 1 - near, replace=False))
        assert len(pick) == m - 1
        for c in sorted(pick):
            rows.append(i)
            cols.append(c)
            vals.append(rng.uniform(-1.0, 1.0) / m)
        rows.append(i)
        cols.append(i)
        vals.append(rng.uniform(1.0, 2.0) * (1.0 if rng.random() < 0.7 else -1.0))
    return PC.canonical(scipy.sparse.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr())


def row_lengths(T):
    return np.diff(T.indptr)


def factor_pairs(problems, dtype):
    """name -> (L, U): the triangles the kernel is checked on."""
    p12 = problems.poisson2d(12)
    r3k = problems.random_nonsym(3000)
    out = {}
    for name, A in (("poisson12", p12), ("random3000", r3k), ("arrow300", PC.arrow(300))):
        out["ilu0_" + name] = PC.split_lu(PC.ilu0_loop(A, dtype))
    out["ssor_poisson12"] = PC.ssor_factors(p12, 1.2, dtype)[:2]
    out["ssor_random3000"] = PC.ssor_factors(r3k, 1.2, dtype)[:2]
    return out


def hand_triangles(dtype):
    """name -> lower triangle: rows of exactly 1, 2, 63, 64 and 65 entries
    side by side, n = 1, n = 65 (dense: every length up to 65), and a
    unit-diagonal L."""
    mixed = triangle(200, [1, 2, 63, 64, 65, 3, 17], seed=1)
    assert {1, 2, 63, 64, 65} <= set(int(m) for m in row_lengths(mixed))
    dense65 = triangle(65, [65], seed=2)
    assert row_lengths(dense65)[-1] == 65
    unit = triangle(90, [5, 9, 33], seed=3).tolil()
    unit.setdiag(1.0)
    one = scipy.sparse.csr_matrix(np.array([[3.0]]))
    return {k: PC.canonical(v, dtype)
            for k, v in (("mixed", mixed), ("n1", one), ("n65", dense65), ("unit", unit.tocsr()))}


# ---------------------------------------------- the apply and its bound
def isai_parts(A, spec, dtype, loop=isai_loop):
    """(W_L, W_U, L, U, scale) of SSOR(omega) (spec ("ssor", omega)) or ILU(0)
    (("ilu0",)) of A, the factors by the host loops."""
    if spec[0] == "ssor":
        lo, up, sc = PC.ssor_factors(A, spec[1], dtype)
    else:
        (lo, up), sc = PC.split_lu(PC.ilu0_loop(A, dtype)), None
    return loop(lo, True, dtype), loop(up, False, dtype), lo, up, sc


def stage(W, T, y, sweeps, scale):
    """x = W y, sweeps times x = x + W (y - T x), then x = scale * x."""
    x = W @ y
    for _ in range(sweeps):
        r = y - T @ x
        x = x + W @ r
    if scale is not None:
        x = (x.T * scale).T
    return x


def apply_model(parts, y, sweeps):
    WL, WU, L, U, sc = parts
    return stage(WU, U, stage(WL, L, y, sweeps, sc), sweeps, None)


def _col(v, like):
    return v.reshape((-1,) + (1,) * (like.ndim - 1))


def stage_bound(W, T, y, ey, sweeps, scale, eps):
    """(x, ex): the stage in floating point and a componentwise bound on the
    difference of two floating-point evaluations of it (any summation order,
    no fused operation) whose inputs differ by at most ey. A product M v of
    rows of at most m entries contributes (m + 2) eps |M| |v| (m - 1 additions
    and one multiplication per side are m u each, eps = 2 u covers both sides,
    and two further eps cover the store's own operation on the product), and
    carries its input's difference as |M| ev. The other operand of a store
    that combines (y in y - T x, x in x + W r) adds eps times its magnitude
    and its own difference; the scale multiplies everything by |scale| and
    adds eps |scale| |x|."""
    aW, aT = abs(W), abs(T)
    mW = int(np.diff(W.indptr).max())
    mT = int(np.diff(T.indptr).max())
    x = W @ y
    ex = aW @ ey + (mW + 2) * eps * (aW @ np.abs(y))
    for _ in range(sweeps):
        z = T @ x
        r = y - z
        er = ey + aT @ ex + (mT + 2) * eps * (aT @ np.abs(x)) + eps * np.abs(y)
        d = W @ r
        ex = ex + aW @ er + (mW + 2) * eps * (aW @ np.abs(r)) + eps * np.abs(x)
        x = x + d
    if scale is not None:
        s = _col(np.abs(scale), x)
        ex = s * ex + eps * s * np.abs(x)
        x = (x.T * scale).T
    return x, ex


def apply_bound(parts, y, sweeps):
    """(x, bound) of the whole apply: the lower stage's difference bound is
    the upper stage's input difference."""
    WL, WU, L, U, sc = parts
    eps = float(np.finfo(WL.dtype).eps)
    t, et = stage_bound(WL, L, y, np.zeros_like(y), sweeps, sc, eps)
    return stage_bound(WU, U, t, et, sweeps, None, eps)


class HostIsai:
    """The preconditioner as a reference user writes it: an object with ``@``
    over scipy products with the loops' W (and the factors, for sweeps)."""

    def __init__(self, A, spec, dtype, sweeps=0, loop=isai_loop):
        self.shape = A.shape
        self.dtype = np.dtype(dtype)
        self.parts = isai_parts(A, spec, dtype, loop)
        self.sweeps = sweeps

    def __matmul__(self, x):
        return apply_model(self.parts, np.asarray(x), self.sweeps)


def device_precond(krylov_amd, A, spec, dtype, sweeps=0, ordering="natural"):
    if spec[0] == "ssor":
        return krylov_amd.SsorPreconditioner(A, omega=spec[1], dtype=dtype, solve="isai", sweeps=sweeps,
                                             ordering=ordering)
    return krylov_amd.Ilu0Preconditioner(A, dtype=dtype, solve="isai", sweeps=sweeps, ordering=ordering)


# ------------------------------------------------- parity with the reference
# name, solver, slot, preconditioner spec, sweeps, problem, keyword arguments;
# b = default_rng(3).standard_normal(n) throughout
CASES = [
    ("cg_p40_ssor_isai", "cg", "M", ("ssor", 1.2), 0, "p40", {"tol": 1e-8}),
    ("cg_p40_ilu0_isai_s1", "cg", "M", ("ilu0",), 1, "p40", {"tol": 1e-8}),
    ("minres_p40_ssor_isai", "minres", "M", ("ssor", 1.2), 0, "p40", {"tol": 1e-8}),
    ("gmres30_r5k_mr_isai", "gmres", "Mr", ("ilu0",), 0, "r5k", {"tol": 1e-8, "maxiter": 30}),
    ("bicgstab_r5k_ml_isai", "bicgstab", "Ml", ("ilu0",), 0, "r5k", {"tol": 1e-8}),
    ("f32_cg_p40_ssor_isai", "cg", "M", ("ssor", 1.2), 0, "p40_f32", {"tol": 1e-4}),
]


def problem(problems, key):
    if key == "r5k":
        A = problems.random_nonsym(5000)
    else:
        A = problems.poisson2d(40)
    n = A.shape[0]
    b = np.random.default_rng(3).standard_normal(n)
    if key == "p40_f32":
        return A.astype(np.float32), b.astype(np.float32)
    return A, b
