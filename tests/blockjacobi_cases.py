"""Block-Jacobi as sequential loops, the partitions and blocks its tests run
on, and the host model of the preconditioner. Shared by
tests/test_blockjacobi_cases.py (CPU), tests/test_gpu_blockjacobi.py (the
device kernels against these, bitwise) and
tests/golden/make_precond_blockjacobi.py (which runs the reference with the
host model). Plain NumPy / SciPy: nothing here loads the library.
"""
import numpy as np
import scipy.sparse

MAX_BLOCK = 32


def canonical(A, dtype=None):
    S = scipy.sparse.csr_matrix(A, dtype=dtype, copy=True)
    S.sum_duplicates()
    S.sort_indices()
    return S


# ------------------------------------------------------------------ loops
def invert_block_loop(B, dtype, return_piv=False):
    """The inverse of the dense block B by in-place Gauss-Jordan with row
    pivoting in `dtype` scalars: the pivot of column c is the row r >= c with
    the largest |M[r, c]| (a strict comparison: the smallest r among equals),
    true divisions, the product rounded before the subtraction. A zero or
    non-finite pivot raises LinAlgError. Rows are updated as vectors: every
    element sees the same two operations as in the scalar loop."""
    dt = np.dtype(dtype)
    M = np.array(B, dtype=dt, copy=True)
    b = M.shape[0]
    assert M.shape == (b, b)
    piv = np.zeros(b, dtype=np.int64)
    one, zero = dt.type(1), dt.type(0)
    with np.errstate(all="ignore"):
        for c in range(b):
            p, best = c, abs(M[c, c])
            for r in range(c + 1, b):
                a = abs(M[r, c])
                if a > best:
                    p, best = r, a
            if p != c:
                M[[c, p]] = M[[p, c]]
            piv[c] = p
            d = M[c, c]
            if d == 0 or not np.isfinite(d):
                raise np.linalg.LinAlgError(f"singular block: pivot {c} is zero or not finite")
            M[c, c] = one
            M[c, :] = M[c, :] / d
            for r in range(b):
                if r == c:
                    continue
                f = M[r, c]
                M[r, c] = zero
                t = f * M[c, :]  # rounded products
                M[r, :] = M[r, :] - t
        for c in range(b - 1, -1, -1):
            p = piv[c]
            if p != c:
                M[:, [c, p]] = M[:, [p, c]]
    assert M.dtype == dt
    return (M, piv) if return_piv else M


def apply_loop(inverses, starts, x):
    """y = blockdiag(inverses) x: for a block with rows [s, s + b),
    y[s + r, c] = sum_j (X[r, j] * x[s + j, c]) from 0 over j ascending, every
    product rounded before its addition, all b terms. Vectorised over the rows
    (and columns) only. `starts` ends in n."""
    x = np.asarray(x)
    dt = x.dtype
    x2 = x.reshape(x.shape[0], -1)
    y = np.zeros_like(x2)
    with np.errstate(all="ignore"):
        for i, X in enumerate(inverses):
            s, b = int(starts[i]), int(starts[i + 1] - starts[i])
            assert X.shape == (b, b) and X.dtype == dt
            acc = np.zeros((b, x2.shape[1]), dtype=dt)
            for j in range(b):
                p = X[:, j:j + 1] * x2[s + j][None, :]
                acc = acc + p
            y[s:s + b] = acc
    return y.reshape(x.shape)


def uniform_starts(n, b):
    """The starts of blocks of b rows, n closing the last (smaller) one."""
    return np.concatenate([np.arange(0, n, b), [n]]).astype(np.int32)


def extract_blocks(A, starts, dtype):
    """The dense diagonal blocks of A's canonical CSR in `dtype`."""
    S = canonical(A, dtype)
    return [S[int(s):int(e), int(s):int(e)].toarray() for s, e in zip(starts[:-1], starts[1:])]


class HostBlockJacobi:
    """The preconditioner as a reference user writes it: an object with
    ``@``, ``shape`` and ``dtype`` over the two loops."""

    def __init__(self, A, starts, dtype):
        self.shape = A.shape
        self.dtype = np.dtype(dtype)
        self.starts = np.asarray(starts)
        assert self.starts[0] == 0 and self.starts[-1] == A.shape[0]
        self.inverses = [invert_block_loop(B, self.dtype) for B in extract_blocks(A, self.starts, self.dtype)]

    def __matmul__(self, x):
        x = np.asarray(x)
        return apply_loop(self.inverses, self.starts, x.astype(self.dtype, copy=False))


# ----------------------------------------------------------------- blocks
SUITE_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32]


def block_suite(dtype):
    """240 blocks: for every size 10 SPD blocks (G G^T / b + 0.1 I) and 10
    shifted random ones (uniform(-1, 1) + 0.5 I, which need row swaps)."""
    out = []
    for b in SUITE_SIZES:
        for seed in range(10):
            rng = np.random.default_rng(1000 * b + seed)
            G = rng.standard_normal((b, b))
            out.append((f"spd{b}_{seed}", (G @ G.T / b + 0.1 * np.eye(b)).astype(dtype)))
            out.append((f"rnd{b}_{seed}", (rng.uniform(-1.0, 1.0, (b, b)) + 0.5 * np.eye(b)).astype(dtype)))
    return out


def right_residual_ratio(B, X):
    """max_ij |B X - I|_ij / (b eps (|B| |X|)_ij) with the products in extended
    precision; eps of the blocks' dtype."""
    b = B.shape[0]
    eps = float(np.finfo(B.dtype).eps)
    Bl, Xl = B.astype(np.longdouble), X.astype(np.longdouble)
    res = np.abs(Bl @ Xl - np.eye(b, dtype=np.longdouble))
    mag = np.abs(Bl) @ np.abs(Xl)
    return float(np.max(res / (b * eps * mag)))


# ------------------------------------------------------------- partitions
MIXED_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32] * 5


def mixed_starts():
    return np.concatenate([[0], np.cumsum(MIXED_SIZES)]).astype(np.int32)


def mixed_matrix(problems):
    """A random_nonsym matrix of the mixed partition's n = 750 (40 entries per
    row: the blocks are sparse inside), every other block overlaid with a
    half-full standard normal block, so that half of the blocks pivot."""
    starts = mixed_starts()
    n = int(starts[-1])
    A = problems.random_nonsym(n, per_row=40, seed=5).tolil()
    rng = np.random.default_rng(6)
    for i in range(0, len(MIXED_SIZES), 2):
        s, b = int(starts[i]), MIXED_SIZES[i]
        D = rng.standard_normal((b, b)) * (rng.random((b, b)) < 0.5)
        for r, c in zip(*np.nonzero(D)):
            A[s + r, s + c] = A[s + r, s + c] + D[r, c]
    return canonical(A.tocsr(), np.float64), starts


def antidiagonal_block(b, seed=0):
    """A block whose largest entry of column c sits in row b - 1 - c: every
    elimination step swaps rows (but the middle one of an odd b)."""
    rng = np.random.default_rng(seed)
    return 0.1 * rng.uniform(-1.0, 1.0, (b, b)) + np.fliplr(np.diag(rng.uniform(2.0, 3.0, b)))


def kernel_cases(problems):
    """name -> (A, starts): what the factor kernel is held to the loop on."""
    out = {}
    out["mixed"] = mixed_matrix(problems)
    md = problems.multidof(12, 4)
    out["multidof12x4_b4"] = (md, uniform_starts(md.shape[0], 4))
    out["multidof12x4_b5"] = (md, uniform_starts(md.shape[0], 5))
    out["n1"] = (scipy.sparse.csr_matrix(np.array([[3.0]])), np.array([0, 1], dtype=np.int32))
    rn = problems.random_nonsym(300)
    out["b1"] = (rn, uniform_starts(300, 1))
    dense = np.random.default_rng(7).uniform(-1.0, 1.0, (70, 70)) + 2.0 * np.eye(70)
    out["dense70_b32"] = (scipy.sparse.csr_matrix(dense), uniform_starts(70, 32))
    anti = scipy.sparse.block_diag([antidiagonal_block(b, b) for b in (2, 5, 8, 17, 32)], format="csr")
    out["antidiagonal"] = (anti, np.concatenate([[0], np.cumsum([2, 5, 8, 17, 32])]).astype(np.int32))
    return out


# ------------------------------------------------- parity with the reference
# name, solver, slot, problem, block size, right-hand-side columns, keyword
# arguments; b = default_rng(3).standard_normal throughout
CASES = [
    ("cg_md24x4", "cg", "M", "md24x4", 4, 1, {"tol": 1e-8}),
    ("cg_md24x4_k3", "cg", "M", "md24x4", 4, 3, {"tol": 1e-8}),
    ("minres_md16x8", "minres", "M", "md16x8", 8, 1, {"tol": 1e-8}),
    ("gmres30_md24x4ns_mr", "gmres", "Mr", "md24x4ns", 4, 1, {"maxiter": 30}),
    ("bicgstab_r5k_ml", "bicgstab", "Ml", "r5k", 8, 1, {"tol": 1e-8}),
    ("cg_p40_b8", "cg", "M", "p40", 8, 1, {"tol": 1e-8}),
    ("f32_cg_md24x4", "cg", "M", "md24x4_f32", 4, 1, {"tol": 1e-4}),
    # 20 fixed steps: only the residual norms are stored
    ("cg_md12x3_k128", "cg", "M", "md12x3", 3, 128, {"tol": 0.0, "maxiter": 20}),
]


def problem(problems, key, cols):
    if key == "r5k":
        A = problems.random_nonsym(5000)
    elif key == "p40":
        A = problems.poisson2d(40)
    elif key == "md16x8":
        A = problems.multidof(16, 8)
    elif key == "md12x3":
        A = problems.multidof(12, 3)
    elif key == "md24x4ns":
        A = problems.multidof(24, 4, sym=False)
    else:
        A = problems.multidof(24, 4)
    n = A.shape[0]
    b = np.random.default_rng(3).standard_normal(n if cols == 1 else (n, cols))
    if key.endswith("_f32"):
        return A.astype(np.float32), b.astype(np.float32)
    return A, b


def point_jacobi(A):
    """diag(A)^-1 as a matrix: what a device that applied only the diagonal
    would be."""
    return scipy.sparse.diags(1.0 / A.diagonal(), format="csr", dtype=A.dtype)
