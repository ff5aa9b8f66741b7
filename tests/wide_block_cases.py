"""Inputs and the comparison rule of the tests at 32 to 256 right-hand-side
columns (tests/test_gpu_wide_blocks.py on the device,
tests/test_wide_block_cases.py on the host). Everything is rebuilt from seeds;
every expected value is computed in the tests by SciPy or oracle/krylov_ref.py.

The SpMV side: launch_spmv sends k = 4..64 to the lane-group kernel and
k = 128, 256 to spmv_sell_kernel with nch = k / 8 column groups, on a grid
that launch_sell_img rounds up to a multiple of 8 blocks and caps at
MAX_GRID; sell_geometry() restates that arithmetic so that the host tests can
show which shape reaches which rule.

The solver side: one block of right-hand sides per (matrix, k), its first
four columns special (block()), and one rule for comparing a history with the
oracle's (classes(), assert_cap(), history_deviation())."""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg

from krylov_amd import problems
from tests import solver_cases

# ------------------------------------------------------------------- SpMV
KT = 8            # columns per lane of spmv_sell_kernel at k > 8
MAX_GRID = 8192   # kMaxGrid
WIDE = (128, 256)  # the widths that run spmv_sell_kernel with column groups
STRUCTURED_WIDTHS = (16, 32, 64, 128, 256)
ODD_WIDTHS = (33, 129)
# rows of the banded matrices: 1, 2 and 38 slices as the widths' smallest
# shapes, and 37 slices, an odd count above one, where (waves + 3) / 4 = 148 is
# no multiple of 8 at k = 128
BANDED_ROWS = (1, 65, 64 * 36 + 5, 64 * 37 + 5)
# (n, k, dtype): nslices * nch = 1094 * 32 = 2188 * 16 = 35008 > 4 * MAX_GRID
GRID_CAP_SHAPES = ((70_001, 256, np.float64), (140_003, 128, np.float32))


def sell_geometry(n, k):
    """launch_sell_img and the head of spmv_sell_kernel for n rows at k = 128
    or 256: {"nslices", "nch", "grid", "rounded" (the multiple-of-8 rule
    changed the grid), "capped", "per_group" (waves per column group),
    "empty" (waves whose slice range is empty), "widest" (slices of the
    longest range)}."""
    assert k in WIDE
    nslices = (n + 63) // 64
    nch = k // KT
    waves = nslices * nch
    grid0 = max(1, min(MAX_GRID, (waves + 3) // 4))
    grid = min(MAX_GRID, (grid0 + 7) // 8 * 8)
    assert 4 * grid % nch == 0
    W = 4 * grid // nch
    spans = [nslices * (m + 1) // W - nslices * m // W for m in range(W)]
    assert sum(spans) == nslices
    return {"nslices": nslices, "nch": nch, "grid": grid, "rounded": grid != grid0,
            "capped": (waves + 3) // 4 > MAX_GRID, "per_group": W, "empty": spans.count(0), "widest": max(spans)}


def banded(n, seed, dtype=np.float64):
    """Rows of 0 to 16 sorted, distinct entries within 400 columns of the
    diagonal (16 offsets drawn once, each row keeping a random share of
    them), standard normal values; slice 1 (if there is one) is empty and
    slice 2 keeps every offset that stays inside the matrix: a matrix like the
    one of test_sell64_k1_regular_compact_bitwise at any n, assembled without
    a loop over the rows."""
    rng = np.random.default_rng(seed)
    offs = np.sort(rng.choice(np.arange(-400, 401), 16, replace=False))
    keep = rng.random((n, 16)) < rng.random((n, 1))
    keep[64:128] = False
    keep[128:192] = True
    cols = np.arange(n)[:, None] + offs[None, :]
    keep &= (cols >= 0) & (cols < n)
    lens = keep.sum(axis=1)
    indptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=indptr[1:])
    indices = cols[keep].astype(np.int32)
    data = rng.standard_normal(indices.shape[0]).astype(dtype)
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def wide_x(n, k, dtype, seed):
    """An (n, k) block at magnitudes 1e-20..1e20 (1e-8..1e8 in float32)."""
    rng = np.random.default_rng(seed)
    e = 20 if np.dtype(dtype) == np.float64 else 8
    return (rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-e, e, (n, k))).astype(dtype)


def structured(name):
    return {"stencil15_3d_12": lambda: problems.stencil15_3d(12), "poisson2d_61": lambda: problems.poisson2d(61)}[name]()


STRUCTURED = ("stencil15_3d_12", "poisson2d_61")


# ---------------------------------------------------------------- the block
def poisson_eigvec(m):
    """kron(v, v), v_i = sin(pi i / (m + 1)): the eigenvector of poisson2d(m)
    to its smallest eigenvalue."""
    v = np.sin(np.pi * np.arange(1, m + 1) / (m + 1))
    return np.kron(v, v)


def _rayleigh_iteration(A, sweeps=8):
    """Rayleigh quotient iteration on a symmetric A from a seeded start and
    shift 0: cubic convergence to some eigenpair."""
    n = A.shape[0]
    eye = sp.identity(n, format="csc")
    v = np.random.default_rng(0).standard_normal(n)
    v /= np.linalg.norm(v)
    sigma = 0.0
    for _ in range(sweeps):
        u = scipy.sparse.linalg.splu((A - sigma * eye).tocsc()).solve(v)
        if not np.all(np.isfinite(u)):  # the shift is an eigenvalue to the last bit
            break
        v = u / np.linalg.norm(u)
        sigma = v @ (A @ v)
    return v


# next to a simple real eigenvalue of problems.random_nonsym(3000, seed=4)
# (it has about 40 real ones; scipy.sparse.linalg.eigs around 0.8 gave this one)
R_REAL_EIGENVALUE = 0.80981770341


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> (A, an eigenvector of A), by name: "poisson<m>";
    "poisson<m>_shift_w" = diag(1 / w) (poisson2d(m) + the diagonal shift of
    Pvar) with w = weights(n), self-adjoint in the inner product of those
    weights; "Pvar" and "R" of solver_cases.inputs() (R =
    problems.random_nonsym(3000, seed=4)); "diag40"."""
    if name == "diag40":
        return sp.diags(np.arange(1.0, 41.0)).tocsr(), np.eye(40)[:, 0]
    if name == "R":
        # (a dense factorisation: the sparse one of a random pattern fills in
        # and takes ten times as long)
        A = solver_cases.inputs()[name]
        lu = scipy.linalg.lu_factor(A.toarray() - R_REAL_EIGENVALUE * np.eye(A.shape[0]))
        v = np.random.default_rng(0).standard_normal(A.shape[0])
        for _ in range(3):
            v = scipy.linalg.lu_solve(lu, v)
            v /= np.linalg.norm(v)
        return A, v
    if name == "Pvar":
        A = solver_cases.inputs()[name]
        return A, _rayleigh_iteration(A)
    assert name.startswith("poisson")
    m = int(name[7:].split("_")[0])
    P = problems.poisson2d(m)
    if "_shift" in name:  # the diagonal that solver_cases.inputs() adds for Pvar
        P = (P + sp.diags(np.random.default_rng(7).uniform(0.0, 2.0, P.shape[0]))).tocsr()
    if name.endswith("_w"):
        # W^-1 P is similar to the symmetric W^-1/2 P W^-1/2: an eigenvector u
        # of that gives the eigenvector W^-1/2 u
        s = sp.diags(1.0 / np.sqrt(weights(P.shape[0])))
        u = _rayleigh_iteration((s @ P @ s).tocsr())
        A = (sp.diags(1.0 / weights(P.shape[0])) @ P).tocsr()
        A.sort_indices()
        return A, s @ u
    return P, poisson_eigvec(m)


def block(name, k, seed=0):
    """The (n, k) right-hand side of a case: column 0 an eigenvector of the
    matrix (it converges at step 1 while the others run on), column 1 zero,
    column 2 scaled by 1e-12, column 3 by 1e12, the others standard normal."""
    A, v = matrix(name)
    n = A.shape[0]
    B = np.random.default_rng([seed, k, n]).standard_normal((n, k))
    B[:, 0] = v
    B[:, 1] = 0.0
    B[:, 2] *= 1e-12
    B[:, 3] *= 1e12
    return B


def unit_block(n=40, k=32):
    """Column c a multiple of unit vector 1 + c: with A = diag(1..n) every
    column's Krylov space is invariant at step 1."""
    B = np.zeros((n, k))
    B[1 + np.arange(k), np.arange(k)] = np.random.default_rng(3).uniform(0.5, 2.0, k)
    return B


# -------------------------------------------------------------------- cases
# (id, solver, matrix, k, keyword arguments); M / Ml / Mr name entries of
# solver_cases.inputs(), inner = "w" is WeightedInner(uniform(1, 2, n), seed 12)
CASES = []
for _s in ("cg", "minres"):
    for _k in (32, 33, 64, 128, 129, 256):
        CASES.append((f"{_s}_poisson29_k{_k}", _s, "poisson29", _k, dict(tol=1e-8)))
for _o in ("mgs", "mgs2"):
    for _k in (32, 128, 256):
        CASES.append((f"gmres_{_o}_R_k{_k}", "gmres", "R", _k, dict(ortho=_o, tol=0.0, maxiter=30)))
CASES += [
    # n k = 2.56 M: past the register-resident MGS kernels, on the streamed one
    ("gmres_poisson100_k256", "gmres", "poisson100", 256, dict(tol=0.0, maxiter=8)),
    # 70 steps: gm_trsv_big_kernel inside a solve
    ("gmres_poisson29_k32_m70", "gmres", "poisson29", 32, dict(tol=0.0, maxiter=70)),
    ("cg_M_Ml_Pvar_k128", "cg", "Pvar", 128, dict(M="Mj", Ml="S", tol=1e-8)),
    ("gmres_all_R_k128", "gmres", "R", 128, dict(M="RMabs", Ml="RMj", Mr="RMj", tol=0.0, maxiter=30)),
    ("minres_M_Pvar_k256", "minres", "Pvar", 256, dict(M="Mj", tol=1e-8)),
    # CG and MINRES need an operator that is self-adjoint in the inner product:
    # poisson2d(29) itself is not in the weighted one (MINRES then stalls and
    # misses the cap), so the rows are scaled by 1 / w. With that alone the
    # solves take 115 steps on a spectrum of 841 distinct eigenvalues, and from
    # step 60 on the oracle's block and single-column histories drift apart by
    # up to 0.1 (the Lanczos recurrence losing orthogonality): no tolerance
    # holds there. The diagonal shift of Pvar brings the solves to 1e-8 within
    # 40 steps, where the oracle's own noise stays below 1e-13.
    ("cg_w_poisson29_k128", "cg", "poisson29_shift_w", 128, dict(inner="w", tol=1e-8)),
    ("minres_w_poisson29_k128", "minres", "poisson29_shift_w", 128, dict(inner="w", tol=1e-8)),
    ("gmres_w_R_k128", "gmres", "R", 128, dict(inner="w", tol=0.0, maxiter=20)),
]
del _s, _k, _o
# the GMRES cases without preconditioner or weights: the persistent MGS kernel
# runs, and the solve is repeated launch per pass (KRY_MGS_PERSIST=0)
PERSISTENT = tuple(c[0] for c in CASES if c[1] == "gmres" and not set(c[4]) & {"M", "Ml", "Mr", "inner"})
STREAMED = ("gmres_poisson100_k256",)
# factorised preconditioners take 64 columns at most
FACTORED_CASES = (("cg_ssor_poisson12_k64", ("ssor", 1.2)), ("cg_ilu0_poisson12_k64", ("ilu0",)))


def case(cid):
    return next(c for c in CASES if c[0] == cid)


def weights(n):
    return np.random.default_rng(12).uniform(1.0, 2.0, n)


def build(c, inner_of=None):
    """-> (solver name, A, B, keyword arguments) of a case, the named
    matrices substituted; inner_of maps the weights to the inner product."""
    _, solver, name, k, kw = c
    A, _ = matrix(name)
    q = solver_cases.inputs() if set(kw) & {"M", "Ml", "Mr"} else {}
    out = {}
    for key, val in kw.items():
        if key in ("M", "Ml", "Mr"):
            val = q[val]
        elif key == "inner":
            val = inner_of(weights(A.shape[0]))
        out[key] = val
    return solver, A, block(name, k), out


def host_inner(w):
    """The reference's custom inner product (tests/test_solvers.py:157-161)
    for blocks, for the oracle."""
    def inner(x, y):
        wy = w.reshape((-1,) + (1,) * (y.ndim - 1)) * y
        return np.einsum("i...,i...->...", x, wy)

    return inner


# ------------------------------------------------------ the comparison rule
# A history entry of column c is compared relatively while the oracle's value
# is at least REDUCTION times the column's initial residual (strict class);
# below that (the eigenvector column after step 1, the tail of a column that
# finishes early) the updated residual is rounding noise of the recurrence on
# both sides and only its size is bounded (floor class).
#
# RTOL is the project's contract for histories (tests/gpu_helpers.py). What it
# rests on here: the oracle's block run against its own single-column runs of
# the same columns, which differ in the summation grouping alone, agree to
# within 7.8e-14 relative over the strict class of the k = 128 cases (measured
# and printed by tests/test_wide_block_cases.py, which asserts it below
# NOISE_BOUND): RTOL keeps more than two orders of magnitude over the
# reference's own noise. On the device the largest deviation over all cases
# was 3.3 % of RTOL (minres_poisson29_k64).
RTOL = 1e-10
REDUCTION = 1e-8
FLOOR_FACTOR = 2.0      # floor class: got < FLOOR_FACTOR * REDUCTION * r0
STRICT_SHARE = 0.9      # of the ordinary columns' entries, in every case
NOISE_BOUND = 1e-11
SPECIAL = 4             # columns 0..3 of block()


def history(info):
    """resnorms as a (steps + 1, k) float64 array."""
    return np.asarray(info.resnorms, dtype=np.float64)


def classes(want):
    """-> (strict, floor) masks over want[:-1] (the last entry, the explicit
    residual when the solve succeeded, is compared on its own)."""
    h = want[:-1]
    strict = (h >= REDUCTION * want[0]) & (want[0] > 0.0)
    return strict, ~strict


def assert_cap(want):
    """The floor class may not swallow a case: over the ordinary columns the
    strict class holds at least STRICT_SHARE of the entries, column 0 starts
    in it, and column 1 is zero throughout."""
    strict, _ = classes(want)
    assert strict.shape[0] >= 1 and strict.shape[1] > SPECIAL
    share = strict[:, 2:].mean()
    assert share >= STRICT_SHARE, share
    assert strict[0, 0] and want[0, 0] > 0.0
    assert np.all(want[:, 1] == 0.0)
    return float(share)


def history_deviation(got, want):
    """Assert the rule on a history and return the largest strict-class
    deviation as a fraction of RTOL."""
    assert got.shape == want.shape, (got.shape, want.shape)
    strict, floor = classes(want)
    g, w = got[:-1], want[:-1]
    r0 = np.broadcast_to(want[0], w.shape)
    assert np.all(got[:, 1] == 0.0) and np.all(want[:, 1] == 0.0)
    assert np.all(np.isfinite(g))
    # (column 1 is in the floor class with r0 = 0: it is exactly zero, above)
    cols = np.ones(w.shape[1], dtype=bool)
    cols[1] = False
    fl = floor & cols
    assert np.all(g[fl] < FLOOR_FACTOR * REDUCTION * r0[fl]), float(np.max(g[fl] / r0[fl]))
    if not strict.any():
        return 0.0
    rel = np.abs(g[strict] - w[strict]) / w[strict]
    worst = float(rel.max() / RTOL)
    assert worst <= 1.0, (worst, np.argwhere(strict)[int(np.argmax(rel))].tolist())
    return worst


def assert_final_and_x(got_info, want_info):
    """The last history entry and xk, as tests/gpu_helpers.assert_parity
    compares them (1e-12 of the largest initial residual; 1e-9 of max |x|),
    and the same per column, so that the column scaled by 1e12 does not hide
    the others: entry within 1e-12 r0 + RTOL times itself, xk within 1e-9 of
    the column's largest entry. The zero column's xk is exactly zero."""
    g, w = history(got_info), history(want_info)
    assert np.all(np.abs(g[-1] - w[-1]) <= 1e-12 * np.max(w[0]) + 1e-300)
    assert np.all(np.abs(g[-1] - w[-1]) <= 1e-12 * w[0] + RTOL * w[-1])
    xg, xw = np.asarray(got_info.xk), np.asarray(want_info.xk)
    assert xg.shape == xw.shape and xg.dtype == xw.dtype
    np.testing.assert_allclose(xg, xw, rtol=1e-9, atol=1e-9 * np.max(np.abs(xw)))
    scale = np.max(np.abs(xw), axis=0)
    excess = np.abs(xg - xw) / np.maximum(1e-9 * (scale + np.abs(xw)), 1e-300)
    assert np.all((excess <= 1.0) | (xg == xw)), float(excess.max())
    assert np.all(xg[:, 1] == 0.0) and np.all(xw[:, 1] == 0.0)
