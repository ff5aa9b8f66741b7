"""Inputs, the float64 reference and the comparison rule of the float32
solver tests (tests/test_gpu_f32.py on the device, tests/test_f32_cases.py on
the host). Everything is rebuilt from seeds; pure NumPy / SciPy plus
oracle/krylov_ref.py, nothing of krylov_amd but its problem generators.

The float kernels group 4 elements per lane (2 in float64), so the sizes are
n = 4097..4100 (n mod 4 = 1, 2, 3, 0) and the last three entries of every
right-hand-side column are scaled by 100: the ragged tail carries most of
||b||, and a kernel that drops it is wrong by O(1), not by O(1e-4).

The reference of a case is the oracle run in float64 on the float32-rounded A
and b. The bound is the oracle's own float32 spread: the oracle run in
float32 under several valid evaluations of its inner product (VARIANTS), whose
largest relative deviation from the float64 history, carried forward as a
running maximum, is the envelope env[i] (the construction of
gpu_helpers.selfnoise_envelope). The device may deviate from the float64 entry
i by max(NOISE_FACTOR * env[i], FLOOR) relative. With ortho="householder" the
reference's inner products sit inside the reflectors, out of reach of
``inner=``; the variants go there through the oracle's ``house_dot`` hook, or
all of them would be one and the same float32 run.

FLOOR = 2 eps32 is derived: an entry with no recurrence behind it is one
rounding of the norm (eps32 / 2) of elements that are each float32-rounded
(at most eps32 / 2 more on the norm), times the same factor 2. The oracle's
default float32 inner (OpenBLAS sdot / einsum) is recorded ("default") but
stays out of the envelope: its error grows with n (5e-5 at n = 4.2 M).
"""
import functools

import numpy as np
import scipy.sparse as sp

from krylov_amd import problems
from oracle import krylov_ref
from tests.gpu_helpers import NOISE_FACTOR

EPS32 = 2.0 ** -23
FLOOR = 2.0 * EPS32
W = 4                 # Vec16<float>::W: elements per lane
SIZES = (4097, 4098, 4099, 4100)
COLUMNS = (1, 2, 3, 8)
STEPS = 25
TAIL = 3              # entries of every column scaled by TAIL_SCALE
TAIL_SCALE = 100.0
ENVELOPE_CAP = 1e-5   # a small case whose envelope exceeds this is a poor case
NPERM = 4
# the variants of the envelope; the large cases take the first two only
VARIANTS = ("pairwise", "f64acc") + tuple(f"perm{i}" for i in range(NPERM))
LARGE_VARIANTS = ("pairwise", "f64acc")
LARGE_M = (1449, 2048, 2049)
_LARGE_MATRICES = tuple(f"poisson{m}" for m in LARGE_M)
LARGE_STEPS = 6
STOP_TOL = 1e-4
STOP_MARGIN = 0.01


# ---------------------------------------------------------------- matrices
def _band64(n):
    """The banded_general matrix of tests/test_gpu_dia.py at n rows: a
    symmetrised random band at offsets 0, +-1, +-17, +-301 plus a dominant
    diagonal (float64, before rounding)."""
    rng = np.random.default_rng(9)
    offs = [-301, -17, -1, 0, 1, 17, 301]
    A = sp.diags([rng.uniform(-1.0, 0.0, n - abs(o)) for o in offs], offs, format="csr")
    A = (A + A.T).tocsr()
    A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)).tocsr()
    A.sort_indices()
    return A


def matrix(name):
    """A float32 CSR matrix by name: "nonsym<n>" = problems.random_nonsym(n);
    "band<n>" = the SPD band; "indef<n>" = the band minus the median of its
    diagonal (a shift inside its spectrum: the diagonal of the result has both
    signs); "poisson<m>" = problems.poisson2d(m). The small ones are built
    once and shared; of the three large ones (170 MB each) only the last one
    used is held, until release_large()."""
    if name in _LARGE_MATRICES:
        return _large_matrix(name)
    return _shared_matrix(name)


@functools.lru_cache(maxsize=None)
def _shared_matrix(name):
    return _matrix(name)


@functools.lru_cache(maxsize=1)
def _large_matrix(name):
    return _matrix(name)


def release_large():
    """Drop the large matrix held: the one test of a large case calls this
    when it is done, so that nothing of its size stays with the process."""
    _large_matrix.cache_clear()


def _matrix(name):
    if name.startswith("nonsym"):
        A = problems.random_nonsym(int(name[6:]))
    elif name.startswith("band"):
        A = _band64(int(name[4:]))
    elif name.startswith("indef"):
        A = _band64(int(name[5:]))
        A = (A - float(np.float32(np.median(A.diagonal()))) * sp.identity(A.shape[0])).tocsr()
        A.sort_indices()
    else:
        assert name.startswith("poisson"), name
        A = problems.poisson2d(int(name[7:]))
    A = A.astype(np.float32)
    A.sort_indices()
    return A


def rhs(n, k, seed=0):
    """The float32 right-hand side: shape (n,) for k = 1, (n, k) otherwise;
    standard normal, column c scaled by 10^u_c (u_c in [-1, 1], so the
    columns' residuals differ in size), the last TAIL rows scaled by
    TAIL_SCALE."""
    rng = np.random.default_rng([seed, n, k])
    B = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-1.0, 1.0, k)
    B[-TAIL:] *= TAIL_SCALE
    B = B.astype(np.float32)
    return B[:, 0].copy() if k == 1 else B


def jacobi(name):
    """A float32 Jacobi-like diagonal preconditioner of a matrix (the inverse
    diagonal times a seeded factor in [0.5, 1.5])."""
    A = matrix(name)
    d = np.abs(A.diagonal().astype(np.float64))
    f = np.random.default_rng(6).uniform(0.5, 1.5, A.shape[0])
    return sp.diags((f / d).astype(np.float32)).tocsr()


# ------------------------------------------------------------------- cases
# (id, solver, matrix, k, keyword arguments); M / Mr = "jacobi" is jacobi() of
# the case's matrix
def _small_cases():
    out = []
    for n in SIZES:
        for k in COLUMNS:
            out.append((f"cg_band{n}_k{k}", "cg", f"band{n}", k, {}))
            out.append((f"minres_band{n}_k{k}", "minres", f"band{n}", k, {}))
            out.append((f"minres_indef{n}_k{k}", "minres", f"indef{n}", k, {}))
            out.append((f"gmres_nonsym{n}_k{k}", "gmres", f"nonsym{n}", k, {}))
        for ortho in ("mgs2", "householder"):
            out.append((f"gmres_{ortho}_nonsym{n}_k1", "gmres", f"nonsym{n}", 1, {"ortho": ortho}))
    for m in (63, 64):
        out.append((f"cg_poisson{m}_k1", "cg", f"poisson{m}", 1, {}))
        out.append((f"minres_poisson{m}_k1", "minres", f"poisson{m}", 1, {}))
    out.append(("cg_M_band4099_k1", "cg", "band4099", 1, {"M": "jacobi"}))
    out.append(("minres_M_band4099_k1", "minres", "band4099", 1, {"M": "jacobi"}))
    out.append(("gmres_Mr_nonsym4099_k1", "gmres", "nonsym4099", 1, {"Mr": "jacobi"}))
    return out


SMALL = _small_cases()
for _c in SMALL:
    _c[4].update(tol=0.0, maxiter=STEPS)
# one stop-at-tolerance case per solver: the float64 run and every variant stop
# at the same step, and the float64 history at that step and the one before
# lies STOP_MARGIN away from the criterion (tests/test_f32_cases.py checks it)
STOP = [
    ("cg_stop_band4099", "cg", "band4099", 1, dict(tol=STOP_TOL, maxiter=200)),
    ("gmres_stop_nonsym4099", "gmres", "nonsym4099", 1, dict(tol=STOP_TOL, maxiter=60)),
    ("minres_stop_band4098", "minres", "band4098", 1, dict(tol=STOP_TOL, maxiter=200)),
]
LARGE = [(f"gmres_poisson{m}", "gmres", f"poisson{m}", 1, dict(tol=0.0, maxiter=LARGE_STEPS)) for m in LARGE_M]
CASES = SMALL + STOP + LARGE
del _c
# the cases the reference itself was run on in float32 with its default inner
# (tests/golden/make_f32.py -> f32.npz): every n mod 4, k = 1, 2 and 3, the
# three orthogonalisations; tests/test_oracle.py holds the oracle to them
PINNED = (
    "cg_band4097_k1", "cg_band4098_k2", "cg_band4099_k3", "cg_band4100_k1",
    "gmres_nonsym4097_k2", "gmres_nonsym4098_k3", "gmres_nonsym4099_k1", "gmres_nonsym4100_k2",
    "gmres_mgs2_nonsym4097_k1", "gmres_householder_nonsym4098_k1",
    "minres_indef4097_k3", "minres_band4098_k1", "minres_indef4099_k2", "minres_band4100_k1",
)


def case(cid):
    return next(c for c in CASES if c[0] == cid)


def ids(cases):
    return [c[0] for c in cases]


def select(solver=None, k=None, matrix_prefix=None, plain=None):
    """The small cases of a solver / column count / matrix family; plain =
    True keeps those with no ortho and no preconditioner."""
    out = []
    for c in SMALL:
        extra = set(c[4]) - {"tol", "maxiter"}
        if solver is not None and c[1] != solver:
            continue
        if k is not None and c[3] not in (k if isinstance(k, tuple) else (k,)):
            continue
        if matrix_prefix is not None and not c[2].startswith(matrix_prefix):
            continue
        if plain is not None and plain != (not extra):
            continue
        out.append(c)
    return out


def build(c):
    """-> (solver, A (float32 CSR), b (float32), keyword arguments with the
    named preconditioners substituted)."""
    _, solver, name, k, kw = c
    A = matrix(name)
    kw = dict(kw)
    for key in ("M", "Mr"):
        if key in kw:
            kw[key] = jacobi(name)
    return solver, A, rhs(A.shape[0], k), kw


# --------------------------------------------------------- inner products
def _colsum(p):
    """NumPy's pairwise sum of the products, per column (the pairwise order
    applies along the contiguous axis only)."""
    if p.ndim == 1:
        return np.add.reduce(p)
    return np.add.reduce(np.ascontiguousarray(p.T), axis=1).reshape(p.shape[1:])


def _f64acc(x, y):
    s = np.einsum("i...,i...->...", x.astype(np.float64), y.astype(np.float64))
    return s.astype(np.float32)[()] if x.dtype == np.float32 else s


def inner_of(variant, n):
    """The inner product of a variant, for the oracle's ``inner=``. Each is a
    valid evaluation of the reference's <x, y>:
    pairwise  NumPy's pairwise sum of the float32 products;
    f64acc    products and sum in float64, rounded once (the device's model);
    perm<i>   the pairwise sum of the products in a fixed random order (of a
              shorter vector, a Householder reflector's: the same order with
              the missing indices left out);
    default   None: the oracle's own np.dot / np.einsum."""
    if variant == "default":
        return None
    if variant == "pairwise":
        return lambda x, y: _colsum(x * y)
    if variant == "f64acc":
        return _f64acc
    assert variant.startswith("perm"), variant
    perm = np.random.default_rng(1000 + int(variant[4:])).permutation(n)
    return lambda x, y: _colsum((x * y)[perm if x.shape[0] == n else perm[perm < x.shape[0]]])


def mutant_inner(kind, n):
    """Two wrong inner products the bound has to catch: "tail" leaves out the
    last n mod 4 elements (the last one when n mod 4 = 0), a dropped ragged
    tail; "scaled" is off by 1 + 1e-5, the size of error a flat 1e-4 hides.
    Both on the f64acc form. (A Householder reflector's shorter vectors end
    where the full ones do and lose the same elements.)"""
    if kind == "tail":
        drop = n % W or 1
        return lambda x, y: _f64acc(x[:x.shape[0] - drop], y[:x.shape[0] - drop])
    assert kind == "scaled", kind
    return lambda x, y: (_f64acc(x, y) * np.float32(1.0 + 1e-5)).astype(np.float32)[()]


# --------------------------------------------------------------- the runs
def _as_run(info):
    return {"numsteps": int(info.numsteps), "success": bool(info.success),
            "resnorms": np.asarray(info.resnorms), "xk": np.asarray(info.xk)}


def run_oracle(c, dtype=np.float32, inner=None):
    """One oracle run of a case in ``dtype``: {"numsteps", "success",
    "resnorms" (as np.asarray makes them), "xk"}."""
    solver, A, b, kw = build(c)
    conv = (lambda M: M) if dtype == np.float32 else (lambda M: M.astype(np.float64))
    kw = {k: (conv(v) if k in ("M", "Mr") else v) for k, v in kw.items()}
    if kw.get("ortho") == "householder":
        # the reference's Householder Arnoldi takes its inner products inside
        # the reflectors, where ``inner`` does not reach: the variant goes there too
        kw["house_dot"] = inner
    _, info = getattr(krylov_ref, solver)(conv(A), b.astype(dtype), inner=inner, **kw)
    return _as_run(info)


def hist64(run):
    return np.asarray(run["resnorms"], dtype=np.float64)


def rel_history(run, ref):
    """|h - h64| / h64 per entry (0 where both are 0)."""
    h, h64 = hist64(run), hist64(ref)
    assert h.shape == h64.shape, (h.shape, h64.shape)
    return np.abs(h - h64) / np.where(h64 != 0.0, h64, 1.0)


def rel_solution(run, ref):
    """||x - x64||_inf / ||x64||_inf (over all columns)."""
    x, x64 = np.asarray(run["xk"], dtype=np.float64), np.asarray(ref["xk"], dtype=np.float64)
    assert x.shape == x64.shape
    return float(np.max(np.abs(x - x64)) / np.max(np.abs(x64)))


def reference(cid):
    """-> {"ref": the float64 run, "variants": {name: float32 run}, "default":
    the float32 run under the oracle's own inner, "env": the per-entry
    envelope, "xenv": the solution's}. Computed once per small case and
    shared, the callers do not modify it; a large case's (its iterates are
    17 to 34 MB each) is computed for its one test and not kept."""
    if case(cid) in LARGE:
        return _reference(cid)
    return _shared_reference(cid)


@functools.lru_cache(maxsize=None)
def _shared_reference(cid):
    return _reference(cid)


def _reference(cid):
    c = case(cid)
    n = matrix(c[2]).shape[0]
    ref = run_oracle(c, np.float64)
    names = LARGE_VARIANTS if c in LARGE else VARIANTS
    runs = {v: run_oracle(c, np.float32, inner_of(v, n)) for v in names}
    out = {"ref": ref, "variants": runs, "default": run_oracle(c, np.float32)}
    same = [r for r in runs.values() if r["numsteps"] == ref["numsteps"]]
    out["env"] = envelope(same, ref) if same else None
    out["xenv"] = max(rel_solution(r, ref) for r in same) if same else None
    return out


def envelope(runs, ref):
    """env[i] = max over j <= i and over the runs of |h[j] - h64[j]| / h64[j].
    The last entry of a solve that stopped at the tolerance, the explicit
    residual, has its own bound (final_atol) and stays out."""
    rel = np.max([rel_history(r, ref).reshape(hist64(ref).shape[0], -1).max(axis=1) for r in runs], axis=0)
    if ref["success"]:
        rel[-1] = 0.0
    return np.maximum.accumulate(rel)


def stop_margin(run, tol=STOP_TOL):
    """How far the history of a run that stopped at step s lies from the
    criterion tol * h[0] at s - 1 and at s, relative to the criterion (the
    updated residual at s is not kept: the explicit one replaced it, and it
    is that one the stop rule confirmed)."""
    h = hist64(run)
    crit = tol * h[0]
    return float(min(abs(h[-2] - crit), abs(h[-1] - crit)) / crit)


def history_bound(env):
    return np.maximum(NOISE_FACTOR * env, FLOOR)


def solution_bound(xenv):
    return max(NOISE_FACTOR * xenv, FLOOR)


def final_atol(c, ref):
    """The project's bound on the final explicit residual:
    64 eps (||b|| + ||A||_1 ||x||) per column, with eps = eps32."""
    _, A, b, _ = build(c)
    a1 = float(abs(A.astype(np.float64)).sum(axis=0).max())
    x = np.asarray(ref["xk"], dtype=np.float64)
    return 64.0 * EPS32 * (np.linalg.norm(b.astype(np.float64), axis=0) + a1 * np.linalg.norm(x, axis=0))


def used(run, R, c):
    """(history, solution): the largest deviation of a run from the float64
    reference as a fraction of its bound; above 1 the run fails. The last
    entry of a run that stopped at the tolerance is the explicit residual: it
    is compared under final_atol and counts into the history's figure."""
    ref = R["ref"]
    rel = rel_history(run, ref)
    rel = rel.reshape(rel.shape[0], -1).max(axis=1)
    frac = rel / history_bound(R["env"])
    if ref["success"]:
        d = np.abs(hist64(run)[-1] - hist64(ref)[-1])
        frac[-1] = float(np.max(d / final_atol(c, ref)))
    return float(frac.max()), rel_solution(run, ref) / solution_bound(R["xenv"])


def check_device(info, cid):
    """Assert a device result against a case's float64 reference under the
    bound; -> (history, solution) fractions of the bound used."""
    c, R = case(cid), reference(cid)
    ref, ora = R["ref"], R["default"]
    run = _as_run(info)
    assert run["numsteps"] == ref["numsteps"] and run["success"] == ref["success"], (run["numsteps"], ref["numsteps"])
    assert run["xk"].dtype == ora["xk"].dtype == np.float32
    assert run["resnorms"].dtype == ora["resnorms"].dtype, (run["resnorms"].dtype, ora["resnorms"].dtype)
    assert run["resnorms"].shape == ora["resnorms"].shape and run["xk"].shape == ora["xk"].shape
    assert np.all(np.isfinite(run["resnorms"])) and np.all(np.isfinite(run["xk"]))
    uh, ux = used(run, R, c)
    body = slice(None, -1) if ref["success"] else slice(None)
    dev = float(rel_history(run, ref)[body].max())
    sdot = f"{used(ora, R, c)[0]:.2f}" if ora["numsteps"] == ref["numsteps"] else "other step count"
    print(f"{cid}: env {R['env'].max():.2e} dev {dev:.2e} dev/bound {uh:.3f} | x: env {R['xenv']:.2e} "
          f"dev {rel_solution(run, ref):.2e} dev/bound {ux:.3f} | oracle default inner dev/bound {sdot}")
    assert uh <= 1.0 and ux <= 1.0, (cid, uh, ux)
    return uh, ux
