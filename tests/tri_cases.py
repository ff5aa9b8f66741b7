"""Matrices whose triangles exercise the sparse triangular solve's plan
(kry_tri_plan) and kernels, shared by tests/test_tri_plan.py (host) and
tests/test_gpu_trisolve.py (device), and a NumPy restatement of the plan."""
import numpy as np
import scipy.sparse as sp

GROUP_ROWS = 1024  # kTriGroupRows (csrc/host_common.hpp)
SLICE = 64

NAMES = ["n1", "diagonal", "chain300", "arrow3000", "poisson40", "rand5000", "level64", "level65"]


def _fan(m):
    """Row 0 coupled to rows 1..m (both ways): the lower triangle has a level
    of exactly m rows."""
    r = np.arange(1, m + 1)
    A = sp.coo_matrix((np.ones(2 * m), (np.concatenate([r, np.zeros(m, int)]), np.concatenate([np.zeros(m, int), r]))),
                      shape=(m + 1, m + 1))
    return (A + sp.identity(m + 1)).tocsr()


def pattern(name):
    """A square CSR matrix; its tril / triu are the triangles under test."""
    from krylov_amd import problems

    if name == "n1":
        A = sp.csr_matrix(np.array([[2.0]]))
    elif name == "diagonal":
        A = sp.identity(50, format="csr")
    elif name == "chain300":  # 300 levels of one row
        A = sp.diags([np.ones(299), np.ones(300), np.ones(299)], [-1, 0, 1], format="csr")
    elif name == "arrow3000":  # last row (and column) full: a row of 3,000 entries, a level of 2,999 rows
        n = 3000
        r = np.arange(n - 1)
        last = np.full(n - 1, n - 1)
        A = sp.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([last, r]), np.concatenate([r, last]))), shape=(n, n))
        A = (A + sp.identity(n)).tocsr()
    elif name == "poisson40":
        A = problems.poisson2d(40)
    elif name == "rand5000":
        A = problems.random_nonsym(5000)
    elif name == "level64":
        A = _fan(64)
    elif name == "level65":
        A = _fan(65)
    else:
        raise KeyError(name)
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def triangle(A, lower):
    T = (sp.tril(A) if lower else sp.triu(A)).tocsr()
    T.sort_indices()
    return T


def plan_py(T, lower):
    """Restatement of kry_tri_plan: level[i] = 1 + max(level[j]) over the
    off-diagonal columns of row i; rows ordered by (level, row); slices of up
    to 64 rows inside a level, width = the slice's longest off-diagonal row;
    launches: a level above 1024 rows alone, else the longest run of
    consecutive levels holding at most 1024 rows together."""
    ip, ix = T.indptr.astype(np.int64), T.indices.astype(np.int64)
    n = T.shape[0]
    level = np.zeros(n, dtype=np.int32)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        cols = ix[ip[i]:ip[i + 1]]
        deps = cols[cols != i]
        level[i] = 1 + (level[deps].max() if deps.size else 0)
    order = np.argsort(level, kind="stable").astype(np.int32)
    nlev = int(level.max()) if n else 0
    counts = np.bincount(level, minlength=nlev + 1)[1:]
    off = np.diff(ip) - 1
    widths = []
    start = 0
    for c in counts:
        rows = order[start:start + c]
        for a in range(0, c, SLICE):
            widths.append(int(off[rows[a:a + SLICE]].max()))
        start += c
    launch = [0]
    lev = 0
    while lev < nlev:
        tot, e = counts[lev], lev + 1
        if tot <= GROUP_ROWS:
            while e < nlev and tot + counts[e] <= GROUP_ROWS:
                tot += counts[e]
                e += 1
        launch.append(e)
        lev = e
    widths = np.array(widths, dtype=np.int32)
    return {"levels": nlev, "launches": len(launch) - 1, "slices": len(widths), "slots": int(SLICE * widths.sum()),
            "max_level": int(counts.max()) if nlev else 0, "level": level, "order": order,
            "launch": np.array(launch, dtype=np.int32), "widths": widths}


def exact_system(A, lower, dtype, k, seed=0):
    """A triangle of A's pattern with small integer off-diagonals and a
    diagonal in {+-1, +-2, +-4}, small integer x, and y = T x formed exactly
    (every partial sum is an integer below 2^24)."""
    rng = np.random.default_rng(seed)
    T = triangle(A, lower).astype(np.float64)
    T.data = rng.choice([-2.0, -1.0, 1.0, 2.0], T.nnz)
    T.setdiag(rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], T.shape[0]))
    T = T.tocsr()
    T.sort_indices()
    shape = (T.shape[0],) if k == 1 else (T.shape[0], k)
    x = rng.integers(-3, 4, shape).astype(np.float64)
    y = T @ x
    return T.astype(dtype), x.astype(dtype), y.astype(dtype)
