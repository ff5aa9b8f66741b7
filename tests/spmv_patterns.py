"""General-CSR sparsity patterns shared by the SpMV tests
(tests/test_gpu_kernels.py, tests/test_gpu_renumber.py) and the exact epilogue
cases (tests/epilogue_cases.py). Host only."""
import numpy as np
import scipy.sparse


def pair_adversarial(dtype, seed=11):
    """A general CSR for the paired-row SELL-128 image: n not a multiple of
    128 or of 2, rows of 0-20 entries, an empty slice, unsorted rows,
    duplicate and explicit-zero entries, values and x spanning 1e+-20
    (1e+-8 in float32, where products stay finite); even
    rows 2l and odd rows 2l + 1 share their offsets in some slices (one 16-B
    x load serves both) and not in others (the second load)."""
    rng = np.random.default_rng(seed)
    n = 128 * 29 + 67
    lens = rng.integers(0, 21, n)
    lens[128:256] = 0  # an empty slice
    rows, cols = [], []
    for i in range(n):
        if (i // 128) % 3 == 0:  # stencil-like: pairs of rows share offsets
            offs = np.sort(rng.choice(np.arange(-900, 900), lens[i - (i & 1)], replace=False))
            c = np.clip(i + offs, 0, n - 1)[: lens[i]]
        else:
            c = rng.integers(max(0, i - 3000), min(n, i + 3000), lens[i])
            if i % 5 == 0:
                c = np.sort(c)
        if i % 7 == 0 and c.shape[0] > 1:
            c[-1] = c[0]  # a duplicate (kept, added twice as csr_matvec does)
        rows.append(np.full(c.shape[0], i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    e = 20 if dtype == np.float64 else 8
    vals = (rng.standard_normal(rows.shape[0]) * 10.0 ** rng.integers(-e, e, rows.shape[0])).astype(dtype)
    vals[::17] = 0.0  # explicit zeros
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    A = scipy.sparse.csr_matrix((vals, cols.astype(np.int32), indptr), shape=(n, n))  # stored order kept
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-e, e, n)).astype(dtype)
    return A, x


def scattered_csr(n, lens, seed, sort=True, dtype=np.float64):
    """CSR with lens[i] uniform random columns in row i (scattered sparsity)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, indptr[-1])
    if sort:
        order = np.lexsort((cols, rows))
        cols = cols[order]
    vals = rng.standard_normal(indptr[-1]).astype(dtype)
    A = scipy.sparse.csr_matrix((vals, cols.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    return A


def adversarial(dtype, seed=0, n=200_003, long_rows=True):
    """Unsorted rows, duplicates, explicit zeros, empty rows, rows longer than
    one 16-entry run (whole slices of them: the image refuses more than 1.25x
    the SELL-64 slots), values and x over a wide exponent range."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    if long_rows:
        lens[1024:1280] = rng.integers(17, 70, 256)
        lens[2048:2176] = rng.integers(30, 34, 128)
    lens[100:130] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cols = rng.integers(0, n, indptr[-1]).astype(np.int32)  # unsorted, wide spans
    dup = rng.integers(0, indptr[-1], indptr[-1] // 20)
    cols[dup[1:]] = cols[dup[:-1]]
    e = 30 if dtype == np.float64 else 8
    vals = (rng.standard_normal(indptr[-1]) * 10.0 ** rng.integers(-e, e, indptr[-1])).astype(dtype)
    vals[::13] = 0.0
    A = scipy.sparse.csr_matrix((vals, cols, indptr), shape=(n, n))
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-e, e, n)).astype(dtype)
    return A, x
