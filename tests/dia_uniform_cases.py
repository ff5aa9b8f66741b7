"""Matrices and the NumPy restatement shared by the uniform-slot-column tests
(tests/test_dia_uniform_plan.py on the host, tests/test_gpu_dia_uniform.py on
the device).

A slot column of the SELL-128/DIA image is uniform when the stored values of
all rows whose mask bit is set have one bit pattern: bits, not ==, so -0.0
differs from +0.0 and NaNs compare by payload; a single present row is
uniform; holes take no part."""
import numpy as np
import scipy.sparse


def csr_from_rows(n, entries, dtype=np.float64):
    """CSR with exactly the given (row, col, value) entries (sorted here by
    row and column; explicit zeros, -0.0 and NaN payloads kept bit for bit)."""
    entries = sorted(entries, key=lambda e: (e[0], e[1]))
    rows = np.array([e[0] for e in entries], dtype=np.int64)
    cols = np.array([e[1] for e in entries], dtype=np.int32)
    vals = np.array([e[2] for e in entries], dtype=dtype)
    indptr = np.searchsorted(rows, np.arange(n + 1)).astype(np.int32)
    A = scipy.sparse.csr_matrix((vals, cols, indptr), shape=(n, n))
    assert A.nnz == len(entries)
    return A


def nan_with_payload(payload):
    return np.array([0x7FF8000000000000 | payload], dtype=np.uint64).view(np.float64)[0]


def tridiag_special():
    """n = 200: slices of 128 and 72 rows, offsets -1, 0, 1 in both.
    Slice 0: offset -1 is -1 except row 50 (-1.5): streamed; offset 0 is +0.0
    except row 10 (-0.0): streamed, although == holds; offset +1 is one NaN
    except row 77, a NaN of another payload: streamed. Slice 1: offset -1 is
    uniform -1; offset 0 is one NaN payload throughout: uniform; offset +1 is
    present in row 150 alone: uniform. No row holds two NaNs."""
    n = 200
    nan_a, nan_b, nan_c = nan_with_payload(0x11), nan_with_payload(0x22), nan_with_payload(0x33)
    ent = []
    for r in range(n):
        if r >= 1:
            ent.append((r, r - 1, -1.5 if r == 50 else -1.0))
        if r < 128:
            ent.append((r, r, -0.0 if r == 10 else 0.0))
            ent.append((r, r + 1, nan_b if r == 77 else nan_a))
        else:
            ent.append((r, r, nan_c))
            if r == 150:
                ent.append((r, r + 1, 2.5))
    return csr_from_rows(n, ent)


TRIDIAG_FLAGS = [0, 0, 0, 1, 1, 1]  # the six slot columns of tridiag_special, in image order


def plan_matrices():
    from krylov_amd import problems

    W, _ = problems.shifted_lap3d_weighted(8)
    return {
        "stencil15_7": problems.stencil15_3d(7),  # n = 343: two full slices and a tail, boundary holes
        "poisson2d_61": problems.poisson2d(61),
        "tridiag_special": tridiag_special(),
        "shifted_lap3d_f32": W,  # row-scaled: mostly not uniform
    }


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint64 if v.dtype.itemsize == 8 else np.uint32)


def uniform_py(A, plan):
    """(flags, values) of every slot column from the plan's widths, offsets
    and masks (kry_dia_plan) and the matrix's stored values."""
    ip, ix, dv = A.indptr, A.indices, A.data
    n = A.shape[0]
    flags, values = [], []
    c = 0
    for s, w in enumerate(plan["widths"]):
        r0 = 128 * s
        for _ in range(int(w)):
            off = int(plan["offsets"][c])
            got = []
            for q in (0, 1):
                word = int(plan["masks"][2 * c + q])
                for lane in range(64):
                    if (word >> lane) & 1:
                        r = r0 + 2 * lane + q
                        assert r < n
                        e = ip[r] + int(np.searchsorted(ix[ip[r]:ip[r + 1]], r + off))
                        assert ix[e] == r + off
                        got.append((r, dv[e]))
            got.sort(key=lambda t: t[0])
            vals = np.array([v for _, v in got], dtype=dv.dtype)
            same = len(got) > 0 and bool(np.all(_bits(vals) == _bits(vals)[0]))
            flags.append(1 if same else 0)
            values.append(vals[0] if same else dv.dtype.type(0))
            c += 1
    return np.array(flags, dtype=np.int32), np.array(values, dtype=dv.dtype)
