"""The host builder's descriptor classes of the SELL-128/DIA image, without a
device (kry_dia_class_plan): the counts a CPU enumeration of the 15-point
stencil's presence rules gives, one slot column per offset present in a
slice, with and without uniform detection; no classes where nothing is shared
or the table would not be smaller than the per-slice descriptors."""
import numpy as np
import pytest
import scipy.sparse

from krylov_amd import _lib, problems


def _csr(A):
    A = scipy.sparse.csr_matrix(A)
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def _blocks(A):
    """Distinct (offset, even-row mask, odd-row mask) blocks of the 128-row
    slices, straight from the CSR arrays: (classes, class columns, columns)."""
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    offs = A.indices.astype(np.int64) - rows
    seen, cols = {}, 0
    for s in range((n + 127) // 128):
        sel = (rows >= 128 * s) & (rows < 128 * s + 128)
        block = []
        for o in np.unique(offs[sel]):
            rl = rows[sel][offs[sel] == o] - 128 * s
            m = [0, 0]
            for r in rl:
                m[r & 1] |= 1 << (int(r) >> 1)
            block.append((int(o), m[0], m[1]))
        cols += len(block)
        seen.setdefault(tuple(block), len(block))
    return len(seen), sum(seen.values()), cols


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("m, want", [(8, (3, 45)), (12, (13, 185)), (16, (6, 70)), (24, (16, 200)), (40, (22, 270))])
def test_stencil_class_counts(m, want, uniform):
    A = _csr(problems.stencil15_3d(m))
    plan = _lib.dia_class_plan(A.indptr, A.indices, A.data, uniform=uniform)
    assert (plan["classes"], plan["class_cols"]) == want
    ncls, ccols, cols = _blocks(A)
    assert (ncls, ccols) == want and plan["cols"] == cols


def test_single_slice_takes_no_classes():
    """One slice: its table would be as large as its descriptors."""
    A = _csr(problems.stencil15_3d(5))
    plan = _lib.dia_class_plan(A.indptr, A.indices, A.data)
    assert plan["cols"] > 0 and (plan["classes"], plan["class_cols"]) == (0, 0)


def test_values_split_classes_only_through_uniform_columns():
    """A tridiagonal matrix whose diagonal differs from slice to slice: with
    uniform detection the value sits in the block and splits the classes;
    without it the three interior slices share one block again."""
    n = 128 * 5
    d = np.repeat(np.arange(2.0, 7.0), 128)
    A = _csr(scipy.sparse.diags([np.full(n - 1, -1.0), d, np.full(n - 1, -1.0)], [-1, 0, 1]))
    on = _lib.dia_class_plan(A.indptr, A.indices, A.data, uniform=True)
    off = _lib.dia_class_plan(A.indptr, A.indices, A.data, uniform=False)
    assert (on["classes"], on["class_cols"]) == (0, 0)  # five distinct blocks: nothing saved
    assert (off["classes"], off["class_cols"]) == (3, 9) and off["cols"] == 15
