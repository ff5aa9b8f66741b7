"""Destroying an operator gives back every device byte that creating it took.

One small operator of every kind of image kry_csr_create builds (csr_upload's
steps, csr_free's list for all of them), each created by the
device build and by the host builders (KRY_DEVICE_BUILD=0): layout() shows the
intended image, and after close() the allocator's bytes_in_use is back where
it was. A create that raises leaves it unchanged too. The matrices are the
ones that pin each selection in test_gpu_device_build.py, test_gpu_kernels.py,
test_gpu_renumber.py and test_gpu_dia_classes.py.
"""
import ctypes
import functools
import gc

import numpy as np
import pytest
import scipy.sparse

from tests.spmv_patterns import scattered_csr
from tests.test_gpu_device_build import _cases
from tests.test_gpu_dia_classes import _random_holes

pytestmark = pytest.mark.gpu


class _Int64Operator:
    """int64 index arrays handed straight to kry_csr_create (CsrOperator
    passes int32 whenever the matrix fits)."""

    def __init__(self, A):
        from krylov_amd import _lib
        from krylov_amd.device import get_context

        ip, ix = A.indptr.astype(np.int64), A.indices.astype(np.int64)
        dv = np.ascontiguousarray(A.data)
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.lib.kry_csr_create(get_context().handle, A.shape[0], ix.shape[0], _lib.ptr(ip), _lib.ptr(ix),
                                           _lib.ptr(dv), _lib.dtype_code(dv.dtype), _lib.KRY_I64,
                                           ctypes.byref(self.handle)))

    def layout(self):
        import krylov_amd

        return krylov_amd.CsrOperator.layout(self)

    def close(self):
        from krylov_amd import _lib

        _lib.check(_lib.lib.kry_csr_destroy(self.handle))


@functools.lru_cache(maxsize=None)
def _matrix(name):
    from krylov_amd import problems

    if name == "span65535":  # test_compact_boundary_spread: one slot column too wide for a uint16 delta
        rows = np.arange(64)
        cols = np.where(rows == 0, 65535, 0).astype(np.int32)
        return scipy.sparse.csr_matrix((np.arange(1.0, 65.0), (rows, cols)), shape=(70_000, 70_000))
    if name == "scattered":  # test_column_blocked_long_segments_and_empty_rows
        lens = np.full(1_200_003, 6)
        lens[:700] = 150
        lens[1000:1300] = 0
        return scattered_csr(1_200_003, lens, seed=11, dtype=np.float64)
    if name == "perm104":  # test_gpu_renumber.py's fixture
        return problems.permuted_sym(problems.stencil15_3d(104), 11)
    if name == "random_holes":
        return _random_holes()
    if name == "irregular":
        return _cases()["irregular"]
    if name == "empty":
        return scipy.sparse.csr_matrix((7, 7))
    return problems.stencil15_3d(int(name))


def _create(name):
    import krylov_amd

    return krylov_amd.CsrOperator(_matrix(name))


# kind -> (create, environment, what layout() must show)
KINDS = {
    "dia_classes_uniform": (lambda: _create("8"), {},
                            lambda lay: lay["dia"] and lay["dia_classes"] == 3 and lay["dia_uniform_cols"] > 0),
    "dia_no_classes": (lambda: _create("random_holes"), {}, lambda lay: lay["dia"] and lay["dia_classes"] == 0),
    "sell_compact_only": (lambda: _create("8"), {"KRY_SPMV_DIA": "0", "KRY_SPMV_PAIR": "0", "KRY_SPMV_RS": "0"},
                          lambda lay: lay["compact"] and lay["slots"] > 0 and lay["col_blocks"] == 0
                          and not (lay["dia"] or lay["pair"] or lay["rs"])),
    "sell_not_compact": (lambda: _create("span65535"), {}, lambda lay: not lay["compact"] and lay["slots"] > 0),
    "irregular_kept_csr": (lambda: _create("irregular"), {}, lambda lay: lay["irregular"] > 0),
    "int64": (lambda: _Int64Operator(_matrix("irregular")), {},
              lambda lay: lay["irregular"] > 0 and not lay["compact"] and lay["slots"] > 0),
    "paired": (lambda: _create("20"), {"KRY_SPMV_DIA": "0"}, lambda lay: lay["pair"] and not lay["dia"]),
    "rank_sorted": (lambda: _create("20"), {"KRY_SPMV_DIA": "0", "KRY_SPMV_PAIR": "0"},
                    lambda lay: lay["rs"] and not lay["pair"] and not lay["dia"]),
    "column_blocked": (lambda: _create("scattered"), {}, lambda lay: lay["col_blocks"] == 5 and not lay["renumbered"]),
    "renumbered": (lambda: _create("perm104"), {},
                   lambda lay: lay["renumbered"] and lay["rs"] and lay["col_blocks"] == 0 and not lay["dia"]),
    "empty": (lambda: _create("empty"), {}, lambda lay: lay["slots"] == 0 and lay["col_blocks"] == 0),
}


def _in_use():
    import krylov_amd

    gc.collect()  # operators other tests dropped are freed now, not between the two readings
    return krylov_amd.memory_stats()["bytes_in_use"]


def _both_builds(create, shows, monkeypatch):
    """create() by the device build and by the host builders: the layout, and
    every byte back after close()."""
    before = _in_use()
    ops = [create()]
    monkeypatch.setenv("KRY_DEVICE_BUILD", "0")
    ops.append(create())
    monkeypatch.delenv("KRY_DEVICE_BUILD")
    for op in ops:
        assert shows(op.layout()), op.layout()
    assert _in_use() > before
    for op in ops:
        op.close()
    assert _in_use() == before


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_close_returns_every_byte(kind, monkeypatch):
    from krylov_amd.device import get_context

    get_context()
    create, env, shows = KINDS[kind]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _both_builds(create, shows, monkeypatch)


def test_close_returns_every_byte_created_like_renumbered(monkeypatch):
    """kry_csr_create_like: the images of P A P^T under another operator's
    permutation, with that operator alive before and after."""
    import krylov_amd

    base = _create("perm104")
    assert base.renumbered
    _both_builds(lambda: krylov_amd.CsrOperator(_matrix("perm104"), like=base),
                 lambda lay: lay["renumbered"] and lay["rs"] and lay["rcm_levels"] == 0, monkeypatch)
    base.close()


@pytest.mark.parametrize("device_build", ["1", "0"])
@pytest.mark.parametrize("defect", ["col_negative", "col_too_large", "indptr_decreasing"])
def test_rejected_create_leaves_nothing_allocated(defect, device_build, monkeypatch):
    """test_device_build_rejects_invalid_csr's three defects, under both builders."""
    import krylov_amd
    from krylov_amd import problems
    from krylov_amd.device import get_context

    get_context()
    monkeypatch.setenv("KRY_DEVICE_BUILD", device_build)
    A = problems.poisson2d(100).tocsr().copy()
    if defect == "col_negative":
        A.indices[777] = -1
    elif defect == "col_too_large":
        A.indices[778] = A.shape[0]
    else:
        A.indptr[5000] = A.indptr[5001] + 1
    before = _in_use()
    with pytest.raises(ValueError):
        krylov_amd.CsrOperator(A)
    assert _in_use() == before
