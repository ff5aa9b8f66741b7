"""Exact-integer cases for the fused SpMV epilogues (host only).

Every solver step is an SpMV with an epilogue fused into it (csrc/device.hpp:
EpiResidual, EpiApDot, EpiStoreDot, EpiLanczos, ...). The library is built
with -ffp-contract=off and sums each row sequentially, so a stored vector is
what NumPy gives with the same element-wise operations; only the order in
which a fused dot's float64 block partials are summed is the device's own.
The cases here take that freedom away: A, b, x0 and the weights w hold small
integers, so every product, row sum and dot is an integer that is exact in
the working type in any order, and the device is compared with an integer
reference by ==.

* the matrix generators keep the sparsity patterns the SpMV tests already use
  (tests/spmv_patterns.py, tests/test_gpu_kernels.py,
  tests/test_gpu_dia_uniform.py) in their stored order and replace the values
  by integers in [-4, 4] with explicit zeros;
* rhs() builds b, x0, w with <r0, r0>_w an exact power of 4 in every column
  (r0 = b - A x0), so the norm's square root and V0 = r0 / 2^m are exact;
* Reference is integer arithmetic over the stored entries (int64, Python
  ints and fractions for the dyadic quantities); nothing comes from SciPy's
  float SpMV.

tests/test_epilogue_cases.py checks the magnitude condition of every case;
tests/test_gpu_epilogue_images.py runs them on the device."""
import functools
import os
from fractions import Fraction

import numpy as np
import scipy.sparse

LIMIT = {np.dtype(np.float32): 2**24, np.dtype(np.float64): 2**53}


# ----------------------------------------------------------------- matrices
def revalued(P, seed, const_offsets=None):
    """P's pattern, entry for entry in its stored order (unsorted rows and
    duplicates stay), with int64 values in [-4, 4]: random, every 17th stored
    entry an explicit zero; entries on a diagonal named in ``const_offsets``
    ({offset: value}) get that value instead."""
    rng = np.random.default_rng(seed)
    vals = rng.integers(-4, 5, P.nnz).astype(np.int64)
    vals[::17] = 0
    if const_offsets:
        rows = np.repeat(np.arange(P.shape[0], dtype=np.int64), np.diff(P.indptr))
        off = P.indices.astype(np.int64) - rows
        for o, v in const_offsets.items():
            vals[off == o] = v
    A = scipy.sparse.csr_matrix((vals, P.indices.copy(), P.indptr.copy()), shape=P.shape)
    assert A.nnz == P.nnz
    return A


def _band_pattern(n, offsets):
    A = scipy.sparse.diags([np.ones(n - abs(o)) for o in offsets], offsets, shape=(n, n), format="csr")
    A.sort_indices()
    A.indices = A.indices.astype(np.int32)
    A.indptr = A.indptr.astype(np.int32)
    return A


def _without_rows(P, rows):
    """P with the stored entries of ``rows`` removed (empty rows)."""
    keep = np.ones(P.shape[0], dtype=bool)
    keep[rows] = False
    lens = np.diff(P.indptr) * keep
    mask = np.repeat(keep, np.diff(P.indptr))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(P.indptr.dtype)
    return scipy.sparse.csr_matrix((P.data[mask], P.indices[mask], indptr), shape=P.shape)


def dia_narrow_plain():
    """5 slot columns, none uniform: the 5-point pattern on 41^2 (n = 1,681,
    odd: a partial last slice), every value random."""
    from krylov_amd import problems

    return revalued(problems.poisson2d(41), 21)


def dia_narrow_mixed():
    """The same pattern with constant off-diagonals (uniform slot columns)
    and a random diagonal (streamed) in every slice; rows 256..383 hold
    nothing (an empty interior slice of the 128-row image)."""
    from krylov_amd import problems

    P = _without_rows(problems.poisson2d(41), np.arange(256, 384))
    return revalued(P, 22, {-41: -1, -1: -2, 1: -1, 41: 3})


def dia_wide_plain():
    """15 slot columns (the 16-per-round kernel), none uniform: the full band
    -7..7 at n = 601, as tests/test_gpu_dia_uniform.py band15, with rows
    128..255 holding nothing (an empty interior slice)."""
    return revalued(_without_rows(_band_pattern(601, list(range(-7, 8))), np.arange(128, 256)), 23)


def dia_wide_mixed():
    """21 slot columns, two rounds per slice, every 4th diagonal random and
    the others constant (tests/test_gpu_dia_uniform.py band21_two_rounds)."""
    offs = list(range(-10, 11))
    const = {o: (t % 4) + 1 for t, o in enumerate(offs) if t % 4 != 3}
    return revalued(_band_pattern(601, offs), 24, const)


def dia_uniform():
    """Every slot column uniform: the 15-point stencil on 15^3 (n = 3,375)
    with centre 4 and neighbours -1."""
    from krylov_amd import problems

    P = problems.stencil15_3d(15)
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    const = {int(o): -1 for o in np.unique(P.indices.astype(np.int64) - rows)}
    const[0] = 4
    return revalued(P, 25, const)


def dia_uniform_12():
    """The same stencil on 12^3 (n = 1,728: 13 full slices and a half), whose
    slices share descriptor classes (tests/test_gpu_dia_classes.py)."""
    from krylov_amd import problems

    P = problems.stencil15_3d(12)
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    const = {int(o): -1 for o in np.unique(P.indices.astype(np.int64) - rows)}
    const[0] = 4
    return revalued(P, 32, const)


# launch_spmv gives the all-uniform wide kernel at most 5120 blocks of 4 waves,
# and wave m walks slices [S m / W, S (m + 1) / W): with S > 20480 slices some
# waves walk two, which is when a slice's store and dot run deferred behind
# the next slice's loads (and behind an empty next slice)
DIA_DEFERRED_N = 128 * 21500 + 67


def dia_uniform_deferred():
    """Nine constant diagonals -4..4 (all uniform, more than 8 slot columns)
    at n = 2,752,067 = 21,501 slices, one more than 1.05 x the 20,480 waves of
    the kernel's grid: about a thousand waves walk two slices. Every third
    slice of rows [128 * 9000, 128 * 12000) is empty, so two-slice waves meet
    (full, full), (full, empty) and (empty, full)."""
    n = DIA_DEFERRED_N
    offs = list(range(-4, 5))
    P = _band_pattern(n, offs)
    sl = np.arange(9000, 12000, 3)
    P = _without_rows(P, (sl[:, None] * 128 + np.arange(128)[None, :]).reshape(-1))
    return revalued(P, 33, {o: (o % 4) + 1 if o else -4 for o in offs})


def dia_band_3779():
    """A 15-offset band at the paired pattern's n = 3,779, none uniform: the
    diagonal-offset partner of pair_general() in the preconditioner cases."""
    return revalued(_band_pattern(128 * 29 + 67, list(range(-7, 8))), 26)


def pair_general():
    """The paired-row SELL-128 pattern (tests/spmv_patterns.py
    pair_adversarial): n = 128 * 29 + 67, rows of 0-20 entries, an empty
    slice, unsorted rows, duplicates."""
    from tests.spmv_patterns import pair_adversarial

    P, _ = pair_adversarial(np.float64)
    assert not P.has_sorted_indices
    return revalued(P, 27)


def rs_general():
    """The rank-sorted pattern (tests/spmv_patterns.py adversarial):
    n = 200,003, unsorted wide-span rows, duplicates, empty rows, rows of up
    to 70 entries."""
    from tests.spmv_patterns import adversarial

    P, _ = adversarial(np.float64)
    return revalued(P, 28)


def cb_scattered():
    """The column-blocked pattern (tests/spmv_patterns.py scattered_csr):
    n = 1,200,003, 150 entries in the first 700 rows, 300 empty rows, 6
    elsewhere."""
    from tests.spmv_patterns import scattered_csr

    n = 1_200_003
    lens = np.full(n, 6)
    lens[:700] = 150
    lens[1000:1300] = 0
    return revalued(scattered_csr(n, lens, seed=11), 29)


def sell_regular():
    """Regular SELL-64 slices (tests/test_gpu_kernels.py
    test_sell64_k1_regular_compact_bitwise): n = 64 * 37 + 5, sorted rows of
    0-16 banded entries, an empty slice, a full-width slice."""
    rng = np.random.default_rng(7)
    n = 64 * 37 + 5
    lens = rng.integers(0, 17, n)
    lens[64:128] = 0
    lens[128:192] = 16
    rows, cols = [], []
    for i in range(n):
        c = np.unique(rng.integers(max(0, i - 400), min(n, i + 400), lens[i]))
        rows.append(np.full(c.shape[0], i))
        cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    P = scipy.sparse.csr_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(n, n))
    P.sort_indices()
    return revalued(P, 30)


def sell_irregular():
    """The adversarial matrix of tests/golden/spmv.npz (unsorted rows,
    duplicates, empty rows, one 3000-entry row: an irregular slice walked
    through the CSR arrays)."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmv.npz"))
    ip, ix = d["f64_i32_indptr"], d["f64_i32_indices"]
    n = ip.shape[0] - 1
    P = scipy.sparse.csr_matrix((np.ones(ix.shape[0]), ix, ip), shape=(n, n))
    return revalued(P, 31)


MATRICES = {f.__name__: f for f in (dia_narrow_plain, dia_narrow_mixed, dia_wide_plain, dia_wide_mixed, dia_uniform,
                                    dia_uniform_12, dia_uniform_deferred, dia_band_3779, pair_general, rs_general,
                                    cb_scattered, sell_regular, sell_irregular)}


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The named integer matrix (int64 values), built once per process."""
    return MATRICES[name]()


def as_float(A, dtype):
    """The integer matrix as a float CSR in the same stored order."""
    B = scipy.sparse.csr_matrix((A.data.astype(dtype), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    assert B.nnz == A.nnz
    return B


# ------------------------------------------------------- integer arithmetic
def int_spmv(A, X, absolute=False):
    """A X over the stored entries in int64 (duplicates added twice, explicit
    zeros multiplied, as csr_matvecs does); absolute: |A| |X|, which bounds
    every partial sum of every row in any order."""
    X = np.asarray(X, dtype=np.int64)
    X2 = X.reshape(X.shape[0], -1)
    a = np.asarray(A.data, dtype=np.int64)
    prod = a[:, None] * X2[A.indices]
    if absolute:
        prod = np.abs(prod)
    cum = np.zeros((prod.shape[0] + 1, X2.shape[1]), dtype=np.int64)
    np.cumsum(prod, axis=0, out=cum[1:])
    ip = np.asarray(A.indptr, dtype=np.int64)
    return (cum[ip[1:]] - cum[ip[:-1]]).reshape(X.shape)


def wdot(x, y, w):
    """<x, y>_w per column as Python ints."""
    x2 = np.asarray(x, dtype=np.int64).reshape(x.shape[0], -1)
    y2 = np.asarray(y, dtype=np.int64).reshape(y.shape[0], -1)
    t = x2 * (np.asarray(w, dtype=np.int64)[:, None] * y2)
    return [int(v) for v in t.sum(axis=0)]


def four_squares(r):
    """Lagrange: non-negative a >= b >= c >= d with a^2 + b^2 + c^2 + d^2 = r."""
    assert r >= 0
    a = int(np.sqrt(r)) + 1
    for a in range(a, -1, -1):
        for b in range(min(a, int(np.sqrt(max(r - a * a, 0))) + 1), -1, -1):
            for c in range(b, -1, -1):
                rest = r - a * a - b * b - c * c
                if rest < 0:
                    continue
                d = int(round(np.sqrt(rest)))
                if d <= c and d * d == rest:
                    return a, b, c, d
    raise AssertionError(r)


def _r0_column(w, rng):
    """One column of r0: no zero entry but those Lagrange leaves, |r0| <= 5,
    sum_i w_i r0_i^2 = 4^m exactly. Every row starts at +-1; rows taken in a
    random order go to +-3 (8 w_i more each) while that fits under the next
    power of 4; four rows of weight 1 then take the four squares of what is
    left."""
    n = w.shape[0]
    sign = rng.choice(np.array([-1, 1], dtype=np.int64), n)
    mag = np.ones(n, dtype=np.int64)
    s0 = int(w.sum())
    m = 0
    while 4**m < s0:
        m += 1
    order = rng.permutation(n)
    ones = order[w[order] == 1]
    assert ones.shape[0] >= 4
    fix = ones[-4:]  # rows of weight 1 kept for the four squares
    cand = order[~np.isin(order, fix)]
    cum = np.cumsum(8 * w[cand])
    take = int(np.searchsorted(cum, 4**m - s0, side="right"))
    mag[cand[:take]] = 3
    left = 4**m - s0 - (int(cum[take - 1]) if take else 0)
    assert 0 <= left
    mag[fix] = four_squares(left + 4)  # the four rows gave 1 each so far
    r0 = sign * mag
    assert int((w * r0 * r0).sum()) == 4**m
    return r0, m


def rhs(A, k, weighted, seed):
    """b, x0 (n x k; length n for k = 1) and w as int64 with |x0| <= 3,
    1 <= w <= 3 (all 1 unweighted), and b = A x0 + r0 where
    <r0, r0>_w is an exact power of 4 in every column: b is A x0 + (+-1 or
    +-3) but for four rows of weight 1 per column, whose entries carry the
    four squares of the remainder."""
    rng = np.random.default_rng(seed)
    n = A.shape[0]
    w = rng.integers(1, 4, n).astype(np.int64) if weighted else np.ones(n, dtype=np.int64)
    x0 = rng.integers(-3, 4, (n, k)).astype(np.int64)
    r0 = np.stack([_r0_column(w, rng)[0] for _ in range(k)], axis=1)
    b = int_spmv(A, x0) + r0
    if k == 1:
        b, x0 = b[:, 0], x0[:, 0]
    return b, x0, w


# ---------------------------------------------------------------- reference
class Reference:
    """The exact quantities of the first solver step on (A, b, x0, w), per
    column: r0 = b - A x0, rho0 = <r0, r0>_w = 4^m, Ar = A r0,
    pAp = <r0, A r0>_w; V0 = r0 / 2^m, H00 = <V0, A V0>_w = pAp / 4^m."""

    def __init__(self, A, b, x0, w):
        self.shape = b.shape
        b2, x2 = b.reshape(b.shape[0], -1), x0.reshape(x0.shape[0], -1)
        self.w = w
        self.Ax0 = int_spmv(A, x2)
        self.r0 = b2 - self.Ax0
        self.rho0 = wdot(self.r0, self.r0, w)
        self.m = []
        for v in self.rho0:
            m = 0
            while 4**m < v:
                m += 1
            self.m.append(m)
        self.Ar = int_spmv(A, self.r0)
        self.pAp = wdot(self.r0, self.Ar, w)
        self.h00 = [Fraction(p, 4**m) for p, m in zip(self.pAp, self.m)]
        # what bounds every intermediate: row partial sums in any order, the
        # stored vectors, and the dots' terms summed in absolute value
        absw = np.asarray(w, dtype=np.int64)[:, None]
        self.max_vector = max(int(np.abs(v).max()) for v in (b2, x2, self.Ax0, self.r0, self.Ar,
                                                               int_spmv(A, x2, absolute=True),
                                                               int_spmv(A, self.r0, absolute=True)))
        self.max_dot = max(max(self.rho0), max(abs(p) for p in self.pAp))
        self.max_dot_abs = int(max((absw * self.r0 * self.r0).sum(axis=0).max(),
                                   (absw * np.abs(self.r0) * np.abs(self.Ar)).sum(axis=0).max()))

    def exact_in(self, dtype):
        """The condition under which the device comparison is exact in
        ``dtype`` vectors: every stored element, row partial sum and dot total
        is an integer below the dtype's limit (the dots' float64 partials sum
        terms whose absolute values stay below 2^53 in any order)."""
        lim = LIMIT[np.dtype(dtype)]
        return self.max_vector < lim and self.max_dot < lim and self.max_dot_abs < 2**53

    def v0(self, dtype):
        """V0 = r0 / 2^m in ``dtype`` (exact: a power-of-two scaling)."""
        return (self.r0.astype(dtype) / np.array([2.0**m for m in self.m], dtype=dtype)).reshape(self.shape)


# ----------------------------------------------------------- configurations
def dia_form(A):
    """(UNI, slot columns per round) of the k = 1 diagonal-offset kernel
    launch_spmv picks for the float matrix A, from the host plans: UNI 0 = no
    uniform slot column, 1 = some, 2 = all (8 per round whatever the width)."""
    from krylov_amd import _lib

    plan = _lib.dia_plan(A.indptr, A.indices)
    up = _lib.dia_uniform_plan(A.indptr, A.indices, A.data)
    assert plan is not None and up is not None
    uni = 2 if up["uniform"] == up["cols"] else (0 if up["uniform"] == 0 else 1)
    return uni, (8 if uni == 2 or plan["max_width"] <= 8 else 16)


def dia_waves_walk_two(A):
    """The all-uniform wide kernel's grid (at most 5120 blocks of 4 waves,
    launch_spmv) has fewer waves than the image has slices: wave m walks
    slices [S m / W, S (m + 1) / W), so some waves walk two."""
    from krylov_amd import _lib

    plan = _lib.dia_plan(A.indptr, A.indices)
    return dia_form(A) == (2, 8) and plan["max_width"] > 8 and plan["slices"] > 4 * 5120


class Config:
    """One image configuration: the matrix, its value dtype, the vector
    dtype, the column count, whether the inner product is weighted, the
    environment switches and the layout() fields that prove the kernel."""

    def __init__(self, id, matrix, k=1, mdtype=np.float64, vdtype=None, weighted=False, env=None, expect=None,
                 form=None, index64=False, persist=False):
        self.id, self.matrix, self.k = id, matrix, k
        self.mdtype = np.dtype(mdtype)
        self.vdtype = np.dtype(vdtype if vdtype is not None else mdtype)
        self.weighted = weighted
        self.env = dict(env or {})
        self.expect = dict(expect or {})
        self.form = form  # DIA, k = 1: (UNI, slot columns per round)
        self.index64 = index64  # int64 indices handed to kry_csr_create
        self.persist = persist  # the persistent CG loop must accept the case
        assert not (weighted and self.vdtype != np.float64)  # Problem promotes weighted solves

    def problem(self):
        """(A as a float CSR, b, x0, w as int64, the Reference)"""
        return _problem(self.matrix, self.k, self.weighted, self.mdtype.name)

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def _problem(name, k, weighted, mdtype):
    A = matrix(name)
    b, x0, w = rhs(A, k, weighted, seed=1001 + 7 * k + (1 if weighted else 0))
    return as_float(A, np.dtype(mdtype)), b, x0, w, Reference(A, b, x0, w)


def clear_caches():
    """Drop the matrices and problems built so far (about 0.5 GB with the
    n = 1,200,003 case): the test modules call it when they finish, so the
    rest of the suite's process does not carry them."""
    _problem.cache_clear()
    matrix.cache_clear()


_SELL = {"KRY_SPMV_DIA": "0", "KRY_SPMV_PAIR": "0", "KRY_SPMV_RS": "0"}
_DIA = {"dia": True, "renumbered": False}
_GEN = {"dia": False, "renumbered": False, "col_blocks": 0}


def _configs():
    out = []
    forms = {"dia_narrow_plain": (0, 8), "dia_wide_plain": (0, 16), "dia_narrow_mixed": (1, 8),
             "dia_wide_mixed": (1, 16), "dia_uniform": (2, 8)}
    for name, form in forms.items():
        for lean in (True, False):
            out.append(Config(f"{name}-{'lean' if lean else 'wide_address'}", name,
                              env={} if lean else {"KRY_DIA_LEAN": "0"}, expect=dict(_DIA, dia_lean=lean), form=form,
                              persist=True))
    out.append(Config("dia_narrow_mixed-weighted", "dia_narrow_mixed", weighted=True, expect=_DIA, form=(1, 8)))
    out.append(Config("dia_wide_plain-f32", "dia_wide_plain", mdtype=np.float32, expect=_DIA, form=(0, 16),
                      persist=True))
    out.append(Config("dia_uniform-f32_matrix_f64_vectors", "dia_uniform", mdtype=np.float32, vdtype=np.float64,
                      expect=_DIA, form=(2, 8)))
    # a wave walks two slices: the deferred store and dot, also behind an empty slice
    for lean in (True, False):
        out.append(Config(f"dia_uniform_deferred-{'lean' if lean else 'wide_address'}", "dia_uniform_deferred",
                          env={} if lean else {"KRY_DIA_LEAN": "0"},
                          expect=dict(_DIA, dia_lean=lean, classes=True, two_slice_waves=True), form=(2, 8)))
    out.append(Config("dia_uniform_12-classes", "dia_uniform_12", expect=dict(_DIA, classes=True), form=(2, 8)))
    out.append(Config("dia_uniform_12-no_classes", "dia_uniform_12", env={"KRY_DIA_CLASSES": "0"},
                      expect=dict(_DIA, dia_classes=0), form=(2, 8)))
    # block right-hand sides on the diagonal-offset image
    for k in (2, 4, 8):
        out.append(Config(f"dia_blk-k{k}", "dia_wide_plain", k=k, expect=_DIA))
    out.append(Config("dia_blk-k4-weighted", "dia_wide_plain", k=4, weighted=True, expect=_DIA))
    for k in (4, 8):
        out.append(Config(f"dia_blk-k{k}-f32", "dia_wide_plain", k=k, mdtype=np.float32, expect=_DIA))
    # (no KRY_SPMV_DIA_BLK=0 twin: the library reads that switch once per process, so a test cannot
    # select the lane-group kernel on a DIA operator and no layout() field would show it; that kernel
    # runs on the general matrix below)
    # the paired image
    for dt in (np.float64, np.float32):
        out.append(Config(f"pair-{np.dtype(dt).name}", "pair_general", mdtype=dt, expect=dict(_GEN, pair=True)))
    out.append(Config("pair-weighted", "pair_general", weighted=True, expect=dict(_GEN, pair=True)))
    # the rank-sorted image, its three kernels
    for rs1 in ("0", "1", "2"):
        out.append(Config(f"rs-rs1_{rs1}", "rs_general", env={"KRY_SPMV_RS1": rs1, "KRY_RENUMBER": "0"},
                          expect=dict(_GEN, rs=True, pair=False)))
    out.append(Config("rs-f32", "rs_general", mdtype=np.float32, env={"KRY_RENUMBER": "0"},
                      expect=dict(_GEN, rs=True, pair=False)))
    out.append(Config("rs-int64-f32_matrix_f64_vectors", "rs_general", mdtype=np.float32, vdtype=np.float64,
                      index64=True, env={"KRY_RENUMBER": "0"}, expect=dict(_GEN, rs=True, pair=False)))
    # column-blocked
    for dt in (np.float64, np.float32):
        out.append(Config(f"cb-{np.dtype(dt).name}", "cb_scattered", mdtype=dt, env={"KRY_RENUMBER": "0"},
                          expect={"dia": False, "renumbered": False, "col_blocks": 5}))
    # SELL-64 at k = 1
    sell = dict(_GEN, pair=False, rs=False)
    out.append(Config("sell-compact", "sell_regular", env=_SELL, expect=dict(sell, compact=True, irregular=0),
                      persist=True))
    out.append(Config("sell-compact-f32", "sell_regular", mdtype=np.float32, env=_SELL,
                      expect=dict(sell, compact=True, irregular=0), persist=True))
    out.append(Config("sell-plain", "sell_regular", env=dict(_SELL, KRY_SELL_COMPACT="0"),
                      expect=dict(sell, compact=False, irregular=0), persist=True))
    out.append(Config("sell-irregular", "sell_irregular", env=_SELL, expect=dict(sell, irregular_slices=True)))
    out.append(Config("sell-int64", "sell_regular", env=_SELL, index64=True, expect=dict(sell, compact=False)))
    # block right-hand sides on a general matrix: k = 2 (SELL-64), 4-64 (lane groups), 128 (KT = 8)
    for k in (2, 4, 16, 64):
        for compact in (True, False):
            out.append(Config(f"general_blk-k{k}-{'compact' if compact else 'plain'}", "pair_general", k=k,
                              env={} if compact else {"KRY_SELL_COMPACT": "0"}, expect=dict(_GEN, compact=compact)))
    out.append(Config("general_blk-k4-weighted", "pair_general", k=4, weighted=True, expect=dict(_GEN, compact=True)))
    out.append(Config("general_blk-k16-f32", "pair_general", k=16, mdtype=np.float32, expect=dict(_GEN, compact=True)))
    out.append(Config("general_blk-k128", "pair_general", k=128, expect=_GEN))
    return out


CONFIGS = _configs()

# (A, M) pairs of the matrix-preconditioner cases: each on another image
PRECOND_PAIRS = [("dia_band_3779", "pair_general"), ("pair_general", "dia_band_3779")]
