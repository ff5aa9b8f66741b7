"""Shapes, inputs and NumPy references shared by the kernel tests of the
scalar-chain vector ops and kry_dot (tests/test_gpu_chain_ops.py on the
device, tests/test_chain_cases.py on the host).

Everything here runs through one template, elementwise_kernel /
launch_elementwise (krylov_amd/csrc/device.hpp): a vector of N = n * k
elements is cut into groups of W elements (16 bytes: W = 2 for float64, 4 for
float32), a block takes GROUPS_PER_BLOCK groups until the grid reaches
MAX_GRID blocks, and above that the per-block span grows in steps of
BLOCK_THREADS groups. The shapes below are the smallest at which each of
these rules can go wrong; test_chain_cases.py derives the property each list
is named for from the constants, so a shape cannot sit in the wrong list."""
import fractions
import functools
import math

import numpy as np

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
DTYPES = (F64, F32)
BLOCK_THREADS = 256      # kBlock
GROUPS_PER_BLOCK = 512   # launch_elementwise: grid_for(groups, kBlock * 2)
MAX_GRID = 8192          # kMaxGrid

LC_AXPY, LC_NEST_ADD, LC_NEST_SUB, LC_DIV, LC_SUB, LC_ADD, LC_COPY, LC_SCALE = range(8)
FORMS = tuple(range(8))
NEEDS_Y = (LC_AXPY, LC_NEST_ADD, LC_NEST_SUB, LC_SUB, LC_ADD)
NEEDS_W = (LC_NEST_ADD, LC_NEST_SUB)  # and b
NEEDS_A = (LC_AXPY, LC_NEST_ADD, LC_NEST_SUB, LC_DIV, LC_SCALE)
SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))


def width(dtype):
    """Elements per 16-byte group."""
    return 16 // np.dtype(dtype).itemsize


def bits(a):
    """The raw bits of a float array (so -0.0 differs from +0.0)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == F64 else np.uint32)


# ------------------------------------------------------------------ shapes
def tail_shapes(dtype):
    """N = n * k is no multiple of W: the last group is a scalar tail."""
    s = [(n, 1) for n in (1, 3, 1023, 1025, 2049, 100003)]
    if np.dtype(dtype) == F32:
        s += [(n, 2) for n in (1, 513, 1025)]
    return s


def boundary_shapes(dtype):
    """k = 1, N one group or one element to either side of g full blocks."""
    W = width(dtype)
    out = []
    for g in (1, 2, 3):
        for d in (-W, -1, 1, W):
            out.append((GROUPS_PER_BLOCK * W * g + d, 1))
    return out


COLUMN_SHAPES = ((513, 2), (5003, 4), (1001, 8), (129, 16), (33, 64), (4099, 64))
# kry_dot alone admits k up to 256 (lincomb and the chain stop at 64)
WIDE_DOT_SHAPES = ((33, 128), (517, 128), (9, 256), (1001, 256))


def above_cap_shape(dtype):
    """One element group past MAX_GRID full blocks at k = 64."""
    return (131075, 64) if np.dtype(dtype) == F64 else (262147, 64)


def elementwise_shapes(dtype):
    """Every shape below the grid cap, in list order, without repeats."""
    out = []
    for s in list(tail_shapes(dtype)) + list(boundary_shapes(dtype)) + list(COLUMN_SHAPES):
        if s not in out:
            out.append(s)
    return out


def launch_geometry(N, dtype):
    """(groups, grid, groups per block, first empty block or None) as
    launch_elementwise and elementwise_kernel compute them."""
    W = width(dtype)
    ngrp = -(-N // W)
    grid = max(1, min(MAX_GRID, -(-ngrp // GROUPS_PER_BLOCK)))
    per = -(-(-(-ngrp // grid)) // BLOCK_THREADS) * BLOCK_THREADS
    first_empty = -(-ngrp // per)
    return ngrp, grid, per, (first_empty if first_empty < grid else None)


# ----------------------------------------------------------- lincomb inputs
def specials(dtype):
    fi = np.finfo(dtype)
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny], dtype=dtype)


def _seed(*key):
    return [int(v) for v in key]


@functools.lru_cache(maxsize=4)
def lincomb_case(n, k, dtype):
    """x, y, w (n x k, standard normal in `dtype`) and per-column float64
    coefficients a, b, pairwise distinct after the cast to `dtype`. Where the
    vectors are long enough their first 81 elements hold every pair of
    special values in (x, y), w walking through them at another stride."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(11, n, k, dtype.itemsize))
    x, y, w = (rng.standard_normal((n, k)).astype(dtype) for _ in range(3))
    sp = specials(dtype)
    m = len(sp)
    nspecial = 0
    if n * k >= 2 * m * m:
        i = np.arange(m * m)
        x.reshape(-1)[: m * m] = sp[i // m]
        y.reshape(-1)[: m * m] = sp[i % m]
        w.reshape(-1)[: m * m] = sp[(i // m + 2 * (i % m) + 3) % m]
        nspecial = m * m
    while True:
        # magnitudes in [0.5, 2): a small coefficient's product rounds far below
        # the sum's last bit, and a contraction would then hardly ever show
        a, b = (rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k) for _ in range(2))
        both = np.concatenate([a.astype(dtype), b.astype(dtype)])
        if len(set(np.abs(both).tolist())) == 2 * k and np.all(both != 0):
            break
    for v in (x, y, w, a, b):
        v.setflags(write=False)
    return {"x": x, "y": y, "w": w, "a": a, "b": b, "nspecial": nspecial}


def lincomb_ref(form, x, y, w, a, b):
    """The header's NumPy expression for `form` in the vectors' dtype V: the
    float64 coefficients are cast to V first (the kernel's `(V)s.a[c]`), every
    operation rounds once to V, nothing is fused."""
    V = x.dtype
    a = None if a is None else np.asarray(a, dtype=np.float64).astype(V)
    b = None if b is None else np.asarray(b, dtype=np.float64).astype(V)
    with np.errstate(all="ignore"):
        if form == LC_AXPY:
            z = x + a * y
        elif form == LC_NEST_ADD:
            z = x + a * (y + b * w)
        elif form == LC_NEST_SUB:
            z = x + a * (y - b * w)
        elif form == LC_DIV:
            z = x / a
        elif form == LC_SUB:
            z = x - y
        elif form == LC_ADD:
            z = x + y
        elif form == LC_COPY:
            z = x.copy()
        elif form == LC_SCALE:
            z = a * x
        else:
            raise ValueError(form)
    assert z.dtype == V and z.shape == x.shape
    return z


def aliases(form):
    """Operand the destination aliases: None (a vector of its own), "x", "y",
    "w", or "xy" (z its own, x and y one vector: forms 4 and 5)."""
    out = [None, "x"]
    if form in NEEDS_Y:
        out.append("y")
    if form in NEEDS_W:
        out.append("w")
    if form in (LC_SUB, LC_ADD):
        out.append("xy")
    return out


def lincomb_combinations(dtype):
    """(form, shape, alias) for every lincomb test below the grid cap."""
    return [(f, s, al) for f in FORMS for s in elementwise_shapes(dtype) for al in aliases(f)]


def fused_last_step(form, x, y, w, a, b, sample=None):
    """(unfused, fused) results of forms 0, 1, 2 when only the last
    multiply-add `x + a * t` is contracted (one rounding instead of two),
    over the finite elements (optionally the first `sample` of them).
    float32: the contraction evaluated in float64 and rounded once;
    float64: exact rational arithmetic."""
    V = x.dtype
    av, bv = a.astype(V), b.astype(V)
    with np.errstate(all="ignore"):
        t = y if form == LC_AXPY else (y + bv * w if form == LC_NEST_ADD else y - bv * w)
        plain = x + av * t
    ab = np.broadcast_to(av, x.shape)
    ok = np.isfinite(plain) & np.isfinite(x) & np.isfinite(t)
    xs, ts, as_, ps = x[ok], t[ok], ab[ok], plain[ok]
    if sample is not None:
        xs, ts, as_, ps = xs[:sample], ts[:sample], as_[:sample], ps[:sample]
    if V == F32:
        fused = (xs.astype(np.float64) + as_.astype(np.float64) * ts.astype(np.float64)).astype(V)
    else:
        Fr = fractions.Fraction
        fused = np.array([float(Fr(float(xx)) + Fr(float(aa)) * Fr(float(tt))) for xx, aa, tt in zip(xs, as_, ts)],
                         dtype=V)
    return ps, fused


def subnormal_cases():
    """float32 cases (name, form, x, y, w, a, b; one column, n = 1027) in
    which operands, intermediate values and results are subnormal: every
    form on subnormal vectors of either sign (a third of x small normals, so
    that sums and quotients cross the boundary both ways), and forms 0 and 7
    with a coefficient that is itself subnormal in float32 on normal data."""
    n = 1027
    rng = np.random.default_rng(_seed(13))
    tiny = np.finfo(np.float32).tiny

    def sub():
        mant = rng.integers(1, 0x800000, n, dtype=np.uint32)
        sign = rng.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)
        return (mant | sign).view(np.float32).reshape(n, 1).copy()

    x, y, w = sub(), sub(), sub()
    x[::3, 0] = (tiny * rng.uniform(1.0, 4.0, len(x[::3]))).astype(np.float32)
    out = []
    for form in FORMS:
        a = np.array([3.0 if form == LC_DIV else 0.7])
        out.append((f"form{form}", form, x, y, w, a, np.array([1.3])))
    xn = rng.standard_normal((n, 1)).astype(np.float32)
    yn = rng.standard_normal((n, 1)).astype(np.float32)
    asub = np.array([3.3e-40])
    out.append(("axpy_subnormal_coefficient", LC_AXPY, x, yn, w, asub, np.array([1.0])))
    out.append(("scale_subnormal_coefficient", LC_SCALE, xn, yn, w, asub, np.array([1.0])))
    return out


def is_subnormal(a):
    a = np.asarray(a)
    return (a != 0) & (np.abs(a) < np.finfo(a.dtype).tiny)


# ---------------------------------------------------------- rowscale inputs
@functools.lru_cache(maxsize=4)
def rowscale_case(n, k, dtype):
    """x (n x k) and d (n,), d in [0.5, 3) and odd multiples of 2^-10 or
    random: quotients by them are inexact, so a reciprocal-multiply shows."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(17, n, k, dtype.itemsize))
    x = rng.standard_normal((n, k)).astype(dtype)
    d = rng.uniform(0.5, 3.0, n).astype(dtype)
    d[::7] = (2 * rng.integers(300, 1500, len(d[::7])) + 1) / 1024.0
    d[::11] *= -1
    x.setflags(write=False)
    d.setflags(write=False)
    return x, d


def rowscale_ref(x, d, mul):
    assert d.dtype == x.dtype and d.shape == (x.shape[0],)
    z = (x.T * d).T if mul else (x.T / d).T
    assert z.dtype == x.dtype
    return np.ascontiguousarray(z)


# --------------------------------------------------------------- dot inputs
@functools.lru_cache(maxsize=4)
def exact_dot_case(n, k, dtype):
    """Integer data whose inner products are exact in any summation order:
    x, y in [-8, 8], weights in {1, 2, 4}; the first rows of every column are
    redrawn until the k weighted sums, and the k unweighted ones, are
    pairwise distinct. Returns x, y (dtype), w (float64), and the exact sums
    as Python-exact int64 (unweighted, weighted)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(19, n, k, dtype.itemsize))
    xi = rng.integers(-8, 9, (n, k), dtype=np.int64)
    yi = rng.integers(-8, 9, (n, k), dtype=np.int64)
    wi = rng.choice(np.array([1, 2, 4], dtype=np.int64), n)
    plain = (xi * yi).sum(axis=0)
    wsum = (xi * wi[:, None] * yi).sum(axis=0)
    head = min(n, 4)
    seen_p, seen_w = set(), set()
    for c in range(k):
        for _ in range(10000):
            if int(plain[c]) not in seen_p and int(wsum[c]) not in seen_w:
                break
            xi[:head, c] = rng.integers(-8, 9, head)
            yi[:head, c] = rng.integers(-8, 9, head)
            plain[c] = (xi[:, c] * yi[:, c]).sum()
            wsum[c] = (xi[:, c] * wi * yi[:, c]).sum()
        else:
            raise AssertionError(f"column {c} of ({n}, {k}): no distinct sum found")
        seen_p.add(int(plain[c]))
        seen_w.add(int(wsum[c]))
    x, y, w = xi.astype(dtype), yi.astype(dtype), wi.astype(np.float64)
    for v in (x, y, w, plain, wsum):
        v.setflags(write=False)
    return {"x": x, "y": y, "w": w, "plain": plain, "weighted": wsum}


@functools.lru_cache(maxsize=4)
def random_dot_case(n, k, dtype):
    """Standard normal x, y rounded to `dtype`, float64 weights in [1, 2)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(_seed(23, n, k, dtype.itemsize))
    x = rng.standard_normal((n, k)).astype(dtype)
    y = rng.standard_normal((n, k)).astype(dtype)
    w = rng.uniform(1.0, 2.0, n)
    for v in (x, y, w):
        v.setflags(write=False)
    return x, y, w


def gamma(n):
    """gamma_m = m u / (1 - m u), m = n + 2, u = 2^-53: a term x (w y) carries
    two roundings and at most n - 1 additions in whatever order the sum runs,
    n + 1 factors (1 + delta) in all (Higham, Accuracy and Stability, Lemma 3.1
    and (3.5)); the last unit covers the error of the extended-precision
    `exact` below."""
    m, u = n + 2, 2.0 ** -53
    return m * u / (1 - m * u)


def dot_exact_and_scale(x, y, w):
    """Per column: sum x_i w_i y_i and sum |x_i w_i y_i| of the inputs as
    given (already rounded to their dtype), in x87 extended precision:
    products and NumPy's pairwise sum err by a few dozen units of 2^-64
    relative to the scale, under one unit of u = 2^-53 for n < 2^24."""
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63, "np.longdouble is not an extended format here"
    assert x.shape[0] < 1 << 24
    t = x.astype(LD) * y.astype(LD)
    if w is not None:
        t = t * w.astype(LD)[:, None]
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def dot_fsum(x, y, w):
    """The exact integer sums of integer-valued data through math.fsum."""
    k = x.shape[1]
    wv = np.ones(x.shape[0]) if w is None else w
    return [math.fsum((x[:, c].astype(np.float64) * wv * y[:, c].astype(np.float64)).tolist()) for c in range(k)]
