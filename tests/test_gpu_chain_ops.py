"""Kernel tests of the scalar-chain vector ops (krylov_amd/csrc/blas.hip:
kry_vec_lincomb, kry_prog_*) and kry_dot, which all run through
elementwise_kernel / launch_elementwise (device.hpp).

include/krylov_hip.h promises that every lincomb form is evaluated exactly as
its NumPy expression tree: the comparisons here are on the raw bits. Inner
products are compared exactly on integer data (any summation order gives the
same integer) and against the order-independent gamma bound on random data.
Shapes, inputs and references come from tests/chain_cases.py;
tests/test_chain_cases.py checks on the host that they can fail."""
import ctypes
import types

import numpy as np
import pytest

from tests import chain_cases as CC

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------- helpers
def _ctx():
    from krylov_amd.device import get_context

    return get_context()


def _up(a):
    from krylov_amd.device import DeviceVector

    return DeviceVector.from_host(_ctx(), a)


def _h(v):
    return None if v is None else v.handle


class _StandIn:
    """What extra._Chain reads of an extra._Dev: ctx, w, prob.kpad and
    prob.inner_dtype."""

    def __init__(self, k, dtype=np.float64, w=None):
        self.ctx = _ctx()
        self.w = w
        self.prob = types.SimpleNamespace(kpad=int(k), inner_dtype=np.dtype(dtype))


def _chain(k, names, cap=8, dtype=np.float64):
    from krylov_amd import extra

    return extra._Chain(_StandIn(k, dtype), list(names), cap=cap)


def _check(C, name, mode, st):
    """kry_prog_check with the mode as given (Chain.check adds bit 2 by dtype)."""
    from krylov_amd import _lib

    _lib.check(_lib.lib.kry_prog_check(C.h, C.r[name], mode, st))


def _assert_bits(got, want, what=""):
    """Same NaNs, and the same bits wherever the reference is not NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"NaN pattern {what}")
    np.testing.assert_array_equal(CC.bits(got)[~wn], CC.bits(want)[~wn], err_msg=str(what))


def _operands(case, form, alias):
    """Device vectors (z, x, y, w) for one launch and the host operands the
    reference takes. The destination is a fresh zeroed vector or the fresh
    upload of the operand it aliases, so a launch that did nothing shows."""
    from krylov_amd.device import DeviceVector

    hx = case["x"]
    hy = case["y"] if form in CC.NEEDS_Y else None
    hw = case["w"] if form in CC.NEEDS_W else None
    if alias == "xy":
        hy = hx
    dx = _up(hx)
    dy = dx if alias == "xy" else (None if hy is None else _up(hy))
    dw = None if hw is None else _up(hw)
    if alias in (None, "xy"):
        dz = DeviceVector(_ctx(), hx.shape[0], hx.shape[1], hx.dtype)
    else:
        dz = {"x": dx, "y": dy, "w": dw}[alias]
    return dz, dx, dy, dw, hx, hy, hw


def _vec_lincomb(form, case, alias):
    from krylov_amd import _lib

    dz, dx, dy, dw, hx, hy, hw = _operands(case, form, alias)
    a = np.ascontiguousarray(case["a"]) if form in CC.NEEDS_A else None
    b = np.ascontiguousarray(case["b"]) if form in CC.NEEDS_W else None
    _lib.check(_lib.lib.kry_vec_lincomb(_ctx().handle, form, dz.handle, dx.handle, _h(dy), _h(dw),
                                        None if a is None else _lib.dptr(a), None if b is None else _lib.dptr(b)))
    return dz.to_host(), CC.lincomb_ref(form, hx, hy, hw, a, b)


def _prog_lincomb(C, form, case, alias, sa, sb):
    """Through the chain: registers "a", "b" hold the unsigned coefficients."""
    dz, dx, dy, dw, hx, hy, hw = _operands(case, form, alias)
    ra = "a" if form in CC.NEEDS_A else None
    rb = "b" if form in CC.NEEDS_W else None
    C.begin()
    C.lc(form, dz, dx, 0, y=dy, w=dw, a=ra, sa=sa, b=rb, sb=sb)
    C.end(0)
    ref = CC.lincomb_ref(form, hx, hy, hw, None if ra is None else sa * case["a"], None if rb is None else sb * case["b"])
    return dz.to_host(), ref


def _lincomb_both(form, case, alias, chains):
    k, dtype = case["x"].shape[1], case["x"].dtype
    if k not in chains:
        chains[k] = _chain(k, ["a", "b"], cap=2, dtype=dtype)
    C = chains[k]
    C.set("a", case["a"])
    C.set("b", case["b"])
    what = (form, dtype.name, case["x"].shape, alias)
    got_v, ref = _vec_lincomb(form, case, alias)
    _assert_bits(got_v, ref, ("kry_vec_lincomb",) + what)
    for sa, sb in CC.SIGNS:
        got_p, ref_p = _prog_lincomb(C, form, case, alias, sa, sb)
        _assert_bits(got_p, ref_p, ("kry_prog_lincomb", sa, sb) + what)
        if (sa, sb) == (1.0, 1.0):
            # the two entry points agree bit for bit, NaN payloads aside
            _assert_bits(got_p, got_v, ("prog against vec",) + what)


# ------------------------------------------------------------- 1. lincomb
@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("form", CC.FORMS)
def test_lincomb_bitwise_both_entry_points(form, dtype):
    """Every form at every tail, block-boundary and column shape, with the
    destination on its own and aliasing each operand, through kry_vec_lincomb
    and through kry_prog_lincomb under the four sign combinations: the bits
    of the header's NumPy expression in the vectors' dtype."""
    chains = {}
    ran = 0
    for n, k in CC.elementwise_shapes(dtype):
        case = CC.lincomb_case(n, k, dtype)
        for alias in CC.aliases(form):
            _lincomb_both(form, case, alias, chains)
            ran += 1
    assert ran == len([c for c in CC.lincomb_combinations(dtype) if c[0] == form])
    print(f"form {form} {np.dtype(dtype).name}: {ran} (shape, alias) combinations, 5 launches each")


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_lincomb_above_the_grid_cap(dtype):
    """LC_NEST_SUB one element group past 8192 blocks of 512 groups: the
    per-block span grows to 768 groups and the trailing blocks own nothing."""
    n, k = CC.above_cap_shape(dtype)
    case = CC.lincomb_case(n, k, dtype)
    assert case["nspecial"] > 0
    _lincomb_both(CC.LC_NEST_SUB, case, None, {})


def test_lincomb_ignored_operands_may_be_null():
    """A form that does not read y, w, b (or a) takes None / -1 for them, and
    ignores whatever it is handed instead."""
    from krylov_amd import _lib

    case = CC.lincomb_case(1001, 8, CC.F64)
    C = _chain(8, ["a", "b"], cap=2)
    C.set("a", case["a"])
    C.set("b", case["b"])
    stray = _up(np.full((3, 8), 9.0))  # another shape: an ignored operand is not even compared
    a, b = np.ascontiguousarray(case["a"]), np.ascontiguousarray(case["b"])
    for form in CC.FORMS:
        hy = case["y"] if form in CC.NEEDS_Y else None
        hw = case["w"] if form in CC.NEEDS_W else None
        ref = CC.lincomb_ref(form, case["x"], hy, hw, a, b)
        for fill in (False, True):  # the unread operands: null, then present
            dx = _up(case["x"])
            dy = _up(hy) if hy is not None else (stray if fill else None)
            dw = _up(hw) if hw is not None else (stray if fill else None)
            pa = _lib.dptr(a) if (form in CC.NEEDS_A or fill) else None
            pb = _lib.dptr(b) if (form in CC.NEEDS_W or fill) else None
            dz = _up(np.zeros_like(case["x"]))
            _lib.check(_lib.lib.kry_vec_lincomb(_ctx().handle, form, dz.handle, dx.handle, _h(dy), _h(dw), pa, pb))
            _assert_bits(dz.to_host(), ref, ("vec", form, fill))
            ra = C.r["a"] if (form in CC.NEEDS_A or fill) else -1
            rb = C.r["b"] if (form in CC.NEEDS_W or fill) else -1
            dz = _up(np.zeros_like(case["x"]))
            C.begin()
            _lib.check(_lib.lib.kry_prog_lincomb(C.h, form, dz.handle, dx.handle, _h(dy), _h(dw), ra, 1.0, rb, 1.0, 0))
            C.end(0)
            _assert_bits(dz.to_host(), ref, ("prog", form, fill))


def test_lincomb_float32_subnormals():
    """float32 subnormal operands, coefficients and results: the bits of
    NumPy, which keeps subnormals. Separate from the tests above because it
    pins down the device's float32 denormal mode rather than the kernel's
    expression tree."""
    chains = {}
    for name, form, x, y, w, a, b in CC.subnormal_cases():
        case = {"x": x, "y": y, "w": w, "a": a, "b": b}
        ref = CC.lincomb_ref(form, x, y, w, a, b)
        assert CC.is_subnormal(ref).any(), name
        _lincomb_both(form, case, None, chains)


# ------------------------------------------------------------ 2. rowscale
def _rowscale(C, x, d, mul, alias):
    from krylov_amd.device import DeviceVector

    dx, dd = _up(x), _up(d[:, None])
    dz = dx if alias else DeviceVector(_ctx(), x.shape[0], x.shape[1], x.dtype)
    C.begin()
    C.rowscale(mul, dz, dx, dd, 0)
    C.end(0)
    return dz.to_host()


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_rowscale_bitwise(dtype):
    """z = (x.T / d).T and (x.T * d).T, destination apart and in place."""
    chains = {}
    shapes = CC.elementwise_shapes(dtype) + [CC.above_cap_shape(dtype)]
    for n, k in shapes:
        x, d = CC.rowscale_case(n, k, dtype)
        if k not in chains:
            chains[k] = _chain(k, ["a"], cap=2, dtype=dtype)
        C = chains[k]
        big = (n, k) == CC.above_cap_shape(dtype)
        for mul in (0, 1):
            ref = CC.rowscale_ref(x, d, mul)
            for alias in ((False,) if big else (False, True)):
                _assert_bits(_rowscale(C, x, d, mul, alias), ref, ("rowscale", np.dtype(dtype).name, n, k, mul, alias))
        if big:
            _assert_bits(_rowscale(C, x, d, 0, True), CC.rowscale_ref(x, d, 0), ("rowscale in place", n, k))


# ---------------------------------------------------------------- 3. dots
def _dots(x, y, w, chains, prog=True):
    """(kry_dot, kry_prog_dot or None) of the columns of x and y."""
    from krylov_amd import _lib

    k = x.shape[1]
    dx, dy = _up(x), _up(y)
    dw = None if w is None else _up(w[:, None])
    out = np.full(k, -7.0)
    _lib.check(_lib.lib.kry_dot(_ctx().handle, dx.handle, dy.handle, _h(dw), _lib.dptr(out)))
    if not prog:
        return out, None
    if k not in chains:
        chains[k] = _chain(k, ["pad", "d"], cap=2, dtype=x.dtype)
    C = chains[k]
    C.D.w = dw
    C.set("d", np.full(k, -7.0))
    C.begin()
    C.dot(dx, dy, "d", 0)
    C.end(0)
    C.D.w = None
    return out, C.get("d")


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_dots_exact_on_integer_data(dtype):
    """Integer data: the inner products are the exact integer sums whatever
    the order, so a dropped or doubled tail element, a stale partial of an
    empty block or a column mix-up (the column sums are pairwise distinct)
    changes the result. kry_dot for k up to 256, kry_prog_dot up to 64, both
    above the grid cap too, weighted and not; the two agree bit for bit."""
    chains = {}
    shapes = CC.elementwise_shapes(dtype) + list(CC.WIDE_DOT_SHAPES) + [CC.above_cap_shape(dtype)]
    for n, k in shapes:
        c = CC.exact_dot_case(n, k, dtype)
        for w, want in ((None, c["plain"]), (c["w"], c["weighted"])):
            got, got_p = _dots(c["x"], c["y"], w, chains, prog=k <= 64)
            what = (np.dtype(dtype).name, n, k, "weighted" if w is not None else "plain")
            np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=str(what))
            if got_p is not None:
                np.testing.assert_array_equal(CC.bits(got_p), CC.bits(got), err_msg=str(what))


@pytest.mark.parametrize("dtype", CC.DTYPES, ids=lambda d: np.dtype(d).name)
def test_dots_random_data_within_gamma(dtype):
    """|got - exact| <= gamma_{n+2} sum |x w y| (any summation order obeys
    it), kry_prog_dot bitwise kry_dot, and five repeats bitwise equal."""
    chains = {}
    shapes = CC.elementwise_shapes(dtype) + list(CC.WIDE_DOT_SHAPES)
    for n, k in shapes:
        x, y, w = CC.random_dot_case(n, k, dtype)
        for wv in (None, w):
            exact, scale = CC.dot_exact_and_scale(x, y, wv)
            got, got_p = _dots(x, y, wv, chains, prog=k <= 64)
            err = np.abs(got.astype(np.longdouble) - exact)
            bound = CC.gamma(n) * scale
            what = (np.dtype(dtype).name, n, k, "weighted" if wv is not None else "plain")
            assert np.all(err <= bound), (what, float(np.max(err / bound)))
            if got_p is not None:
                np.testing.assert_array_equal(CC.bits(got_p), CC.bits(got), err_msg=str(what))
            if (n, k) in ((100003, 1), (5003, 4), (4099, 64), (1001, 256)):
                for _ in range(4):
                    again, again_p = _dots(x, y, wv, chains, prog=k <= 64)
                    np.testing.assert_array_equal(CC.bits(again), CC.bits(got), err_msg=str(what))
                    if again_p is not None:
                        np.testing.assert_array_equal(CC.bits(again_p), CC.bits(got), err_msg=str(what))


# ------------------------------------------------------- 4. chain control
def test_check_mode4_compares_the_float32_rounded_norm():
    v = 1.0 + 2.0 ** -30
    assert np.float32(v) == np.float32(1.0) and v > 1.0
    C = _chain(4, ["n"], cap=4)
    C.set(None, np.full(4, 1.0))
    C.set("n", np.full(4, v))
    C.begin()
    for st in range(3):
        _check(C, "n", 0, st)
    rows, mid = C.end(3)
    assert mid is None and rows.shape == (3, 4)  # mode 0: 1 + 2^-30 > 1, never stops
    np.testing.assert_array_equal(rows, np.full((3, 4), v))
    C.begin()
    for st in range(3):
        _check(C, "n", 4, st)
    rows, mid = C.end(3)
    assert mid is None and rows.shape == (1, 4)  # rounded to float32 it meets the criterion at step 0
    np.testing.assert_array_equal(CC.bits(rows), CC.bits(np.full((1, 4), v)))  # the row is the unrounded value
    # mode 1 | 4: the same comparison, stopping at the step
    C.begin()
    _check(C, "n", 1, 0)
    _check(C, "n", 5, 1)
    rows, mid = C.end(3)
    assert rows.shape == (1, 4) and mid is not None
    np.testing.assert_array_equal(CC.bits(mid), CC.bits(np.full(4, v)))


@pytest.mark.parametrize("k,bad", [(4, 2), (4, 0), (64, 63), (64, 31)])
def test_check_needs_every_column(k, bad):
    C = _chain(k, ["n"], cap=4)
    crit = np.linspace(1.0, 2.0, k)
    C.set(None, crit)
    ok = crit * 0.5
    ok[::3] = crit[::3]  # equality meets the criterion
    for mode in (0, 1):
        miss = ok.copy()
        miss[bad] = np.nextafter(crit[bad], np.inf)
        C.set("n", miss)
        C.begin()
        for st in range(2):
            _check(C, "n", mode, st)
        rows, mid = C.end(2)
        assert mid is None and len(rows) == 2, (mode, "one column misses: no stop")
        C.set("n", ok)
        C.begin()
        for st in range(2):
            _check(C, "n", mode, st)
        rows, mid = C.end(2)
        if mode == 0:
            assert mid is None and len(rows) == 1
            np.testing.assert_array_equal(rows[0], ok)
        else:
            assert len(rows) == 0 and mid is not None
            np.testing.assert_array_equal(mid, ok)


def test_check_inf_criterion_and_nan_norm():
    C = _chain(4, ["n"], cap=4)
    C.set(None, np.array([1.0, 1.0, 1.0, np.inf]))
    for last in (1e300, np.inf):  # a padded column (+inf) always passes
        C.set("n", np.array([0.5, 0.5, 0.5, last]))
        C.begin()
        _check(C, "n", 0, 0)
        _check(C, "n", 0, 1)
        rows, mid = C.end(2)
        assert len(rows) == 1 and mid is None and rows[0, 3] == last
    for col, crit in ((3, np.inf), (1, 1.0)):  # a NaN norm never stops the chunk, not even under +inf
        nrm = np.array([0.5, 0.5, 0.5, 0.5])
        nrm[col] = np.nan
        C.set("n", nrm)
        for mode in (0, 1, 4, 5):
            C.begin()
            _check(C, "n", mode, 0)
            _check(C, "n", mode, 1)
            rows, mid = C.end(2)
            assert mid is None and len(rows) == 2, (col, mode)
            if mode & 3 == 0:
                assert np.isnan(rows[:, col]).all()


def _ones_and_targets(k, count):
    from krylov_amd.device import DeviceVector

    src = _up(np.full((37, k), 3.0))
    return src, [DeviceVector(_ctx(), 37, k, np.float64) for _ in range(count)]


def test_stop_placement_mode0_and_mode1():
    from krylov_amd import extra

    k = 4
    C = _chain(k, ["n", "m"], cap=4)
    C.set(None, np.full(k, 1.0))
    three, zeros = np.full((37, k), 3.0), np.zeros((37, k))
    # mode 0 succeeds at step 1: the rest of step 1 runs, step 2 does not
    src, (z_same, z_next, z_before) = _ones_and_targets(k, 3)
    C.begin()
    C.sc(extra.SOP_SET, "n", 0, value=5.0)
    _check(C, "n", 0, 0)
    C.lc(extra.LC_COPY, z_before, src, 0)
    C.sc(extra.SOP_SET, "n", 1, value=0.25)
    _check(C, "n", 0, 1)
    C.lc(extra.LC_COPY, z_same, src, 1)
    C.sc(extra.SOP_SET, "n", 2, value=0.125)
    _check(C, "n", 0, 2)
    C.lc(extra.LC_COPY, z_next, src, 2)
    rows, mid = C.end(3)
    assert mid is None
    np.testing.assert_array_equal(rows, np.array([[5.0] * k, [0.25] * k]))
    np.testing.assert_array_equal(z_before.to_host(), three)
    np.testing.assert_array_equal(z_same.to_host(), three)
    np.testing.assert_array_equal(z_next.to_host(), zeros)
    np.testing.assert_array_equal(C.get("n"), np.full(k, 0.25))  # step 2's scalar did not run either
    # mode 1 succeeds at step 1: nothing later in step 1 runs, the row comes apart
    src, (z_same, z_next, z_before) = _ones_and_targets(k, 3)
    C.begin()
    C.sc(extra.SOP_SET, "n", 0, value=5.0)
    _check(C, "n", 0, 0)
    C.sc(extra.SOP_SET, "m", 0, value=4.0)
    _check(C, "m", 1, 0)
    C.lc(extra.LC_COPY, z_before, src, 0)
    C.sc(extra.SOP_SET, "n", 1, value=3.0)
    _check(C, "n", 0, 1)
    C.sc(extra.SOP_SET, "m", 1, value=0.25)
    _check(C, "m", 1, 1)
    C.lc(extra.LC_COPY, z_same, src, 1)
    C.lc(extra.LC_COPY, z_next, src, 2)
    rows, mid = C.end(3)
    assert len(rows) == 1 and mid is not None  # done = 1, midstep = 1
    np.testing.assert_array_equal(rows[0], np.full(k, 5.0))
    np.testing.assert_array_equal(mid, np.full(k, 0.25))  # replaces the row mode 0 wrote at step 1
    np.testing.assert_array_equal(z_before.to_host(), three)
    np.testing.assert_array_equal(z_same.to_host(), zeros)
    np.testing.assert_array_equal(z_next.to_host(), zeros)


@pytest.mark.parametrize("stopped", [True, False])
def test_every_launch_type_is_gated(stopped):
    """In a stopped chunk lincomb, dot, rowscale, spmv and permute leave
    their destination untouched; the same launches in a running chunk (the
    control) write it."""
    import krylov_amd
    from krylov_amd import extra, problems
    from krylov_amd.device import DeviceVector

    k, n = 4, 256
    A = krylov_amd.CsrOperator(problems.poisson2d(16))
    rng = np.random.default_rng(29)
    hx = rng.standard_normal((n, k))
    hd = rng.uniform(1.0, 2.0, n)
    mark = np.full((n, k), 7.0)
    C = _chain(k, ["n", "d"], cap=4)
    C.set(None, np.full(k, 1.0))
    C.set("d", np.full(k, 7.0))
    dx, dd = _up(hx), _up(hd[:, None])
    z = {name: _up(mark) for name in ("lincomb", "rowscale", "spmv", "permute")}
    C.begin()
    C.sc(extra.SOP_SET, "n", 0, value=0.0 if stopped else 2.0)
    _check(C, "n", 0, 0)  # stopped: stop_at = 1
    C.lc(extra.LC_COPY, z["lincomb"], dx, 1)
    C.dot(dx, dx, "d", 1)
    C.rowscale(False, z["rowscale"], dx, dd, 1)
    C.spmv(A, dx, z["spmv"], 1)
    C.permute(A, dx, z["permute"], True, 1)
    rows, mid = C.end(2)
    assert len(rows) == (1 if stopped else 2) and mid is None
    if stopped:
        for name, v in z.items():
            np.testing.assert_array_equal(v.to_host(), mark, err_msg=name)
        np.testing.assert_array_equal(C.get("d"), np.full(k, 7.0))
    else:
        np.testing.assert_array_equal(z["lincomb"].to_host(), hx)
        np.testing.assert_array_equal(z["rowscale"].to_host(), CC.rowscale_ref(hx, hd, 0))
        y = DeviceVector(_ctx(), n, k, np.float64)
        A.matvec_op(dx, y)
        np.testing.assert_array_equal(z["spmv"].to_host(), y.to_host())
        p = DeviceVector(_ctx(), n, k, np.float64)
        A.permute(dx, p, True)
        np.testing.assert_array_equal(z["permute"].to_host(), p.to_host())
        assert np.all(C.get("d") != 7.0)


def test_end_returns_at_most_the_steps_asked_for():
    from krylov_amd import extra

    C = _chain(4, ["n"], cap=8)
    C.set(None, np.full(4, 1.0))
    C.begin()
    for st in range(6):
        C.sc(extra.SOP_SET, "n", st, value=10.0 + st)
        _check(C, "n", 0, st)
    rows, mid = C.end(3)
    assert mid is None and rows.shape == (3, 4)
    np.testing.assert_array_equal(rows[:, 0], [10.0, 11.0, 12.0])
    # a stop inside the asked-for steps still wins
    C.begin()
    for st in range(6):
        C.sc(extra.SOP_SET, "n", st, value=0.5 if st == 1 else 10.0 + st)
        _check(C, "n", 0, st)
    rows, mid = C.end(4)
    assert mid is None and rows.shape == (2, 4)
    # a mode-1 stop at or past the asked-for steps is not reported
    C.begin()
    for st in range(4):
        C.sc(extra.SOP_SET, "n", st, value=0.5 if st == 2 else 10.0)
        _check(C, "n", 1, st)
    rows, mid = C.end(2)
    assert mid is None and rows.shape == (2, 4)


def test_prog_spmv_bitwise_spmv_op():
    import krylov_amd
    from krylov_amd import problems
    from krylov_amd.device import DeviceVector

    A = krylov_amd.CsrOperator(problems.poisson2d(16))
    hx = np.random.default_rng(31).standard_normal((256, 4))
    dx = _up(hx)
    y0, y1 = (DeviceVector(_ctx(), 256, 4, np.float64) for _ in range(2))
    A.matvec_op(dx, y0)
    C = _chain(4, ["n"], cap=2)
    C.begin()
    C.spmv(A, dx, y1, 0)
    C.end(0)
    want = y0.to_host()
    assert np.any(want != 0)
    np.testing.assert_array_equal(CC.bits(y1.to_host()), CC.bits(want))


def test_sop_sqrt_bitwise_numpy():
    from krylov_amd import extra

    rng = np.random.default_rng(37)
    vals = np.concatenate([rng.uniform(0.0, 4.0, 128), 10.0 ** rng.uniform(-300, 300, 120),
                           rng.uniform(1.0, 4.0, 8) * 2.0 ** -1060])  # the last: subnormal doubles
    assert vals.size == 256 and np.all(vals > 0)
    C = _chain(64, ["a", "r"], cap=2)
    for i in range(0, 256, 64):
        C.set("a", vals[i:i + 64])
        C.begin()
        C.sc(extra.SOP_SQRT, "r", 0, a="a")
        C.end(0)
        np.testing.assert_array_equal(CC.bits(C.get("r")), CC.bits(np.sqrt(vals[i:i + 64])))


def test_sop_muldivg_guards_the_product_and_may_alias():
    from krylov_amd import extra

    a = np.array([3.0, -2.0, 5.0, 7.0, 1e-300, -4.0, 0.3, 9.0])
    b = np.array([2.0, 0.7, -1.0, 3.0, 0.1, 6.0, -0.9, 0.0])
    c = np.array([1e-200, 0.0, 4.0, -3.0, 1e-160, 2.0, 0.7, 1.1])
    e = np.array([1e-200, 5.0, 0.0, 0.3, 1e-155, -1.0, 0.1, 1.3])
    den = c * e
    assert den[0] == 0.0 and c[0] != 0 and e[0] != 0  # the product underflows: guarded, though no factor is 0
    assert den[4] != 0.0 and abs(den[4]) < np.finfo(np.float64).tiny  # a subnormal product is not
    want = (a * b) / np.where(den != 0.0, den, 1.0)
    C = _chain(8, ["a", "b", "c", "e", "d"], cap=2)
    for nm, v in (("a", a), ("b", b), ("c", c), ("e", e)):
        C.set(nm, v)
    C.begin()
    C.sc(extra.SOP_MULDIVG, "d", 0, a="a", b="b", c="c", e="e")
    C.end(0)
    np.testing.assert_array_equal(CC.bits(C.get("d")), CC.bits(want))
    for alias in ("a", "b", "c", "e"):  # beta = rho * alpha / ... written over one of its operands
        for nm, v in (("a", a), ("b", b), ("c", c), ("e", e)):
            C.set(nm, v)
        C.begin()
        C.sc(extra.SOP_MULDIVG, alias, 0, a="a", b="b", c="c", e="e")
        C.end(0)
        np.testing.assert_array_equal(CC.bits(C.get(alias)), CC.bits(want), err_msg=alias)


# ------------------------------------------------------------ 5. refusals
def _vec(n, k, dtype=np.float64):
    from krylov_amd.device import DeviceVector

    return DeviceVector(_ctx(), n, k, dtype)


def test_vec_lincomb_refusals():
    from krylov_amd import _lib

    L, ctx = _lib.lib, _ctx().handle
    a, b = np.ones(8), np.ones(8)
    pa, pb = _lib.dptr(a), _lib.dptr(b)
    z, x, y, w = (_vec(10, 8) for _ in range(4))
    for form in (-1, 8, 100):
        assert L.kry_vec_lincomb(ctx, form, z.handle, x.handle, y.handle, w.handle, pa, pb) == _lib.KRY_EINVAL
    for form in CC.FORMS:
        assert L.kry_vec_lincomb(ctx, form, z.handle, x.handle, y.handle, w.handle, pa, pb) == _lib.KRY_OK
        assert L.kry_vec_lincomb(ctx, form, None, x.handle, y.handle, w.handle, pa, pb) == _lib.KRY_EINVAL
        assert L.kry_vec_lincomb(ctx, form, z.handle, None, y.handle, w.handle, pa, pb) == _lib.KRY_EINVAL
        for missing, needed in (("y", CC.NEEDS_Y), ("w", CC.NEEDS_W), ("a", CC.NEEDS_A), ("b", CC.NEEDS_W)):
            args = {"y": y.handle, "w": w.handle, "a": pa, "b": pb}
            args[missing] = None
            rc = L.kry_vec_lincomb(ctx, form, z.handle, x.handle, args["y"], args["w"], args["a"], args["b"])
            assert rc == (_lib.KRY_EINVAL if form in needed else _lib.KRY_OK), (form, missing)
    others = [_vec(11, 8), _vec(10, 4), _vec(10, 8, np.float32)]
    for o in others:  # rows, columns, dtype
        assert L.kry_vec_lincomb(ctx, CC.LC_COPY, o.handle, x.handle, None, None, None, None) == _lib.KRY_EINVAL
        assert L.kry_vec_lincomb(ctx, CC.LC_ADD, z.handle, x.handle, o.handle, None, None, None) == _lib.KRY_EINVAL
        assert L.kry_vec_lincomb(ctx, CC.LC_NEST_ADD, z.handle, x.handle, y.handle, o.handle, pa, pb) == _lib.KRY_EINVAL
    for k in (128, 3):
        zz, xx = _vec(10, k), _vec(10, k)
        ak = np.ones(k)
        rc = L.kry_vec_lincomb(ctx, CC.LC_SCALE, zz.handle, xx.handle, None, None, _lib.dptr(ak), None)
        assert rc == _lib.KRY_EUNSUPPORTED, k


def test_prog_lincomb_refuses_missing_operands():
    """kry_prog_lincomb mirrors kry_vec_lincomb: a form whose y, w, ra or rb
    is missing is KRY_EINVAL and leaves the destination alone (it used to
    compute on uninitialised registers, or divide by a coefficient of 0, and
    return KRY_OK)."""
    from krylov_amd import _lib

    L = _lib.lib
    k = 8
    C = _chain(k, ["a", "b"], cap=2)
    C.set("a", np.full(k, 2.0))
    C.set("b", np.full(k, 3.0))
    mark = np.full((10, k), 7.0)
    x, y, w = (_up(np.full((10, k), v)) for v in (1.0, 4.0, 5.0))
    C.begin()
    for form in CC.FORMS:
        for missing, needed in (("y", CC.NEEDS_Y), ("w", CC.NEEDS_W), ("ra", CC.NEEDS_A), ("rb", CC.NEEDS_W)):
            z = _up(mark)
            args = {"y": y.handle, "w": w.handle, "ra": C.r["a"], "rb": C.r["b"]}
            args[missing] = -1 if missing in ("ra", "rb") else None
            rc = L.kry_prog_lincomb(C.h, form, z.handle, x.handle, args["y"], args["w"], args["ra"], 1.0, args["rb"],
                                    1.0, 0)
            if form in needed:
                assert rc == _lib.KRY_EINVAL, (form, missing)
                np.testing.assert_array_equal(z.to_host(), mark)
            else:
                assert rc == _lib.KRY_OK, (form, missing)
                assert np.all(z.to_host() != 7.0), (form, missing)
    for form in (-1, 8):
        assert L.kry_prog_lincomb(C.h, form, x.handle, x.handle, y.handle, w.handle, 0, 1.0, 1, 1.0, 0) == _lib.KRY_EINVAL
    for reg in (-2, 2):
        assert L.kry_prog_lincomb(C.h, CC.LC_AXPY, x.handle, x.handle, y.handle, None, reg, 1.0, -1, 1.0, 0) == _lib.KRY_EINVAL
    C.end(0)


def test_chain_refusals():
    from krylov_amd import _lib

    L = _lib.lib
    C = _chain(8, ["a", "b"], cap=4)
    C.begin()
    x8, y8, d8 = _vec(10, 8), _vec(10, 8), _vec(10, 1)
    for k in (4, 16):  # vectors whose k differs from the chain's
        x, y, z = _vec(10, k), _vec(10, k), _vec(10, k)
        assert L.kry_prog_dot(C.h, x.handle, y.handle, None, 0, 0) == _lib.KRY_EINVAL
        assert L.kry_prog_lincomb(C.h, CC.LC_ADD, z.handle, x.handle, y.handle, None, -1, 1.0, -1, 1.0, 0) == _lib.KRY_EINVAL
        assert L.kry_prog_rowscale(C.h, 0, z.handle, x.handle, d8.handle, 0) == _lib.KRY_EINVAL
    assert L.kry_prog_dot(C.h, x8.handle, y8.handle, None, 0, 0) == _lib.KRY_OK
    assert L.kry_prog_rowscale(C.h, 1, y8.handle, x8.handle, d8.handle, 0) == _lib.KRY_OK
    assert L.kry_prog_rowscale(C.h, 1, y8.handle, x8.handle, _vec(10, 1, np.float32).handle, 0) == _lib.KRY_EINVAL
    assert L.kry_prog_rowscale(C.h, 1, y8.handle, x8.handle, _vec(9, 1).handle, 0) == _lib.KRY_EINVAL
    for step in (4, 5, 1000, -1):  # step >= cap: past the history
        assert L.kry_prog_check(C.h, 0, 0, step) == _lib.KRY_EINVAL
    assert L.kry_prog_check(C.h, 0, 0, 3) == _lib.KRY_OK
    for mode in (2, 3, 6, 8):
        assert L.kry_prog_check(C.h, 0, mode, 0) == _lib.KRY_EINVAL
    C.end(4)
    for k in (3, 128):
        h = ctypes.c_void_p()
        assert L.kry_prog_create(_ctx().handle, 2, k, 4, ctypes.byref(h)) == _lib.KRY_EUNSUPPORTED
        assert not h.value
