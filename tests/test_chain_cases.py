"""Host-only checks of tests/chain_cases.py: the conditions that keep the
device tests of tests/test_gpu_chain_ops.py from passing vacuously. No kernel
is launched here."""
import math

import numpy as np
import pytest

from tests import chain_cases as CC


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_tail_shapes_end_in_a_partial_group(dtype):
    W = CC.width(dtype)
    assert W == {8: 2, 4: 4}[np.dtype(dtype).itemsize]
    shapes = CC.tail_shapes(dtype)
    assert len(shapes) == (6 if W == 2 else 9)
    for n, k in shapes:
        assert k < W and (n * k) % W != 0, (n, k)
    # one group alone, one tail behind full blocks, and every remainder mod W
    assert {(n * k) % W for n, k in shapes} == set(range(1, W))
    assert any(n * k < W for n, k in shapes)
    assert any(CC.launch_geometry(n * k, dtype)[1] > 1 for n, k in shapes)


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_boundary_shapes_straddle_whole_blocks(dtype):
    W = CC.width(dtype)
    shapes = CC.boundary_shapes(dtype)
    assert len(shapes) == 12 and len(set(shapes)) == 12
    for g in (1, 2, 3):
        full = CC.GROUPS_PER_BLOCK * W * g  # elements of g whole blocks
        near = [n for n, k in shapes if abs(n - full) <= W]
        assert sorted(n - full for n in near) == [-W, -1, 1, W]
        grids = set()
        for N in near:
            ngrp, grid, per, empty = CC.launch_geometry(N, dtype)
            assert per == CC.GROUPS_PER_BLOCK and empty is None
            assert abs(ngrp - CC.GROUPS_PER_BLOCK * g) <= 1
            grids.add(grid)
        assert grids == {g, g + 1}  # the last block full to the brim, and one group into the next
    assert all(k == 1 for _, k in shapes)


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_column_shapes_fill_groups_and_blocks(dtype):
    W = CC.width(dtype)
    assert sorted({k for _, k in CC.COLUMN_SHAPES}) == [2, 4, 8, 16, 64]
    for n, k in CC.COLUMN_SHAPES:
        assert k & (k - 1) == 0 and k <= 64
        assert n % 2 == 1  # odd row counts: the last group of a k < W block is a tail
        _, grid, per, empty = CC.launch_geometry(n * k, dtype)
        assert per <= CC.GROUPS_PER_BLOCK and empty is None
    assert any(CC.launch_geometry(n * k, dtype)[1] > 1 for n, k in CC.COLUMN_SHAPES)
    for n, k in CC.WIDE_DOT_SHAPES:
        assert k in (128, 256) and CC.launch_geometry(n * k, dtype)[3] is None
    assert {k for _, k in CC.WIDE_DOT_SHAPES} == {128, 256}
    shapes = CC.elementwise_shapes(dtype)
    assert len(shapes) == len(set(shapes))
    assert set(shapes) == set(CC.tail_shapes(dtype)) | set(CC.boundary_shapes(dtype)) | set(CC.COLUMN_SHAPES)
    # every other shape stays under the cap, so only above_cap_shape reaches that regime
    for n, k in list(shapes) + list(CC.WIDE_DOT_SHAPES):
        assert CC.launch_geometry(n * k, dtype)[0] <= CC.MAX_GRID * CC.GROUPS_PER_BLOCK


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_above_cap_shape_grows_the_span_and_empties_blocks(dtype):
    W = CC.width(dtype)
    n, k = CC.above_cap_shape(dtype)
    N = n * k
    cap = CC.MAX_GRID * CC.GROUPS_PER_BLOCK * W  # elements of a full grid of 512-group blocks
    assert cap < N <= cap + CC.GROUPS_PER_BLOCK * W  # the smallest excess: under one block's worth
    ngrp, grid, per, empty = CC.launch_geometry(N, dtype)
    assert grid == CC.MAX_GRID
    assert per > CC.GROUPS_PER_BLOCK and per % CC.BLOCK_THREADS == 0
    assert per == CC.GROUPS_PER_BLOCK + CC.BLOCK_THREADS
    assert empty is not None and empty < grid  # trailing blocks own empty spans
    assert per * (empty - 1) < ngrp <= per * empty
    assert N * np.dtype(dtype).itemsize < 68e6
    assert k == 64


# ----------------------------------------------------------------- lincomb
@pytest.mark.parametrize("dtype", CC.DTYPES)
@pytest.mark.parametrize("form", [CC.LC_AXPY, CC.LC_NEST_ADD, CC.LC_NEST_SUB])
def test_lincomb_data_shows_a_fused_multiply_add(form, dtype):
    """A contracted last step must change at least 10 % of the elements."""
    shapes = [s for s in CC.elementwise_shapes(dtype) if s[0] * s[1] >= 1000]
    assert len(shapes) >= 15
    for n, k in shapes:
        c = CC.lincomb_case(n, k, dtype)
        plain, fused = CC.fused_last_step(form, c["x"], c["y"], c["w"], c["a"], c["b"], sample=1500)
        assert len(plain) >= 900
        frac = float(np.mean(CC.bits(plain) != CC.bits(fused)))
        print(f"form {form} {np.dtype(dtype).name} ({n}, {k}): fused last step changes {100 * frac:.1f} %")
        assert frac >= 0.10, (form, dtype, n, k, frac)


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_lincomb_coefficients_and_specials(dtype):
    sp = CC.specials(dtype)
    for n, k in CC.elementwise_shapes(dtype) + [(129, 16)]:
        c = CC.lincomb_case(n, k, dtype)
        av, bv = c["a"].astype(dtype), c["b"].astype(dtype)
        both = np.concatenate([av, bv, -av, -bv])
        assert len(set(both.tolist())) == 4 * k  # a wrong column or a swapped a / b shows, under either sign
        if np.dtype(dtype) == CC.F32:
            assert np.all(av.astype(np.float64) != c["a"])  # the cast to V rounds
        m = len(sp)
        if n * k >= 2 * m * m:
            assert c["nspecial"] == m * m
            pairs = {(xb, yb) for xb, yb in zip(CC.bits(c["x"]).reshape(-1)[: m * m].tolist(),
                                                CC.bits(c["y"]).reshape(-1)[: m * m].tolist())}
            assert len(pairs) == m * m
            assert set(CC.bits(c["w"]).reshape(-1)[: m * m].tolist()) == set(CC.bits(sp).tolist())
        else:
            assert c["nspecial"] == 0
    # the references of the special block hold NaNs and non-NaNs, signed zeros included
    c = CC.lincomb_case(5003, 4, dtype)
    z = CC.lincomb_ref(CC.LC_SUB, c["x"], c["y"], None, None, None).reshape(-1)[: c["nspecial"]]
    assert np.isnan(z).any() and np.isinf(z).any()
    zb = set(CC.bits(z).tolist())
    assert int(CC.bits(np.array([0.0], dtype=dtype))[0]) in zb and int(CC.bits(np.array([-0.0], dtype=dtype))[0]) in zb


def test_lincomb_ref_stays_in_the_vectors_dtype():
    c = CC.lincomb_case(1001, 8, CC.F32)
    for form in CC.FORMS:
        z = CC.lincomb_ref(form, c["x"], c["y"], c["w"], c["a"], c["b"])
        assert z.dtype == np.float32
    # the float64 coefficient is rounded before it multiplies
    z = CC.lincomb_ref(CC.LC_SCALE, c["x"], None, None, c["a"], None)
    with np.errstate(all="ignore"):
        promoted = (c["a"] * c["x"].astype(np.float64)).astype(np.float32)
    assert np.any(CC.bits(z) != CC.bits(promoted))


def test_lincomb_combination_count():
    per_form = {f: len(CC.aliases(f)) for f in CC.FORMS}
    assert per_form == {0: 3, 1: 4, 2: 4, 3: 2, 4: 4, 5: 4, 6: 2, 7: 2}
    assert len(CC.lincomb_combinations(CC.F64)) == 25 * len(CC.elementwise_shapes(CC.F64))
    assert len(CC.lincomb_combinations(CC.F32)) == 25 * len(CC.elementwise_shapes(CC.F32))


def test_subnormal_cases_are_subnormal():
    seen = set()
    for name, form, x, y, w, a, b in CC.subnormal_cases():
        assert x.dtype == y.dtype == w.dtype == np.float32
        z = CC.lincomb_ref(form, x, y, w, a, b)
        assert np.mean(CC.is_subnormal(z)) >= 0.25, name  # subnormal results
        if "coefficient" in name:
            assert CC.is_subnormal(a.astype(np.float32)).all()
        else:
            assert np.mean(CC.is_subnormal(x)) >= 0.5 and CC.is_subnormal(y).all() and CC.is_subnormal(w).all()
        # flushing inputs or results to zero would change the result
        flushed = np.where(CC.is_subnormal(z), np.copysign(np.float32(0), z), z)
        assert np.any(CC.bits(flushed) != CC.bits(z))
        seen.add(form)
    assert seen == set(CC.FORMS)


# ---------------------------------------------------------------- rowscale
@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_rowscale_divisors_expose_a_reciprocal_multiply(dtype):
    x, d = CC.rowscale_case(5003, 4, dtype)
    assert d.dtype == x.dtype and np.all(d != 0) and np.any(d < 0)
    q = CC.rowscale_ref(x, d, 0)
    r = (x.T * (np.ones(1, dtype=dtype) / d)).T
    frac = float(np.mean(CC.bits(q) != CC.bits(np.ascontiguousarray(r))))
    print(f"{np.dtype(dtype).name}: x * (1 / d) differs from x / d in {100 * frac:.1f} % of the elements")
    assert frac > 0.01  # not vacuous; nothing is measured against this figure
    mant, _ = np.frexp(np.abs(d))
    assert np.mean(mant != 0.5) > 0.99  # powers of two are the exception


# -------------------------------------------------------------------- dots
@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_exact_dot_data_is_exact_in_any_order(dtype):
    rng = np.random.default_rng(5)
    shapes = CC.elementwise_shapes(dtype) + list(CC.WIDE_DOT_SHAPES)
    for n, k in shapes:
        c = CC.exact_dot_case(n, k, dtype)
        x, y, w = c["x"], c["y"], c["w"]
        assert np.all(x == np.rint(x)) and np.all(np.abs(x) <= 8) and np.all(np.abs(y) <= 8)
        assert set(w.tolist()) <= {1.0, 2.0, 4.0}
        for wv, want in ((None, c["plain"]), (w, c["weighted"])):
            assert len(set(want.tolist())) == k  # pairwise distinct column sums
            ww = np.ones(n) if wv is None else wv
            terms = x.astype(np.float64) * (ww[:, None] * y.astype(np.float64))
            assert float(np.abs(terms).sum(axis=0).max()) < 2.0 ** 53  # bounds every partial sum in every order
            np.testing.assert_array_equal(terms.sum(axis=0), want.astype(np.float64))
            for _ in range(3):
                p = rng.permutation(n)
                seq = np.zeros(k)
                for row in terms[p] if n <= 2100 else ():
                    seq = seq + row
                if n <= 2100:
                    np.testing.assert_array_equal(seq, want.astype(np.float64))
                np.testing.assert_array_equal(terms[p].sum(axis=0), want.astype(np.float64))
            if n * k <= 300000:
                assert CC.dot_fsum(x, y, wv) == [float(v) for v in want]


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_above_cap_exact_dot_data(dtype):
    n, k = CC.above_cap_shape(dtype)
    c = CC.exact_dot_case(n, k, dtype)
    assert len(set(c["plain"].tolist())) == k and len(set(c["weighted"].tolist())) == k
    assert n * 8 * 8 * 4 < 2 ** 53
    terms = c["x"].astype(np.float64) * (c["w"][:, None] * c["y"].astype(np.float64))
    np.testing.assert_array_equal(terms.sum(axis=0), c["weighted"].astype(np.float64))
    np.testing.assert_array_equal(terms[::-1].sum(axis=0), c["weighted"].astype(np.float64))


@pytest.mark.parametrize("dtype", CC.DTYPES)
def test_gamma_bound_holds_for_pairwise_and_sequential_sums(dtype):
    for n, k in [(100003, 1), (5003, 4), (1025, 1)]:
        x, y, w = CC.random_dot_case(n, k, dtype)
        assert x.dtype == np.dtype(dtype)
        for wv in (None, w):
            exact, scale = CC.dot_exact_and_scale(x, y, wv)
            ww = np.ones(n) if wv is None else wv
            terms = x.astype(np.float64) * (ww[:, None] * y.astype(np.float64))  # the device's x * (w * y)
            pairwise = np.sum(terms, axis=0)
            seq = np.zeros(k)
            for row in terms:
                seq = seq + row
            g = CC.gamma(n)
            assert 0 < g < 1e-10
            for got in (pairwise, seq):
                err = np.abs(got.astype(np.longdouble) - exact)
                assert np.all(err <= g * scale), (n, k, float(err.max()), float((g * scale).min()))
            # the bound is not slack by orders of magnitude beyond its n: a float32 sum misses it
            if k == 1:
                low = np.float64(np.sum(terms.astype(np.float32), axis=0)[0])
                assert abs(np.longdouble(low) - exact[0]) > g * scale[0]


def test_gamma_is_the_stated_formula():
    u = 2.0 ** -53
    assert CC.gamma(1000) == 1002 * u / (1 - 1002 * u)
    assert math.isclose(CC.gamma(1), 3 * u, rel_tol=1e-12)
