"""Block-Jacobi on the device: the factor kernel against the sequential
Gauss-Jordan loop of tests/blockjacobi_cases.py (bitwise), the apply against
the j-ascending block product on the device's own inverses (bitwise), the
refusals, the chain step, and the solvers against the reference's results
with the host model of the same preconditioner
(tests/golden/precond_blockjacobi.npz)."""
import os

import numpy as np
import pytest
import scipy.sparse

from krylov_amd import problems
from tests import blockjacobi_cases as BC
from tests import gpu_helpers as H

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module")
def cases():
    return BC.kernel_cases(problems)


# ----------------------------------------------------------------- factor
@DTYPES
def test_factor_kernel_is_bitwise_the_loop(cases, dtype):
    import krylov_amd

    for name, (A, starts) in cases.items():
        P = krylov_amd.BlockJacobiPreconditioner(A, blocks=starts[:-1], dtype=dtype)
        assert P.blocks.dtype == np.int32 and np.array_equal(P.blocks, starts), name
        got = P.inverse_blocks()
        want = [BC.invert_block_loop(B, dtype) for B in BC.extract_blocks(A, starts, dtype)]
        assert len(got) == len(want) == len(starts) - 1, name
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == dtype and g.shape == w.shape, (name, i)
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} block {i} of {w.shape[0]} rows")
        lay = P.layout()
        sizes = np.diff(starts)
        assert lay["blocks"] == len(sizes) and lay["block_sizes"] == (int(sizes.min()), int(sizes.max())), name
        assert lay["value_bytes"] == int(np.sum(sizes.astype(np.int64) ** 2)) * np.dtype(dtype).itemsize
        assert lay["launches"] == 1 and lay["factor_kernel_seconds"] >= 0.0


def test_uniform_partitions_and_single_rows(cases):
    import krylov_amd

    md, _ = cases["multidof12x4_b4"]
    P = krylov_amd.BlockJacobiPreconditioner(md, block_size=5)
    assert np.array_equal(P.blocks, BC.uniform_starts(md.shape[0], 5)) and P.blocks[-1] - P.blocks[-2] == 1
    rn, _ = cases["b1"]
    for dtype in (np.float64, np.float32):
        P = krylov_amd.BlockJacobiPreconditioner(rn, block_size=1, dtype=dtype)
        inv = np.array([X[0, 0] for X in P.inverse_blocks()])
        np.testing.assert_array_equal(_bits(inv), _bits(dtype(1) / rn.diagonal().astype(dtype)))
    dense, _ = cases["dense70_b32"]
    P = krylov_amd.BlockJacobiPreconditioner(dense, block_size=32)
    assert [X.shape[0] for X in P.inverse_blocks()] == [32, 32, 6]
    assert P.factored and P.max_cols == 256 and P.solve_kind == "exact"


def test_partition_refusals():
    import krylov_amd

    A = problems.poisson2d(8)
    with pytest.raises(NotImplementedError, match="at most 32"):
        krylov_amd.BlockJacobiPreconditioner(A, block_size=33)
    with pytest.raises(NotImplementedError, match=r"block 1 \(from row 4\) has 60 rows"):
        krylov_amd.BlockJacobiPreconditioner(A, blocks=[0, 4])
    with pytest.raises(ValueError, match="start at row 0"):
        krylov_amd.BlockJacobiPreconditioner(A, blocks=[2, 4])
    with pytest.raises(ValueError, match="increase strictly"):
        krylov_amd.BlockJacobiPreconditioner(A, blocks=[0, 8, 8, 16, 32, 48])
    with pytest.raises(ValueError, match="past the last row"):
        krylov_amd.BlockJacobiPreconditioner(A, blocks=[0, 32, 64])
    with pytest.raises(ValueError, match="exactly one"):
        krylov_amd.BlockJacobiPreconditioner(A)
    with pytest.raises(ValueError, match="exactly one"):
        krylov_amd.BlockJacobiPreconditioner(A, block_size=4, blocks=[0])
    with pytest.raises(ValueError, match="block_size"):
        krylov_amd.BlockJacobiPreconditioner(A, block_size=0)
    with pytest.raises(ValueError, match="square"):
        krylov_amd.BlockJacobiPreconditioner(scipy.sparse.csr_matrix(np.ones((4, 6))), block_size=2)
    with pytest.raises(TypeError, match="complex"):
        krylov_amd.BlockJacobiPreconditioner(A.astype(np.complex128), block_size=2)


def test_singular_blocks_name_the_smallest(cases):
    import krylov_amd

    A, starts = cases["mixed"]
    D = A.tolil()
    for blk in (40, 9):  # two singular blocks: a zero row inside the block
        s, e = int(starts[blk]), int(starts[blk + 1])
        D[s + 1, s:e] = 0.0
    D = D.tocsr()
    with pytest.raises(np.linalg.LinAlgError, match=rf"block 9 \(from row {int(starts[9])}\)"):
        krylov_amd.BlockJacobiPreconditioner(D, blocks=starts[:-1])
    with pytest.raises(np.linalg.LinAlgError, match=r"block 0 \(from row 0\)"):
        krylov_amd.BlockJacobiPreconditioner(np.array([[1.0, 2.0], [2.0, 4.0]]), block_size=2)
    with pytest.raises(np.linalg.LinAlgError, match=r"block 1 \(from row 1\)"):
        krylov_amd.BlockJacobiPreconditioner(np.diag([1.0, np.inf, 2.0]), block_size=1)


# ------------------------------------------------------------------ apply
@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["f64", "f32"])
def applied(request, cases):
    """name -> (P, starts, the device's inverses, x of 256 columns, apply_loop of it), once per dtype."""
    import krylov_amd

    dtype = request.param
    out = {}
    for name in ("mixed", "multidof12x4_b4"):
        A, starts = cases[name]
        P = krylov_amd.BlockJacobiPreconditioner(A, blocks=starts[:-1], dtype=dtype)
        inv = P.inverse_blocks()
        x = np.random.default_rng(3).standard_normal((A.shape[0], 256)).astype(dtype)
        out[name] = (P, starts, inv, x, BC.apply_loop(inv, starts, x))
    return dtype, out


@pytest.mark.parametrize("k", [1, 2, 3, 8, 64, 128, 256])
def test_apply_is_bitwise_the_loop(applied, k):
    dtype, objs = applied
    for name, (P, starts, inv, x, want) in objs.items():
        xs = x[:, 0] if k == 1 else x[:, :k]
        got = P @ xs
        assert got.dtype == dtype and got.shape == xs.shape, name
        # column c of a k-column apply is the single-column apply: the loop's value for that column
        np.testing.assert_array_equal(_bits(got), _bits(want[:, 0] if k == 1 else want[:, :k]), err_msg=f"{name} k={k}")


def test_apply_in_place_poison_and_width(applied):
    from krylov_amd.device import DeviceVector

    dtype, objs = applied
    for name, (P, starts, inv, x, want) in objs.items():
        n = x.shape[0]
        for k in (1, 8):
            v = DeviceVector.from_host(P.ctx, x[:, :k], dtype=dtype)
            P.matvec_device(v, v)  # y aliases x
            np.testing.assert_array_equal(_bits(v.to_host()), _bits(want[:, :k]), err_msg=f"{name} in place k={k}")
        blk = 7
        s, e = int(starts[blk]), int(starts[blk + 1])
        z = x[:, :4].copy()
        z[s + (e - s) // 2, 2] = np.inf
        with np.errstate(all="ignore"):
            wz = BC.apply_loop(inv, starts, z)
        gz = P @ z
        assert np.array_equal(gz, wz, equal_nan=True)  # NaN for NaN, whatever its sign and payload
        bad = ~np.isfinite(gz)
        np.testing.assert_array_equal(_bits(gz[~bad]), _bits(wz[~bad]))
        assert bad[s:e, 2].all() and bad.sum() == e - s, name
        with pytest.raises(NotImplementedError, match="256 right-hand-side columns"):
            P @ np.ones((n, 257), dtype=dtype)
        assert P.layout()["launches"] == 1


def test_chain_step_is_the_direct_apply(cases):
    """kry_prog_precond (what bicgstab's Ml= enqueues) is bitwise
    kry_precond_apply, and writes nothing in a stopped chunk."""
    import krylov_amd
    from krylov_amd import _helpers, extra

    A, starts = cases["mixed"]
    n = A.shape[0]
    Y = np.random.default_rng(8).standard_normal((n, 4))
    P = krylov_amd.BlockJacobiPreconditioner(A, blocks=starts[:-1])
    want = BC.apply_loop(P.inverse_blocks(), starts, Y)
    np.testing.assert_array_equal(_bits(P.solve(Y)), _bits(want))
    prob = _helpers.Problem(A, Y, None, None, Ml=P)
    assert not prob.A.renumbered
    D = extra._Dev(prob)
    C = extra._Chain(D, ["n"], cap=4)
    yv, xv = D.upload(Y), D.zeros()
    C.begin()
    assert C.apply("Ml", yv, xv, 0) is xv
    C.end(1)
    np.testing.assert_array_equal(_bits(xv.to_host()), _bits(want))
    zv = D.zeros()
    C.set(None, np.full(4, 1.0))
    C.begin()
    C.sc(extra.SOP_SET, "n", 0, value=0.0)
    C.check("n", 0)
    C.apply("Ml", D.upload(Y), zv, 1)
    rows, _ = C.end(2)
    assert len(rows) == 1
    np.testing.assert_array_equal(zv.to_host(), np.zeros((n, 4)))


def test_other_refusals():
    import krylov_amd
    from krylov_amd import _lib
    from krylov_amd._lib import check, lib

    A = problems.multidof(4, 4)
    n = A.shape[0]
    with pytest.raises(TypeError, match="CsrOperator"):
        krylov_amd.BlockJacobiPreconditioner(krylov_amd.CsrOperator(A), block_size=4)
    P32 = krylov_amd.BlockJacobiPreconditioner(A, block_size=4, dtype=np.float32)
    with pytest.raises(ValueError, match="dtype="):
        krylov_amd.cg(A, np.ones(n), M=P32)
    P = krylov_amd.BlockJacobiPreconditioner(A, block_size=4)
    with pytest.raises(NotImplementedError, match="devices="):
        krylov_amd.cg(A, np.ones((n, 2)), M=P, devices=[0])
    with pytest.raises(ValueError, match="shape"):
        krylov_amd.cg(problems.multidof(3, 4), np.ones(36), M=P)
    op = krylov_amd.CsrOperator(A)

    class Renumbered:
        renumbered = True

        def __getattr__(self, name):
            return getattr(op, name)

    import krylov_amd._helpers as helpers

    orig = helpers.as_device_operator
    helpers.as_device_operator = lambda a, **kw: Renumbered()
    try:
        with pytest.raises(NotImplementedError, match="KRY_RENUMBER=0"):
            helpers.Problem(A, np.ones(n), None, None, M=P)
    finally:
        helpers.as_device_operator = orig
    # the stage is the only one of its preconditioner
    S = krylov_amd.SsorPreconditioner(A)
    with pytest.raises(ValueError, match="only stage"):
        check(lib.kry_precond_add_bjacobi(S.handle, P._bj))
    sv = krylov_amd.device.DeviceVector.from_host(P.ctx, np.ones((n, 1)), dtype=np.float64)
    with pytest.raises(ValueError, match="no other stage"):
        check(lib.kry_precond_add_scale(P.handle, sv.handle))
    check(lib.kry_precond_fuse(P.handle))  # a no-op
    assert P.layout()["launches"] == 1 and not P.layout()["fused"]
    assert _lib.lib.kry_version() >= 113


# ----------------------------------------------------------------- parity
@pytest.fixture(scope="module")
def fixtures():
    return np.load(os.path.join(HERE, "golden", "precond_blockjacobi.npz"))


@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c[0])
def test_parity_with_the_reference(fixtures, case):
    """Step count and success equal; history within 1e-10 * want_k +
    2 * spread * want_0 (1e-4 * want_k for the float32 case, whose tolerance
    is 1e-4; bicgstab with the absolute floor 1e-14 ||r_0|| of
    tests/test_gpu_precond.py)."""
    import krylov_amd

    name, solver, slot, key, bs, cols, kw = case
    A, b = BC.problem(problems, key, cols)
    P = krylov_amd.BlockJacobiPreconditioner(A, block_size=bs, dtype=A.dtype)
    _, info = getattr(krylov_amd, solver)(A, b, **{slot: P}, **kw)
    rtol = 1e-4 if name.startswith("f32_") else 1e-10
    want = fixtures[name + "_resnorms"]
    got = np.asarray(info.resnorms, dtype=np.float64)
    print(name, "steps", info.numsteps, int(fixtures[name + "_numsteps"]), "spread", float(fixtures[name + "_spread"]))
    assert info.numsteps == int(fixtures[name + "_numsteps"])
    assert bool(info.success) == bool(fixtures[name + "_success"])
    assert got.shape == want.shape
    w0 = np.max(np.abs(want[0]))
    floor = 1e-14 * w0 if solver == "bicgstab" else 0.0
    bound = rtol * np.abs(want) + H.NOISE_FACTOR * float(fixtures[name + "_spread"]) * w0 + floor
    err = np.abs(got - want)
    print(name, "largest fraction of the bound used", float(np.max(err / bound)), "at", int(np.argmax(err / bound)))
    assert np.all(err <= bound), (float(np.max(err / bound)), int(np.argmax(err / bound)))
