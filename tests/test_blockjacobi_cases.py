"""The block-Jacobi loops of tests/blockjacobi_cases.py against the properties
that define them, the host-only plan of the factor kernel (kry_bjacobi_plan)
and the teeth of the parity cases. No device."""
import os

import numpy as np
import pytest

from krylov_amd import problems
from tests import blockjacobi_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_model_inverts(dtype):
    """Over the 240 blocks of block_suite (sizes 1 to 32, SPD and shifted
    random), componentwise |B X - I| <= c b eps |B| |X| with c four times the
    same ratio of numpy.linalg.inv on the same blocks in the same dtype
    (Gauss-Jordan's right residual is modestly larger than LU's). Measured,
    largest ratio over the suite: the loop 1.876 (fp64) and 1.546 (fp32),
    numpy.linalg.inv 0.639 (fp64) and 0.440 (fp32), the residuals taken in
    extended precision."""
    suite = BC.block_suite(dtype)
    assert len(suite) == 240 and {B.shape[0] for _, B in suite} == set(BC.SUITE_SIZES)
    model = ref = 0.0
    for name, B in suite:
        X = BC.invert_block_loop(B, dtype)
        assert X.dtype == dtype and np.all(np.isfinite(X)), name
        model = max(model, BC.right_residual_ratio(B, X))
        ref = max(ref, BC.right_residual_ratio(B, np.linalg.inv(B).astype(dtype)))
    print(np.dtype(dtype).name, "largest |B X - I| / (b eps |B||X|): loop", model, "numpy.linalg.inv", ref)
    assert ref > 0.0
    assert model <= 4.0 * ref, (model, ref)


def test_pivoting():
    P = np.array([[0.0, 1.0], [1.0, 0.0]])
    X, piv = BC.invert_block_loop(P, np.float64, return_piv=True)
    np.testing.assert_array_equal(X, P)
    assert list(piv) == [1, 1]
    # equal magnitudes: the smaller row index is the pivot
    _, piv = BC.invert_block_loop(np.array([[1.0, 2.0], [-1.0, 1.0]]), np.float64, return_piv=True)
    assert list(piv) == [0, 1]
    _, piv = BC.invert_block_loop(np.array([[1.0, 2.0, 0.0], [-2.0, 1.0, 1.0], [2.0, 0.0, 1.0]]), np.float32,
                                  return_piv=True)
    assert piv[0] == 1
    with pytest.raises(np.linalg.LinAlgError):
        BC.invert_block_loop(np.array([[1.0, 2.0], [2.0, 4.0]]), np.float64)
    with pytest.raises(np.linalg.LinAlgError):
        BC.invert_block_loop(np.array([[np.inf]]), np.float64)
    one = BC.invert_block_loop(np.array([[3.0]]), np.float32)
    assert one.dtype == np.float32 and one[0, 0] == np.float32(1) / np.float32(3)
    for b in (2, 5, 8, 17, 32):  # every step of an anti-diagonal-dominant block swaps
        _, piv = BC.invert_block_loop(BC.antidiagonal_block(b, b), np.float64, return_piv=True)
        assert all(piv[c] == max(c, b - 1 - c) for c in range(b))


def test_apply_loop_is_the_block_product():
    A, starts = BC.mixed_matrix(problems)
    P = BC.HostBlockJacobi(A, starts, np.float64)
    x = np.random.default_rng(3).standard_normal((A.shape[0], 3))
    y = P @ x
    for i, X in enumerate(P.inverses):
        s, e = starts[i], starts[i + 1]
        np.testing.assert_allclose(y[s:e], X @ x[s:e], rtol=1e-12, atol=1e-12 * np.max(np.abs(y[s:e])))
    np.testing.assert_array_equal((P @ x[:, 1]), y[:, 1])  # a column does not depend on the others
    x[starts[4] + 1, 0] = np.inf  # poisons block 4, column 0, and nothing else
    z = P @ x
    bad = ~np.isfinite(z)
    assert bad[starts[4]:starts[5], 0].all() and bad.sum() == starts[5] - starts[4]


# -------------------------------------------------------------------- plan
def _check_plan(n, starts):
    from krylov_amd import _lib

    plan = _lib.bjacobi_plan(n, starts)
    sizes = np.diff(np.concatenate([starts, [n]]))
    tasks, blocklist = plan["tasks"], plan["blocklist"]
    assert sorted(blocklist.tolist()) == list(range(len(starts)))  # every block in exactly one task
    assert plan["max_block"] == sizes.max() and plan["min_block"] == sizes.min()
    assert plan["values"] == int(np.sum(sizes.astype(np.int64) ** 2))
    covered = 0
    for t, (first, count, g) in enumerate(tasks.tolist()):
        assert first == covered and 1 <= count <= 64 // g and g in (4, 8, 16, 32)
        covered += count
        for blk in blocklist[first:first + count]:
            b = int(sizes[blk])
            assert b <= g and (g == 4 or b > g // 2)  # the smallest class that holds it
        last_of_class = t + 1 == len(tasks) or tasks[t + 1][2] != g
        assert count == 64 // g or last_of_class
    assert covered == len(starts)
    gs = tasks[:, 2]
    assert np.all(np.diff(gs) >= 0)  # by class
    for g in set(gs.tolist()):  # inside a class the blocks ascend
        members = np.concatenate([blocklist[f:f + c] for f, c, gg in tasks.tolist() if gg == g])
        assert np.all(np.diff(members) > 0)
    return plan


def test_plan_covers_every_block_once():
    """Fails on a library without kry_bjacobi_plan."""
    starts = BC.mixed_starts()
    plan = _check_plan(int(starts[-1]), starts[:-1])
    # 5 blocks of each size: classes of 20 (g = 4), 15 (8), 15 (16), 15 (32) blocks: partial last tasks everywhere
    assert [(int(g), int(np.sum(plan["tasks"][plan["tasks"][:, 2] == g][:, 1]))) for g in (4, 8, 16, 32)] == \
        [(4, 20), (8, 15), (16, 15), (32, 15)]
    assert plan["tasks"][:, 1].tolist() == [16, 4, 8, 7, 4, 4, 4, 3] + [2] * 7 + [1]
    _check_plan(1, np.array([0], dtype=np.int32))
    _check_plan(2304, BC.uniform_starts(2304, 4)[:-1])  # 576 blocks of 4: 36 full tasks
    p = _check_plan(2304, BC.uniform_starts(2304, 5)[:-1])
    assert p["min_block"] == 4 and p["max_block"] == 5
    p = _check_plan(70, BC.uniform_starts(70, 32)[:-1])
    assert p["tasks"].tolist() == [[0, 1, 8], [1, 2, 32]]  # the block of 6, then the two of 32


def test_plan_refuses_malformed_partitions():
    from krylov_amd import _lib

    def plan(n, starts):
        return _lib.bjacobi_plan(n, np.array(starts, dtype=np.int32))

    with pytest.raises(ValueError, match="start at row 0"):
        plan(10, [1, 5])
    with pytest.raises(ValueError, match="increase strictly"):
        plan(10, [0, 4, 4])
    with pytest.raises(ValueError, match="increase strictly"):
        plan(10, [0, 6, 3])
    with pytest.raises(ValueError, match="past the last row"):
        plan(10, [0, 4, 10])
    with pytest.raises(ValueError):
        plan(10, [])
    with pytest.raises(NotImplementedError, match=r"block 1 \(from row 4\) has 33 rows"):
        plan(50, [0, 4, 37])
    with pytest.raises(NotImplementedError, match=r"block 2 .* has 40 rows"):
        plan(50, [0, 4, 10])
    assert plan(36, [0, 4])["max_block"] == 32


# ------------------------------------------------------------------- teeth
@pytest.mark.parametrize("case", BC.CASES, ids=lambda c: c[0])
def test_parity_cases_tell_block_jacobi_from_less(case):
    """The reference's step count with block-Jacobi differs from its count
    without a preconditioner and from its count with diag(A)^-1 in the same
    slot, so a device that applied the identity or only the diagonal fails the
    parity test's step count. A case that runs to its maxiter (the 20 fixed
    steps of the 128-column case; GMRES with maxiter 30, which ends there
    unconverged with or without a preconditioner) has one count by
    construction: there the last residual norms of the three runs differ by
    more than a tenth in every column, a thousand times the parity bound."""
    name = case[0]
    d = np.load(os.path.join(HERE, "golden", "precond_blockjacobi.npz"))
    steps = int(d[name + "_numsteps"])
    if not bool(d[name + "_success"]):
        assert steps == case[6]["maxiter"]
        last = d[name + "_resnorms"][-1]
        for other in ("none", "jacobi"):
            assert int(d[f"{name}_{other}_numsteps"]) == steps
            o = d[f"{name}_{other}_last"]
            assert np.all(np.abs(o - last) > 0.1 * np.maximum(np.abs(o), np.abs(last)))
        return
    assert steps != int(d[name + "_none_numsteps"])
    assert steps != int(d[name + "_jacobi_numsteps"])
