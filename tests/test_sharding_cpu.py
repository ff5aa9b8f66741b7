"""RHS-column sharding on CPU: the product's host code over gloo.

``krylov_amd.shard`` is the rank bookkeeping and the outer loop of
``krylov_amd.distributed`` (the layout of every rank's columns in the global
per-column vectors, the zero-padded allreduce, the global criterion with its
+inf padding, the explicit-residual recheck, the global history). Here it
runs exactly as on GPUs, with the device solver state replaced by a host
engine restating the device step (tests/shard_engines.py) and RCCL by gloo,
at world sizes 2, 3 and 4. The reference couples a block's columns only
through ``np.all(resnorms[-1] <= criterion)`` (cg.py:156,162, gmres.py:193,
minres.py:162) and the invariance test (arnoldi.py:187, 270-272), so the
sharded solve must reproduce the reference's own unsharded block fixtures.
"""
import os
import socket
import threading

import numpy as np
import pytest

from tests import golden_io

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo(rank, world, port):
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(v):
        t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).copy())
        dist.all_reduce(t)
        return t.numpy().copy()

    return dist, allreduce


def _worker(rank, world, port, outdir, which):
    import sys

    sys.path.insert(0, REPO)
    dist, allreduce = _gloo(rank, world, port)
    from krylov_amd import problems
    from krylov_amd.shard import ShardLayout, drive
    from tests import shard_engines as E

    d = golden_io.load("solvers")
    out = {}
    if which == "cg":
        P = problems.poisson2d(64)
        B = d["poisson64_B"]
        kl = B.shape[1] // world
        lay = ShardLayout(kl, kl, rank, world)
        eng = E.HostCG(P, B[:, rank * kl:(rank + 1) * kl], lay, allreduce)
        out["success"], out["k"], res = drive(eng, lay, allreduce, 1e-8, 1e-15, P.shape[0], np.float64)
        out["res"], out["x"] = np.array(res), eng.xk()
    elif which == "cg_uneven":
        # 8 columns over 3 ranks as krylov_amd.multi splits them: 3 device
        # columns each, the last rank's third a zero column outside the layout
        P = problems.poisson2d(64)
        B = d["poisson64_B"]
        kcs = [3, 3, 2]
        Bl = B[:, 3 * rank:3 * rank + kcs[rank]]
        if kcs[rank] < 3:
            Bl = np.concatenate([Bl, np.zeros((B.shape[0], 3 - kcs[rank]))], axis=1)
        lay = ShardLayout(3, 3, rank, world, kcs)
        eng = E.HostCG(P, Bl, lay, allreduce)
        out["success"], out["k"], res = drive(eng, lay, allreduce, 1e-8, 1e-15, P.shape[0], np.float64)
        out["res"], out["x"] = np.array(res), eng.xk()[:, :kcs[rank]]
    elif which == "gmres":
        R = problems.random_nonsym(5000)
        B = d["rand5k_B3"]
        lay = ShardLayout(1, 1, rank, world)
        eng = E.HostGMRES(R, B[:, [rank]], lay, allreduce, 20)
        out["success"], out["k"], res = drive(eng, lay, allreduce, 0.0, 1e-15, 20, np.float64)
        out["res"], out["x"] = np.array(res), eng.xk()
        # a tolerance at which the columns converge at different steps: the
        # global rule keeps every rank going until the slowest column is done
        eng = E.HostGMRES(R, B[:, [rank]], lay, allreduce, 60)
        out["tol_success"], out["tol_k"], res = drive(eng, lay, allreduce, 1e-6, 1e-15, 60, np.float64)
        out["tol_res"] = np.array(res)
    else:
        P = problems.poisson2d(32)
        B = np.random.default_rng(3).standard_normal((P.shape[0], world))
        B[:, 1] *= 1e-3
        lay = ShardLayout(1, 1, rank, world)
        eng = E.HostMINRES(P, B[:, [rank]], lay, allreduce)
        out["success"], out["k"], res = drive(eng, lay, allreduce, 1e-8, 1e-15, P.shape[0], np.float64)
        out["res"], out["x"] = np.array(res), eng.xk()
    np.savez(os.path.join(outdir, f"{which}{rank}.npz"), **out)
    dist.destroy_process_group()


def _spawn(tmp_path, which, world):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), which), nprocs=world, join=True)
    return [np.load(tmp_path / f"{which}{r}.npz") for r in range(world)]


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_cg_reproduces_block_cg_bitwise(tmp_path, world):
    """8 columns over 2 or 4 ranks: the reference's block-CG fixture bit for
    bit (the per-column recurrences are independent; sharding changes no bit)."""
    d = golden_io.load("solvers")
    outs = _spawn(tmp_path, "cg", world)
    for o in outs:
        assert bool(o["success"]) and int(o["k"]) == int(d["cg_poisson64_blk8_numsteps"])
        np.testing.assert_array_equal(o["res"], d["cg_poisson64_blk8_resnorms"])  # global history on every rank
    np.testing.assert_array_equal(np.concatenate([o["x"] for o in outs], axis=1), d["cg_poisson64_blk8_xk"])


def test_sharded_cg_uneven_split_reproduces_block_cg(tmp_path):
    """8 columns over 3 ranks (3 + 3 + 2 real, the last rank padded with a zero
    column that the layout leaves out of the history and the stop rule, as
    krylov_amd.multi splits a block): the block-CG fixture bit for bit."""
    d = golden_io.load("solvers")
    outs = _spawn(tmp_path, "cg_uneven", 3)
    for o in outs:
        assert bool(o["success"]) and int(o["k"]) == int(d["cg_poisson64_blk8_numsteps"])
        np.testing.assert_array_equal(o["res"], d["cg_poisson64_blk8_resnorms"])
    np.testing.assert_array_equal(np.concatenate([o["x"] for o in outs], axis=1), d["cg_poisson64_blk8_xk"])


def test_sharded_gmres_global_rules(tmp_path):
    from krylov_amd import problems
    from oracle import krylov_ref

    world = 3
    outs = _spawn(tmp_path, "gmres", world)
    d = golden_io.load("solvers")
    R = problems.random_nonsym(5000)
    _, blk = krylov_ref.gmres(R, d["rand5k_B3"], maxiter=60, tol=1e-6)
    ref_res = np.asarray(d["gmres_rand5k_blk3_resnorms"])
    for r, o in enumerate(outs):
        assert int(o["k"]) == int(d["gmres_rand5k_blk3_numsteps"]) and not bool(o["success"])
        np.testing.assert_allclose(o["res"], ref_res, rtol=1e-12)  # global history on every rank
        np.testing.assert_allclose(o["x"][:, 0], d["gmres_rand5k_blk3_xk"][:, r], rtol=1e-9, atol=1e-12)
        assert bool(o["tol_success"]) and int(o["tol_k"]) == blk.numsteps  # the slowest column decides
        ref = np.asarray(blk.resnorms)
        np.testing.assert_allclose(o["tol_res"][:-1], ref[:-1], rtol=1e-12)
        # the final entry is the explicit residual: compared absolutely
        np.testing.assert_allclose(o["tol_res"][-1], ref[-1], rtol=0, atol=1e-12 * ref[0].max())


def test_sharded_minres_global_rules(tmp_path):
    from krylov_amd import problems
    from oracle import krylov_ref

    world = 2
    outs = _spawn(tmp_path, "minres", world)
    P = problems.poisson2d(32)
    B = np.random.default_rng(3).standard_normal((P.shape[0], world))
    B[:, 1] *= 1e-3
    _, blk = krylov_ref.minres(P, B, tol=1e-8)
    ref = np.asarray(blk.resnorms)
    for r, o in enumerate(outs):
        assert bool(o["success"]) and int(o["k"]) == blk.numsteps
        np.testing.assert_allclose(o["res"][:-1], ref[:-1], rtol=1e-12)
        np.testing.assert_allclose(o["res"][-1], ref[-1], rtol=0, atol=1e-12 * ref[0].max())
        np.testing.assert_allclose(o["x"][:, 0], blk.xk[:, r], rtol=1e-10, atol=1e-13)


# ------------------------------------------------------------- layout units
def test_shard_layout_padding_and_global_vectors():
    """3 real columns padded to 4 on each of 3 ranks: real slots, the
    zero-padded all-gather, and +inf criterion on the padded slots."""
    from krylov_amd.shard import ShardLayout

    lays = [ShardLayout(3, 4, r, 3) for r in range(3)]
    np.testing.assert_array_equal(lays[0].real, [0, 1, 2, 4, 5, 6, 8, 9, 10])
    assert lays[2].off == 8 and lays[2].total == 12
    parts = [lay.glob(np.array([r + 0.5, r + 1.5, r + 2.5, 99.0]), lambda v: v) for r, lay in enumerate(lays)]
    summed = np.sum(parts, axis=0)
    np.testing.assert_array_equal(summed[lays[0].real], [0.5, 1.5, 2.5, 1.5, 2.5, 3.5, 2.5, 3.5, 4.5])
    crit = lays[1].criterion_full(np.arange(9.0))
    np.testing.assert_array_equal(crit[lays[1].real], np.arange(9.0))
    assert np.all(np.isinf(crit[[3, 7, 11]]))
    with pytest.raises(ValueError):
        ShardLayout(2, 1, 0, 2)
    # an uneven split: rank r's first kcs[r] device columns are real
    lu = ShardLayout(3, 4, 1, 3, kcs=[3, 3, 2])
    np.testing.assert_array_equal(lu.real, [0, 1, 2, 4, 5, 6, 8, 9])
    assert np.all(np.isinf(lu.criterion_full(np.zeros(8))[[3, 7, 10, 11]]))
    with pytest.raises(ValueError):
        ShardLayout(3, 4, 0, 3, kcs=[3, 4, 1])


def test_file_rendezvous_threads(tmp_path):
    """The torch-free unique-id exchange: rank 0 publishes, others poll."""
    from krylov_amd.shard import file_rendezvous

    path = str(tmp_path / "uid")
    payload = os.urandom(128)
    got = [None] * 4

    def rank(r):
        got[r] = file_rendezvous(path, r, lambda: payload, timeout=20)

    ts = [threading.Thread(target=rank, args=(r,)) for r in (3, 2, 1, 0)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(g == payload for g in got)
    with pytest.raises(TimeoutError):
        file_rendezvous(str(tmp_path / "never"), 1, lambda: b"", timeout=0.2)
