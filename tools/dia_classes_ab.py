"""A/B of the descriptor classes of the SELL-128/DIA image on the metric CG
(15-point stencil 216^3, bench.run_cg_bench: 5 timed regions of 200
iterations after 20 warm-up steps, then the event pass for the SpMV's launch
time), alternating, in one call on one card:

    python tools/dia_classes_ab.py ROUNDS NAME[:KEY=VALUE,...] ...

e.g. `2 classes off:KRY_DIA_CLASSES=0 parent:TREE=build_ab/parent
cap4096:KRY_DIA_GRID=4096`. KEY=VALUE pairs are environment variables of the
variant's process, except TREE: a checkout of another commit with its library
built, whose package and bench.py the variant then imports instead of this
tree's (the parent commit: its binding does not know this build's entry
points, so its library cannot be loaded through KRYLOV_LIB). The matrix is
built once on the host; every variant of every round runs in a fresh child
process (forked before anything touches the GPU, so the library and its
switches, which are read once per process, are the child's own), one at a
time, under a time limit. The first child that fails or overruns ends the run.
One line per child: NAME round ms_per_step median (min - max) spmv_ms it/s,
the operator's class count and the seconds kry_csr_create took."""
import importlib.util
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 150


def _problems():
    # krylov_amd/problems.py on its own: importing the package loads the library
    spec = importlib.util.spec_from_file_location("_problems", os.path.join(ROOT, "krylov_amd", "problems.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _child(A, env, q):
    env = dict(env)
    tree = os.path.abspath(env.pop("TREE", ROOT))
    os.environ.update(env)
    sys.path.insert(0, tree)
    import numpy as np

    import bench

    assert os.path.dirname(os.path.abspath(bench.__file__)) == tree
    r = bench.run_cg_bench(A, lambda _r: np.ones(A.shape[0]), 200, 20, bench.Job.single(), repeats=5)
    ms = [1e3 * e / 200 for e in r["elapsed_all"]]
    # the operator upload (kry_csr_create), as bench.py's end_to_end leg times it: median of 3
    import time

    import krylov_amd

    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        op = krylov_amd.CsrOperator(A)
        op.ctx.synchronize()
        ts.append(time.perf_counter() - t0)
        del op
    q.put({"ms": ms, "spmv_ms": 1e3 * r["spmv_avg_s"], "dia_classes": r["layout"].get("dia_classes"),
           "csr_create_s": sorted(ts)[1]})


def main():
    rounds = int(sys.argv[1])
    variants = []
    for spec in sys.argv[2:]:
        name, _, envs = spec.partition(":")
        variants.append((name, dict(kv.split("=", 1) for kv in envs.split(",") if kv)))
    A = _problems().stencil15_3d(216)
    mp = multiprocessing.get_context("fork")
    out = []
    for rnd in range(rounds):
        for name, env in variants:
            q = mp.Queue()
            p = mp.Process(target=_child, args=(A, env, q))
            p.start()
            p.join(LIMIT_S)
            if p.is_alive():
                p.kill()
                p.join()
                sys.exit(f"{name}: over {LIMIT_S} s, stopping")
            if p.exitcode != 0:
                sys.exit(f"{name}: exit {p.exitcode}, stopping")
            r = q.get(timeout=10)
            ms = sorted(r["ms"])
            med = ms[len(ms) // 2]
            print(f"{name:12s} {rnd + 1} ms_per_step {med:.4f} ({ms[0]:.4f} - {ms[-1]:.4f}) "
                  f"spmv_ms {r['spmv_ms']:.4f} it/s {1e3 / med:.0f} classes={r['dia_classes']} "
                  f"csr_create_s={r['csr_create_s']:.4f}", flush=True)
            out.append({"name": name, "round": rnd + 1, **r})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
