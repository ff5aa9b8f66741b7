"""A/B of builds and environment switches on the metric CG (15-point stencil
216^3, bench.run_cg_bench: 5 timed regions of 200 iterations after 20 warm-up
steps, then the event pass for the SpMV's launch time), alternating, in one
call on one card:

    python tools/dia_lean_ab.py ROUNDS NAME[:KEY=VALUE,...] ...

e.g. `2 lean old:KRY_DIA_LEAN=0 parent:KRYLOV_LIB=build_ab/libkrylov_hip.so
cap4096:KRY_DIA_GRID=4096`. The matrix is built once on the host; every
variant of every round runs in a fresh child process (forked before anything
touches the GPU, so the library and its switches, which are read once per
process, are the child's own), one at a time, under a time limit. The first
child that fails or overruns ends the run. One line per child:
NAME round ms_per_step median (min - max) spmv_ms it/s."""
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
    os.environ.update(env)
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench

    r = bench.run_cg_bench(A, lambda _r: np.ones(A.shape[0]), 200, 20, bench.Job.single(), repeats=5)
    ms = [1e3 * e / 200 for e in r["elapsed_all"]]
    q.put({"ms": ms, "spmv_ms": 1e3 * r["spmv_avg_s"], "dia_lean": r["layout"].get("dia_lean")})


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
                  f"spmv_ms {r['spmv_ms']:.4f} it/s {1e3 / med:.0f} lean={r['dia_lean']}", flush=True)
            out.append({"name": name, "round": rnd + 1, **r})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
