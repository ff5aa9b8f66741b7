#!/usr/bin/env python
"""Rates of gauss_seidel / ssor / chebyshev and of the sparse triangular solve
they stand on, beside the same iteration on the host, as one JSON line.

    python tools/bench_stationary.py [--out FILE] [--small]

Workloads: poisson2d(1000) (1,999 thin levels) and random_nonsym(2_000_000)
(about 60 fat levels), b = ones. Per workload:
  tri_lower / tri_upper   the triangular solve alone (k = 1): ms per call from
        HIP events around a region of back-to-back solves, its levels,
        launches and image bytes, and image bytes / time as a fraction of
        8 TB/s (the matrix stream alone: x and y add 16 n bytes)
  <solver>.iters_per_s    device iterations per second: the difference of two
        whole calls of K_LONG and K_SHORT iterations (tol = 0), so uploads, the
        host analysis and the downloads cancel
  <solver>.host_iters_per_s   the same iteration with scipy
        (spsolve_triangular + csr_matvec), timed in this run on this machine;
        scipy's two kernels are serial whatever the thread count
Every figure is the median of REGIONS timed regions after a warm-up.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve_triangular

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS = 5
K_SHORT, K_LONG = 8, 40
HBM = 8.0e12


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def time_tri(op, n, dtype):
    from krylov_amd.device import DeviceVector

    y = DeviceVector.from_host(op.ctx, np.ones((n, 1)), dtype=dtype)
    x = DeviceVector(op.ctx, n, 1, dtype)
    for _ in range(2):
        op.solve_device(y, x)
    op.ctx.synchronize()
    reps = 10
    ms = []
    for _ in range(REGIONS):
        op.ctx.timer_start()
        for _ in range(reps):
            op.solve_device(y, x)
        ms.append(op.ctx.timer_stop() / reps)
    lay = op.layout()
    t = median(ms) * 1e-3
    return {"ms_per_call": median(ms), "ms_regions": [round(m, 4) for m in ms], "levels": lay["levels"],
            "launches": lay["launches"], "slices": lay["slices"], "slots": lay["slots"], "image_bytes": lay["bytes"],
            "fraction_of_8TBps": lay["bytes"] / t / HBM}


def time_solver(fn, short, long_):
    fn(long_)  # warm-up: code objects, the operator's upload (cached afterwards)
    per = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        fn(short)
        t1 = time.perf_counter()
        fn(long_)
        t2 = time.perf_counter()
        per.append(((t2 - t1) - (t1 - t0)) / (long_ - short))
    return 1.0 / median(per), per


def host_rate(step, its=3):
    step()
    per = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(its):
            step()
        per.append((time.perf_counter() - t0) / its)
    return 1.0 / median(per)


def workload(name, A, bounds):
    import krylov_amd

    A = sp.csr_matrix(A)
    n = A.shape[0]
    b = np.ones(n)
    out = {"n": n, "nnz": int(A.nnz)}
    L, U = sp.tril(A).tocsr(), sp.triu(A).tocsr()
    for key, T, lower in (("tri_lower", L, True), ("tri_upper", U, False)):
        op = krylov_amd.TriangularOperator(T, lower=lower)
        out[key] = time_tri(op, n, np.float64)
        op.close()
    d = A.diagonal()
    Ls, Us = (sp.tril(A, -1) + sp.diags(d)).tocsr(), (sp.triu(A, 1) + sp.diags(d)).tocsr()
    state = {"x": np.zeros(n), "r": b.copy(), "p": np.zeros(n)}

    def host_gs():
        state["x"] += spsolve_triangular(L, state["r"], lower=True)
        state["r"] = b - A @ state["x"]

    def host_ssor():
        y = spsolve_triangular(Ls, state["r"], lower=True)
        y = y * d
        state["x"] += spsolve_triangular(Us, y, lower=False)
        state["r"] = b - A @ state["x"]

    def host_cheb():
        state["p"] = state["r"] + 0.25 * state["p"]
        state["x"] += 0.1 * state["p"]
        state["r"] -= 0.1 * (A @ state["p"])

    solvers = {
        "gauss_seidel": (lambda k: krylov_amd.gauss_seidel(A, b, tol=0.0, maxiter=k), host_gs),
        "ssor": (lambda k: krylov_amd.ssor(A, b, tol=0.0, maxiter=k), host_ssor),
        "chebyshev": (lambda k: krylov_amd.chebyshev(A, b, bounds, tol=0.0, maxiter=k), host_cheb),
    }
    for sname, (dev, host) in solvers.items():
        with np.errstate(all="ignore"):
            rate, per = time_solver(dev, K_SHORT, K_LONG)
            state.update(x=np.zeros(n), r=b.copy(), p=np.zeros(n))
            hrate = host_rate(host)
        out[sname] = {"iters_per_s": rate, "host_iters_per_s": hrate, "speedup": rate / hrate,
                      "s_per_iter_regions": [round(p, 6) for p in per]}
        print(f"{name} {sname}: device {rate:.1f} it/s, host {hrate:.2f} it/s", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    from krylov_amd import _lib, problems

    if _lib.device_count() < 1:
        raise SystemExit("bench_stationary needs a GPU: it measures nothing without one")
    m, n = (60, 20_000) if args.small else (1000, 2_000_000)
    res = {"bench": "stationary", "regions": REGIONS, "k_short": K_SHORT, "k_long": K_LONG,
           "host_threads_env": os.environ.get("OMP_NUM_THREADS"), "build_id": _lib.build_id(), "workloads": {}}
    lo = 8 * np.sin(np.pi / (2 * (m + 1))) ** 2
    res["workloads"][f"poisson2d({m})"] = workload("poisson2d", problems.poisson2d(m), (lo, 8 - lo))
    R = problems.random_nonsym(n)
    dmax = float(np.abs(R.diagonal()).max())
    res["workloads"][f"random_nonsym({n})"] = workload("random_nonsym", R, (0.1 * dmax, 2.0 * dmax))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
