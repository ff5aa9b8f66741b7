#!/usr/bin/env python
"""Cost and effect of the factorised preconditioners (SsorPreconditioner,
Ilu0Preconditioner) as one JSON line.

    python tools/bench_precond.py [--out FILE] [--small]

Workloads: poisson2d(1000) (SPD, 1,999 thin levels) and
random_nonsym(2_000_000) (nonsymmetric, fat levels), b = ones. Every
preconditioner runs in natural order (ssor, ilu0) and in the multicolour order
(ssor_mc, ilu0_mc: ordering="multicolor") in the same run, and in natural order
with its two solves replaced by approximate-inverse products (solve="isai")
without and with one relaxation sweep (ssor_isai, ssor_isai_s1, ilu0_isai,
ilu0_isai_s1). Per workload: spmv_ms, one A x on a device vector, timed like an
apply. Per workload and preconditioner:
  setup_s        the constructor, whole (host analysis, uploads, images)
  factor_s       ILU(0) only: kry_ilu0_factor (analysis, upload, the
                 factorisation kernels, the values' way back)
  isai_s, isai_kernel_s, image_s   solve="isai" only: the two krylov_amd.isai
                 calls (checks, transposes, upload, kernel, the values' way
                 back), of that the two kry_isai_lower kernels alone (HIP
                 events), and the device images of W (and T with sweeps)
  ms_per_apply   one P r on a device vector (k = 1): HIP events around a
                 region of back-to-back applies (5, or as many as fill 20 ms),
                 median of REGIONS regions
  stages         levels / launches of every stage
  launches, fused, colors   kernel launches per apply, whether the apply is the
                 fused one, the number of colours (null in natural order)
and per solver (cg on the SPD workload, gmres(30) = gmres_restarted on both)
without a preconditioner and with each one (cg: M; gmres: Mr):
  steps, success, wall_s   iterations and host wall time of one whole call to
                 tol = 1e-8 (after a two-step call that loads the code objects
                 and caches the operator's upload), capped at MAX_CG steps /
                 MAX_CYCLES cycles
The block-Jacobi leg (BlockJacobiPreconditioner; --bjacobi runs it alone,
--no-bjacobi leaves it out) is a section of its own, "bjacobi": on
multidof(700, 4) (n = 1.96 M, several unknowns per node) CG without a
preconditioner, with the point-Jacobi matrix diag(A)^-1 as M and with
block_size=4; on poisson2d(1000) the same with block_size=8; on
random_nonsym(2_000_000) gmres(30) without, with diag(A)^-1 and with
block_size=8 as Mr. Per workload spmv_ms; per preconditioner setup_s (the
constructor), factor_s (kry_bjacobi_create: plan, uploads, kernels),
factor_kernel_s (the factor kernels alone, HIP events), ms_per_apply as above
(the point-Jacobi matrix: its SpMV), blocks, block_sizes, value_bytes; per
solve steps, success, wall_s, once with b = ones ("solves", as the other legs)
and once with b = default_rng(3).standard_normal(n) ("solves_rng3", the
right-hand side of the parity cases).
No threshold is attached: the tool records what it measures.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REGIONS = 5
TOL = 1e-8
MAX_CG = 6000
MAX_CYCLES = 40
RESTART = 30


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def time_apply(P):
    """P: a preconditioner or a CsrOperator (the SpMV beside the applies)."""
    from krylov_amd.device import DeviceVector

    y = DeviceVector.from_host(P.ctx, np.ones((P.n, 1)), dtype=P.dtype)
    x = DeviceVector(P.ctx, P.n, 1, P.dtype)
    for _ in range(2):
        P.matvec_device(y, x)
    P.ctx.synchronize()
    P.ctx.timer_start()
    P.matvec_device(y, x)
    reps = int(min(2000, max(5, np.ceil(20.0 / max(P.ctx.timer_stop(), 1e-3)))))
    ms = []
    for _ in range(REGIONS):
        P.ctx.timer_start()
        for _ in range(reps):
            P.matvec_device(y, x)
        ms.append(P.ctx.timer_stop() / reps)
    return median(ms), [round(m, 4) for m in ms]


def build(name, make):
    t0 = time.perf_counter()
    P = make()
    out = {"setup_s": time.perf_counter() - t0}
    if hasattr(P, "factor_seconds"):
        out["factor_s"] = P.factor_seconds
    if hasattr(P, "isai_seconds"):
        out["isai_s"], out["isai_kernel_s"], out["image_s"] = P.isai_seconds, P.isai_kernel_seconds, P.image_seconds
    out["ms_per_apply"], out["ms_regions"] = time_apply(P)
    lay = P.layout()
    if "factor" in lay:
        out["factor_plan"] = lay["factor"]
    if lay["solve"] == "isai":
        out["stages"] = [{"sweeps": s["sweeps"], "scale": s["scale"],
                          "image": [k for k in ("dia", "col_blocks", "pair", "rs") if s["isai"][k]]}
                         for s in lay["stages"]]
    else:
        out["stages"] = [{k: s[k] for k in ("levels", "launches") if k in s} or s for s in lay["stages"]]
    out["solve"], out["sweeps"] = lay["solve"], lay["sweeps"]
    out["launches"], out["fused"], out["colors"] = lay["launches"], lay["fused"], lay["colors"]
    print(f"  {name}: setup {out['setup_s']:.2f} s, apply {out['ms_per_apply']:.3f} ms", file=sys.stderr, flush=True)
    return P, out


def solve_cg(A, b, M):
    import krylov_amd

    krylov_amd.cg(A, b, M=M, tol=0.0, maxiter=2)
    t0 = time.perf_counter()
    _, info = krylov_amd.cg(A, b, M=M, tol=TOL, maxiter=MAX_CG)
    return {"steps": int(info.numsteps), "success": bool(info.success), "wall_s": time.perf_counter() - t0,
            "final_relres": float(np.max(info.resnorms[-1]) / np.max(info.resnorms[0]))}


def solve_gmres(A, b, Mr):
    import krylov_amd

    krylov_amd.gmres_restarted(A, b, restart=2, tol=0.0, max_cycles=1, Mr=Mr)
    t0 = time.perf_counter()
    _, infos = krylov_amd.gmres_restarted(A, b, restart=RESTART, tol=TOL, max_cycles=MAX_CYCLES, Mr=Mr)
    wall = time.perf_counter() - t0
    first = float(np.max(infos[0].resnorms[0]))
    return {"steps": int(sum(i.numsteps for i in infos)), "cycles": len(infos), "success": bool(infos[-1].success),
            "wall_s": wall, "final_relres": float(np.max(infos[-1].resnorms[-1])) / first}


def build_bjacobi(name, A, bs):
    import krylov_amd

    t0 = time.perf_counter()
    P = krylov_amd.BlockJacobiPreconditioner(A, block_size=bs)
    out = {"setup_s": time.perf_counter() - t0, "factor_s": P.factor_seconds,
           "factor_kernel_s": P.factor_kernel_seconds}
    out["ms_per_apply"], out["ms_regions"] = time_apply(P)
    lay = P.layout()
    out.update({k: lay[k] for k in ("blocks", "block_sizes", "value_bytes", "map_bytes", "launches")})
    print(f"  {name}: setup {out['setup_s']:.2f} s, factor kernel {out['factor_kernel_s'] * 1e3:.3f} ms, "
          f"apply {out['ms_per_apply']:.3f} ms", file=sys.stderr, flush=True)
    return P, out


def workload_bjacobi(name, A, spd, bs):
    """none / point Jacobi / block-Jacobi on one matrix: cg (M) on an SPD one,
    gmres(30) (Mr) otherwise."""
    import krylov_amd
    import scipy.sparse

    n = A.shape[0]
    b = np.ones(n)
    out = {"n": n, "nnz": int(A.nnz), "block_size": bs, "precond": {}, "solves": {}}
    out["spmv_ms"], _ = time_apply(krylov_amd.as_device_operator(A))
    t0 = time.perf_counter()
    J = scipy.sparse.diags(1.0 / A.diagonal(), format="csr")
    Jop = krylov_amd.CsrOperator(J, like=krylov_amd.as_device_operator(A))
    out["precond"]["jacobi"] = {"setup_s": time.perf_counter() - t0}
    out["precond"]["jacobi"]["ms_per_apply"], out["precond"]["jacobi"]["ms_regions"] = time_apply(Jop)
    P, out["precond"][f"bjacobi{bs}"] = build_bjacobi(f"{name} bjacobi{bs}", A, bs)
    sname, fn = ("cg", solve_cg) if spd else (f"gmres({RESTART})", solve_gmres)
    # b = ones as in the other legs, and the right-hand side of the parity cases (tests/blockjacobi_cases.py)
    for key, rhs in (("solves", b), ("solves_rng3", np.random.default_rng(3).standard_normal(n))):
        out[key] = {}
        for pname, M in (("none", None), ("jacobi", J), (f"bjacobi{bs}", P)):
            with np.errstate(all="ignore"):
                try:
                    r = fn(A, rhs, M)
                except Exception as e:  # recorded, not hidden
                    r = {"error": f"{type(e).__name__}: {e}"}
            out[key][f"{sname}/{pname}"] = r
            print(f"  {name} {key} {sname}/{pname}: {r}", file=sys.stderr, flush=True)
    return out


def workload(name, A, spd):
    import krylov_amd

    n = A.shape[0]
    b = np.ones(n)
    out = {"n": n, "nnz": int(A.nnz), "precond": {}, "solves": {}}
    precs = {"none": None}
    out["spmv_ms"], _ = time_apply(krylov_amd.as_device_operator(A))
    isai = {"solve": "isai"}
    for pname, make in (("ssor", lambda: krylov_amd.SsorPreconditioner(A, omega=1.0)),
                        ("ilu0", lambda: krylov_amd.Ilu0Preconditioner(A)),
                        ("ssor_mc", lambda: krylov_amd.SsorPreconditioner(A, omega=1.0, ordering="multicolor")),
                        ("ilu0_mc", lambda: krylov_amd.Ilu0Preconditioner(A, ordering="multicolor")),
                        ("ssor_isai", lambda: krylov_amd.SsorPreconditioner(A, omega=1.0, **isai)),
                        ("ssor_isai_s1", lambda: krylov_amd.SsorPreconditioner(A, omega=1.0, sweeps=1, **isai)),
                        ("ilu0_isai", lambda: krylov_amd.Ilu0Preconditioner(A, **isai)),
                        ("ilu0_isai_s1", lambda: krylov_amd.Ilu0Preconditioner(A, sweeps=1, **isai))):
        try:
            precs[pname], out["precond"][pname] = build(pname, make)
        except Exception as e:  # recorded, not hidden: e.g. a singular pivot
            out["precond"][pname] = {"error": f"{type(e).__name__}: {e}"}
    solvers = ([("cg", solve_cg)] if spd else []) + [(f"gmres({RESTART})", solve_gmres)]
    for sname, fn in solvers:
        for pname, P in precs.items():
            with np.errstate(all="ignore"):
                try:
                    r = fn(A, b, P)
                except Exception as e:
                    r = {"error": f"{type(e).__name__}: {e}"}
            out["solves"][f"{sname}/{pname}"] = r
            print(f"  {name} {sname}/{pname}: {r}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--bjacobi", action="store_true", help="the block-Jacobi leg alone")
    ap.add_argument("--no-bjacobi", action="store_true", help="everything but the block-Jacobi leg")
    args = ap.parse_args()
    from krylov_amd import _lib, problems

    if _lib.device_count() < 1:
        raise SystemExit("bench_precond needs a GPU: it measures nothing without one")
    m, n = (60, 20_000) if args.small else (1000, 2_000_000)
    res = {"bench": "precond", "regions": REGIONS, "tol": TOL, "max_cg": MAX_CG, "max_cycles": MAX_CYCLES,
           "restart": RESTART, "build_id": _lib.build_id(), "workloads": {}}
    if not args.bjacobi:
        res["workloads"][f"poisson2d({m})"] = workload("poisson2d", problems.poisson2d(m), True)
        res["workloads"][f"random_nonsym({n})"] = workload("random_nonsym", problems.random_nonsym(n), False)
    if not args.no_bjacobi:
        md = 40 if args.small else 700
        res["bjacobi"] = {
            f"multidof({md}, 4)": workload_bjacobi("multidof", problems.multidof(md, 4), True, 4),
            f"poisson2d({m})": workload_bjacobi("poisson2d", problems.poisson2d(m), True, 8),
            f"random_nonsym({n})": workload_bjacobi("random_nonsym", problems.random_nonsym(n), False, 8),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
