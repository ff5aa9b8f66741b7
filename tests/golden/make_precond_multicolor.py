"""Golden runs of the reference's solvers with the multicolour SSOR and ILU(0)
preconditioners as M / Ml / Mr, made by running the REFERENCE itself, imported
read-only as in make_golden.py. Run only in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_precond_multicolor.py

The preconditioner is the host model of ``ordering="multicolor"``: the
permutation of tests/multicolor_cases.py ``color_py`` around the ``HostPrecond``
of tests/precond_factored_cases.py built on B = A[perm][:, perm]
(``host_precond_mc``). The cases are those of precond_factored_cases.CASES
without the ones that mix a matrix into another slot and without Chebyshev.
Per case, as make_precond_factored.py:
  <name>_resnorms / _numsteps / _success / _xk / _ops   the reference's Info
  <name>_spread   max_k |resnorm_k - variant_k| / resnorm_0 over the same call
                  with a pairwise inner product, and with the preconditioner
                  applied through dense scipy.linalg.solve_triangular

Both variants must take the fixture's step count, a converged case's last two
history entries must stay 1e-6 relative away from the criterion, and the step
counts must be the ones listed in STEPS.

Output: tests/golden/precond_multicolor.npz.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from make_golden import _import_reference, problems  # noqa: E402
from make_precond_factored import _pairwise_inner  # noqa: E402

from tests import multicolor_cases as MC  # noqa: E402
from tests import precond_factored_cases as PC  # noqa: E402

# the reference's step counts with these preconditioners
STEPS = {"cg_p40_ssor": 39, "cg_p40_ilu0": 38, "cg_p40_ssor_block": 63, "cg_p40_ml": 15, "minres_p40_ssor": 39,
         "gmres_r3k_mr": 9, "gmres_r3k_ml": 9, "gmres_r3k_m_mgs2": 20, "bicgstab_r3k_mr": 5, "cgs_r3k_m": 5,
         "f32_cg_p40_ssor": 27}


def cases():
    return [c for c in PC.CASES
            if c[1] != "chebyshev" and not any(isinstance(c[5].get(nm), tuple) for nm in ("M", "Ml", "Mr"))]


def main():
    krylov = _import_reference()
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    assert [c[0] for c in cases()] == list(STEPS)
    for name, solver, slot, spec, key, kw in cases():
        A, b = PC.problem(problems, key)
        P = MC.host_precond_mc(A, spec, A.dtype)
        with quiet, np.errstate(all="ignore"):
            sol, info = PC.call(krylov, solver, A, b, slot, P, kw)
        res = np.asarray(info.resnorms, dtype=np.float64)
        assert info.numsteps == STEPS[name], (name, info.numsteps)
        out[f"{name}_resnorms"] = res
        out[f"{name}_numsteps"] = np.array(info.numsteps)
        out[f"{name}_success"] = np.array(bool(info.success))
        out[f"{name}_xk"] = np.asarray(info.xk)
        ops = info.num_operations
        out[f"{name}_ops"] = (np.full(6, np.nan) if ops is None else
                              np.array([ops[k] for k in ("A", "M", "Ml", "Mr", "inner", "axpy")], dtype=np.float64))
        tol = kw.get("tol", 1e-5)
        if info.success and tol > 0 and info.numsteps > 0:
            crit = np.maximum(tol * res[0], 1e-15)
            for e in (res[-1], res[-2]):
                assert np.all(np.abs(e - crit) > 1e-6 * crit), (name, np.max(np.abs(e - crit) / crit))
        variants = [(P, {"inner": _pairwise_inner}), (MC.host_precond_mc(A, spec, A.dtype, dense=True), {})]
        r0 = float(np.max(res[0]))
        spread = 0.0
        for Pv, extra in variants:
            with quiet, np.errstate(all="ignore"):
                _, iv = PC.call(krylov, solver, A, b, slot, Pv, kw, **extra)
            rv = np.asarray(iv.resnorms, dtype=np.float64)
            assert iv.numsteps == info.numsteps and rv.shape == res.shape, (name, iv.numsteps, info.numsteps)
            spread = max(spread, float(np.max(np.abs(rv - res)) / r0))
        out[f"{name}_spread"] = np.array(spread)
        print(f"{name}: steps {info.numsteps} success {bool(info.success)} spread {spread:.2e}", flush=True)
    path = os.path.join(HERE, "precond_multicolor.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
