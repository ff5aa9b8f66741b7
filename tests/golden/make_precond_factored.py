"""Golden runs of the reference's solvers with factorised preconditioners
(SSOR, ILU(0)) as M / Ml / Mr, made by running the REFERENCE itself, imported
read-only as in make_golden.py. Run only in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_precond_factored.py

The preconditioners are plain Python objects whose ``@`` goes through scipy
``spsolve_triangular`` (tests/precond_factored_cases.py HostPrecond), the way
the reference's users write them; the ILU(0) factors come from the sequential
loop ``ilu0_loop`` there. The cases are listed in
tests/precond_factored_cases.py (the tests regenerate the inputs from the same
generators; only outputs are stored). Per case:
  <name>_resnorms / _numsteps / _success / _xk / _ops   the reference's Info
  <name>_spread   the case's own spread: max_k |resnorm_k - variant_k| /
                  resnorm_0 over the same reference call made with a pairwise
                  inner product, and with the preconditioner applied through
                  dense scipy.linalg.solve_triangular on the same factors
  cheb_p40_ssor_eigs   the eigenvalue estimates handed to chebyshev: the
                  extreme eigenvalues of M A from its dense spectrum

For every case that converges by `tol` the script asserts that neither of the
last two history entries is within 1e-6 relative of the criterion: a step
count must not hinge on rounding.

Output: tests/golden/precond_factored.npz.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden import _import_reference, problems  # noqa: E402


def _by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pairwise_inner(x, y):
    """The default inner product summed pairwise (np.sum)."""
    return np.sum(x.conj() * y, axis=0)


def _cheb_eigs(A, P):
    """The extreme eigenvalues of M A (real: M and A are SPD), from the dense
    spectrum, M applied to the columns of A."""
    MA = P @ A.toarray()
    ev = np.sort(scipy.linalg.eigvals(MA).real)
    return np.array([ev[0], ev[-1]])


def main():
    krylov = _import_reference()
    PC = _by_path("_precond_factored_cases", "tests", "precond_factored_cases.py")
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    for name, solver, slot, spec, key, kw in PC.CASES:
        A, b = PC.problem(problems, key)
        P = PC.host_precond(A, spec, A.dtype)
        eigs = None
        if solver == "chebyshev":
            eigs = _cheb_eigs(A, PC.host_precond(A, spec, A.dtype, dense=True))
            out[f"{name}_eigs"] = eigs
        with quiet, np.errstate(all="ignore"):
            sol, info = PC.call(krylov, solver, A, b, slot, P, kw, eigs=eigs)
        res = np.asarray(info.resnorms, dtype=np.float64)
        out[f"{name}_resnorms"] = res
        out[f"{name}_numsteps"] = np.array(info.numsteps)
        out[f"{name}_success"] = np.array(bool(info.success))
        out[f"{name}_xk"] = np.asarray(info.xk)
        ops = info.num_operations
        out[f"{name}_ops"] = (np.full(6, np.nan) if ops is None else
                              np.array([ops[k] for k in ("A", "M", "Ml", "Mr", "inner", "axpy")], dtype=np.float64))
        # a step count must not hinge on rounding
        tol = kw.get("tol", 1e-5)
        if info.success and tol > 0 and info.numsteps > 0:
            crit = np.maximum(tol * res[0], 1e-15)
            for e in (res[-1], res[-2]):
                assert np.all(np.abs(e - crit) > 1e-6 * crit), (name, np.max(np.abs(e - crit) / crit))
        # the case's own spread
        variants = [(P, {"inner": _pairwise_inner}), (PC.host_precond(A, spec, A.dtype, dense=True), {})]
        r0 = float(np.max(res[0]))
        spread = 0.0
        for Pv, extra in variants:
            with quiet, np.errstate(all="ignore"):
                _, iv = PC.call(krylov, solver, A, b, slot, Pv, kw, eigs=eigs, **extra)
            rv = np.asarray(iv.resnorms, dtype=np.float64)
            assert iv.numsteps == info.numsteps and rv.shape == res.shape, (name, iv.numsteps, info.numsteps)
            spread = max(spread, float(np.max(np.abs(rv - res)) / r0))
        out[f"{name}_spread"] = np.array(spread)
        print(f"{name}: steps {info.numsteps} success {bool(info.success)} spread {spread:.2e}", flush=True)
    path = os.path.join(HERE, "precond_factored.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
