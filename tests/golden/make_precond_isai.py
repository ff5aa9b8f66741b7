"""Golden runs of the reference's solvers preconditioned by SSOR and ILU(0)
objects that solve their factors with the incomplete sparse approximate
inverse (ISAI), made by running the REFERENCE itself, imported read-only as in
make_golden.py. Run only in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_precond_isai.py

The preconditioner is a plain Python object whose ``@`` is scipy products with
W_L, W_U (and the factors, for relaxation sweeps) from the sequential loop of
tests/isai_cases.py (HostIsai). The cases are listed there (CASES); every b is
default_rng(3).standard_normal(n), and the tests regenerate the inputs from
the same generators: only outputs are stored. Per case:
  <name>_resnorms / _numsteps / _success / _xk   the reference's Info
  <name>_spread   max_k |resnorm_k - variant_k| / resnorm_0 over the same
                  reference call made with a pairwise inner product

The script asserts that the step count does not move under the pairwise inner
product, and for a case that converges by `tol` that neither of the last two
history entries is within 1e-6 relative of the criterion: a step count must not
hinge on rounding. A case that fails either gets another seed or tolerance
here and in CASES; none needed one.

Output: tests/golden/precond_isai.npz.
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

from tests import isai_cases as IC  # noqa: E402


def _pairwise_inner(x, y):
    """The default inner product summed pairwise (np.sum)."""
    return np.sum(x.conj() * y, axis=0)


def main():
    krylov = _import_reference()
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    for name, solver, slot, spec, sweeps, key, kw in IC.CASES:
        A, b = IC.problem(problems, key)
        P = IC.HostIsai(A, spec, A.dtype, sweeps)
        run = getattr(krylov, solver)
        with quiet, np.errstate(all="ignore"):
            _, info = run(A, b, **{slot: P}, **kw)
        res = np.asarray(info.resnorms, dtype=np.float64)
        out[f"{name}_resnorms"] = res
        out[f"{name}_numsteps"] = np.array(info.numsteps)
        out[f"{name}_success"] = np.array(bool(info.success))
        out[f"{name}_xk"] = np.asarray(info.xk)
        tol = kw["tol"]
        if info.success and info.numsteps > 0:
            crit = np.maximum(tol * res[0], 1e-15)
            for e in (res[-1], res[-2]):
                assert np.all(np.abs(e - crit) > 1e-6 * crit), (name, np.max(np.abs(e - crit) / crit))
        with quiet, np.errstate(all="ignore"):
            _, iv = run(A, b, **{slot: P}, inner=_pairwise_inner, **kw)
        rv = np.asarray(iv.resnorms, dtype=np.float64)
        assert iv.numsteps == info.numsteps and rv.shape == res.shape, (name, iv.numsteps, info.numsteps)
        spread = float(np.max(np.abs(rv - res)) / float(np.max(res[0])))
        out[f"{name}_spread"] = np.array(spread)
        print(f"{name}: steps {info.numsteps} success {bool(info.success)} spread {spread:.2e}", flush=True)
    path = os.path.join(HERE, "precond_isai.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
