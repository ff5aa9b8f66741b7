"""Golden runs of the reference's solvers preconditioned by block-Jacobi, made
by running the REFERENCE itself, imported read-only as in make_golden.py. Run
only in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_precond_blockjacobi.py

The preconditioner is a plain Python object whose ``@`` is the two sequential
loops of tests/blockjacobi_cases.py (HostBlockJacobi: Gauss-Jordan inverses of
the diagonal blocks, the j-ascending block product). The cases are listed
there (CASES); every b is default_rng(3).standard_normal, and the tests
regenerate the inputs from the same generators: only outputs are stored. Per
case:
  <name>_resnorms / _numsteps / _success / _xk   the reference's Info (no _xk
                  for the 128-column case)
  <name>_spread   max_k |resnorm_k - variant_k| / resnorm_0 over the same
                  reference call made with a pairwise inner product
  <name>_none_numsteps / _none_last, <name>_jacobi_numsteps / _jacobi_last
                  step count and last history entry of the same call without
                  a preconditioner and with diag(A)^-1 in the same slot: what
                  a device that applied the identity or only the diagonal
                  would reproduce (tests/test_blockjacobi_cases.py)

The script asserts that the step count does not move under the pairwise inner
product, and for a case that converges by its tolerance that neither of the
last two history entries is within 1e-6 relative of the criterion: a step
count must not hinge on rounding.

Output: tests/golden/precond_blockjacobi.npz.
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

from tests import blockjacobi_cases as BC  # noqa: E402


def _pairwise_inner(x, y):
    """The default inner product summed pairwise (np.sum). numpy sums pairwise
    along a contiguous axis only (down the rows of an (n, k) block it adds row
    by row, which is the default inner product's own order), so a block's
    products are transposed first."""
    p = x.conj() * y
    return np.sum(p, axis=0) if p.ndim == 1 else np.sum(np.ascontiguousarray(p.T), axis=-1)


def main():
    krylov = _import_reference()
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    for name, solver, slot, key, bs, cols, kw in BC.CASES:
        A, b = BC.problem(problems, key, cols)
        P = BC.HostBlockJacobi(A, BC.uniform_starts(A.shape[0], bs), A.dtype)
        run = getattr(krylov, solver)
        with quiet, np.errstate(all="ignore"):
            _, info = run(A, b, **{slot: P}, **kw)
        res = np.asarray(info.resnorms, dtype=np.float64)
        out[f"{name}_resnorms"] = res
        out[f"{name}_numsteps"] = np.array(info.numsteps)
        out[f"{name}_success"] = np.array(bool(info.success))
        if cols <= 8:
            out[f"{name}_xk"] = np.asarray(info.xk)
        if info.success and info.numsteps > 0 and kw.get("tol", 1.0) > 0:
            tol = kw.get("tol", 1e-5)
            crit = np.maximum(tol * res[0], 1e-15)
            for e in (res[-1], res[-2]):
                assert np.all(np.abs(e - crit) > 1e-6 * crit), (name, np.max(np.abs(e - crit) / crit))
        with quiet, np.errstate(all="ignore"):
            _, iv = run(A, b, **{slot: P}, inner=_pairwise_inner, **kw)
        rv = np.asarray(iv.resnorms, dtype=np.float64)
        assert iv.numsteps == info.numsteps and rv.shape == res.shape, (name, iv.numsteps, info.numsteps)
        spread = float(np.max(np.abs(rv - res)) / float(np.max(res[0])))
        out[f"{name}_spread"] = np.array(spread)
        line = f"{name}: steps {info.numsteps} success {bool(info.success)} spread {spread:.2e}"
        for other, M in (("none", None), ("jacobi", BC.point_jacobi(A))):
            with quiet, np.errstate(all="ignore"):
                _, io_ = run(A, b, **({} if M is None else {slot: M}), **kw)
            out[f"{name}_{other}_numsteps"] = np.array(io_.numsteps)
            out[f"{name}_{other}_last"] = np.asarray(io_.resnorms, dtype=np.float64)[-1]
            line += f" {other} {io_.numsteps}"
        print(line, flush=True)
    path = os.path.join(HERE, "precond_blockjacobi.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
