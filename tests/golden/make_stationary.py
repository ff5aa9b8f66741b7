"""Golden runs of the reference's stationary solvers and Chebyshev iteration
(richardson, jacobi, gauss_seidel, sor, ssor: stationary.py; chebyshev:
chebyshev.py), made by running the REFERENCE itself, imported read-only as in
make_golden.py. Run only in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stationary.py

The cases are listed in tests/stationary_cases.py (the tests regenerate the
inputs from the same seeds; only outputs are stored). Per case:
  <name>_resnorms / _numsteps / _success   the reference's Info
  <name>_x                                 info.xk (n <= 1600), else
  <name>_xs                                info.xk at stationary_cases.sample_index(n)
  <name>_spread   the case's own spread: max_k |resnorm_k - variant_k| /
                  resnorm_0 over the same reference call made through its
                  dense branch (A.toarray(), n <= 5000) and with a pairwise
                  inner product

For every case that converges by `tol` the script asserts that neither of the
last two history entries is within 1e-6 relative of the criterion: a step
count must not hinge on rounding.

Output: tests/golden/stationary.npz.
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden import _import_reference, problems  # noqa: E402


def _by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pairwise_inner(w=None):
    """The default (or weighted) inner product summed pairwise (np.sum)."""

    def inner(x, y):
        wy = y if w is None else (w.reshape((-1,) + (1,) * (y.ndim - 1)) * y)
        return np.sum(x.conj() * wy, axis=0)

    return inner


def _weighted_inner(w):
    """tests/test_solvers.py:157-161 of the reference, for (n,) and (n, k)."""

    def inner(x, y):
        if y.ndim == 1:
            return np.dot(x.T, w * y)
        return np.einsum("i...,i...->...", x.conj(), w.reshape((-1,) + (1,) * (y.ndim - 1)) * y)

    return inner


def main():
    krylov = _import_reference()
    H = _by_path("_gpu_helpers", "tests", "gpu_helpers.py")
    SC = _by_path("_stationary_cases", "tests", "stationary_cases.py")
    quiet = contextlib.redirect_stdout(io.StringIO())
    out = {}
    for name, solver, make in SC.all_cases(problems, H):
        A, b, kw = make()
        with quiet, np.errstate(all="ignore"):
            _, info = SC.call(krylov, solver, A, b, kw, _weighted_inner, callback=lambda x, r: None)
        res = np.asarray(info.resnorms)
        out[f"{name}_resnorms"] = res.astype(np.float64)
        out[f"{name}_numsteps"] = np.array(info.numsteps)
        out[f"{name}_success"] = np.array(bool(info.success))
        xk = np.asarray(info.xk)
        n = xk.shape[0]
        if n <= SC.FULL_X:
            out[f"{name}_x"] = xk
        else:
            out[f"{name}_xs"] = xk[SC.sample_index(n)]
        # a step count must not hinge on rounding
        tol = kw.get("tol", 1e-5)
        if info.success and tol > 0 and info.numsteps > 0:
            crit = np.maximum(tol * res[0], 1e-15)
            for e in (res[-1], res[-2]):
                worst = np.max(np.abs(np.asarray(e, dtype=np.float64) - crit) / crit)
                assert np.all(np.abs(np.asarray(e, dtype=np.float64) - crit) > 1e-6 * crit), (name, worst)
        # the case's own spread
        variants = []
        w = kw.get("inner_weights")
        kwp = {k: v for k, v in kw.items() if k != "inner_weights"}
        kwp["inner"] = _pairwise_inner(w)
        variants.append((A, kwp))
        if scipy.sparse.issparse(A) and A.shape[0] <= 5000:
            variants.append((A.toarray(), kw))
        r0 = float(np.max(res[0])) if res.size else 0.0
        spread = 0.0
        for Av, kwv in variants:
            with quiet, np.errstate(all="ignore"):
                _, iv = SC.call(krylov, solver, Av, b, kwv, _weighted_inner, callback=lambda x, r: None)
            rv = np.asarray(iv.resnorms, dtype=np.float64)
            assert iv.numsteps == info.numsteps and rv.shape == res.shape, (name, iv.numsteps, info.numsteps)
            if r0 > 0:
                spread = max(spread, float(np.max(np.abs(rv - res.astype(np.float64))) / r0))
        out[f"{name}_spread"] = np.array(spread)
        print(f"{name}: steps {info.numsteps} success {bool(info.success)} spread {spread:.2e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "stationary.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "stationary.npz")))


if __name__ == "__main__":
    main()
