"""The REFERENCE's own float32 runs on a subset of the float32 cases.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_f32.py

Imports the reference read-only, as make_golden.py does, and runs krylov.cg,
krylov.gmres and krylov.minres in float32 with the default inner product on
the cases named in tests/f32_cases.py (PINNED): one size per n mod 4 residue,
k = 1, 2 and 3, and ortho = mgs, mgs2 and householder for GMRES. The inputs
are rebuilt from seeds by tests/f32_cases.py; only outputs are stored.

Output: tests/golden/f32.npz with, per case, the history as the reference
returned it (``_resnorms``, in its own dtype), ``_xk``, ``_numsteps``,
``_success`` and the dtype names (``_resnorms_dtype``, ``_xk_dtype``).
tests/test_oracle.py holds oracle/krylov_ref.py to it bitwise.
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)


def main():
    from make_golden import _import_reference

    from tests import f32_cases as F

    krylov = _import_reference()
    out = {}
    for cid in F.PINNED:
        solver, A, b, kw = F.build(F.case(cid))
        with contextlib.redirect_stdout(io.StringIO()):  # gmres.py prints
            _, info = getattr(krylov, solver)(A, b, **kw)
        h, x = np.asarray(info.resnorms), np.asarray(info.xk)
        out[f"{cid}_resnorms"] = h
        out[f"{cid}_xk"] = x
        out[f"{cid}_numsteps"] = np.array(info.numsteps)
        out[f"{cid}_success"] = np.array(info.success)
        out[f"{cid}_resnorms_dtype"] = np.array(h.dtype.name)
        out[f"{cid}_xk_dtype"] = np.array(x.dtype.name)
        print(f"{cid}: {info.numsteps} steps, resnorms {h.dtype} {h.shape}, xk {x.dtype} {x.shape}")
    path = os.path.join(HERE, "f32.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
