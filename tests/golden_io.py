"""Reference fixtures that are stored in parts, so that no committed file
exceeds 1 MiB: ``load(name)`` gives all arrays of a fixture as one mapping,
``save(name, arrays)`` writes the parts (tests/golden/make_golden.py)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture -> ((file stem, rule for the keys it holds), ...); the first part takes the rest
PARTS = {
    # the block right-hand-side cases (Poisson 64^2 x 8, rand5k x 3) apart from the single-column ones
    "solvers": (("solvers", None),
                ("solvers_block", lambda k: "blk" in k or k.startswith(("poisson64_", "rand5k_B")))),
    # the int64-index matrices apart from the int32 ones
    "spmv": (("spmv", None), ("spmv_i64", lambda k: "_i64_" in k)),
}


def _stem(name, key):
    for stem, rule in PARTS[name][1:]:
        if rule(key):
            return stem
    return PARTS[name][0][0]


def load(name):
    out = {}
    for stem, _ in PARTS.get(name, ((name, None),)):
        with np.load(os.path.join(GOLD, f"{stem}.npz")) as d:
            assert not set(d.files) & set(out), (name, stem)
            out.update({k: d[k] for k in d.files})
    return out


def save(name, arrays):
    for stem, _ in PARTS[name]:
        part = {k: v for k, v in arrays.items() if _stem(name, k) == stem}
        np.savez_compressed(os.path.join(GOLD, f"{stem}.npz"), **part)
