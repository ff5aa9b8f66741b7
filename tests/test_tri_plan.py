"""The host side of the sparse triangular solve and of the stationary solvers:
the analysis (kry_tri_plan: levels, row order, slices, launch grouping) against
a NumPy restatement, the same analysis built stand-alone under the host
sanitizers, the argument checks that need no device, and the reference
fixture's contents. No kernel is launched here."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import tri_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("name", TC.NAMES)
def test_tri_plan_matches_restatement(name, lower, itype):
    from krylov_amd import _lib

    T = TC.triangle(TC.pattern(name), lower)
    got = _lib.tri_plan(T.indptr.astype(itype), T.indices.astype(itype), lower)
    want = TC.plan_py(T, lower)
    for key in ("levels", "launches", "slices", "slots", "max_level"):
        assert got[key] == want[key], key
    for key in ("level", "order", "launch", "widths"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_tri_plan_regimes():
    """The shapes the plan has to serve: one row per level (all merged into
    one workgroup's launch), a level above the workgroup's capacity (a launch
    of its own), levels of exactly 64 and 65 rows (one and two slices)."""
    from krylov_amd import _lib

    def plan(name, lower):
        T = TC.triangle(TC.pattern(name), lower)
        return _lib.tri_plan(T.indptr, T.indices, lower)

    p = plan("chain300", True)
    assert (p["levels"], p["launches"], p["slices"], p["max_level"]) == (300, 1, 300, 1)
    p = plan("arrow3000", True)  # 2,999 independent rows, then the full row
    assert (p["levels"], p["launches"], p["max_level"]) == (2, 2, 2999)
    assert p["widths"][-1] == 2999 and p["slots"] == 64 * 2999
    p = plan("arrow3000", False)  # the last row first, then 2,999 rows of one entry
    assert (p["levels"], p["launches"], p["max_level"]) == (2, 2, 2999)
    assert p["slices"] == 1 + (2999 + 63) // 64
    assert plan("level64", True)["slices"] == 2 and plan("level65", True)["slices"] == 3
    p = plan("poisson40", True)
    assert (p["levels"], p["max_level"]) == (79, 40)
    assert plan("diagonal", True)["levels"] == 1 and plan("n1", False)["slots"] == 0


def test_tri_plan_rejects_bad_triangles():
    from krylov_amd import _lib

    A = TC.pattern("poisson40")
    with pytest.raises(ValueError):  # entries above the diagonal in a "lower" triangle
        _lib.tri_plan(A.indptr, A.indices, True)
    L = sp.tril(A, -1).tocsr()  # no diagonal at all
    with pytest.raises(np.linalg.LinAlgError):
        _lib.tri_plan(L.indptr, L.indices, True)
    T = TC.triangle(A, True)
    ix = T.indices.copy()
    a = T.indptr[41]
    ix[a], ix[a + 1] = ix[a + 1], ix[a]  # an unsorted row
    with pytest.raises(ValueError):
        _lib.tri_plan(T.indptr, ix, True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tri_plan_under_host_sanitizers(tmp_path):
    """tools/tri_plan_check.cpp with host_image.cpp under ASan + UBSan: a
    stand-alone program run directly over the same matrices; it checks the
    plan and the image itself, and its counts are the library's."""
    from krylov_amd import _lib

    exe = str(tmp_path / "tri_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread",
                           os.path.join(REPO, "tools", "tri_plan_check.cpp"),
                           os.path.join(REPO, "krylov_amd", "csrc", "host_image.cpp"), "-o", exe])
    files, want = [], []
    for name in TC.NAMES:
        for lower in (True, False):
            for itype in (np.int32, np.int64):
                T = TC.triangle(TC.pattern(name), lower)
                ip, ix = T.indptr.astype(itype), T.indices.astype(itype)
                path = str(tmp_path / f"{name}_{int(lower)}_{np.dtype(itype).itemsize}.bin")
                with open(path, "wb") as f:
                    f.write(np.array([T.shape[0], T.nnz, np.dtype(itype).itemsize, int(lower)], dtype=np.int64).tobytes())
                    f.write(ip.tobytes())
                    f.write(ix.tobytes())
                p = _lib.tri_plan(ip, ix, lower)
                files.append(path)
                want.append([p[k] for k in ("levels", "launches", "slices", "slots", "max_level")])
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(files)
    for line, path, w in zip(lines, files, want):
        parts = line.split()
        assert parts[0] == path and [int(v) for v in parts[1:]] == w


def test_argument_checks_need_no_device():
    import krylov_amd
    from krylov_amd import problems
    from krylov_amd.triangular import canonical_triangle

    A = problems.poisson2d(8)
    b = np.ones(A.shape[0])
    Z = A.tolil()
    Z[5, 5] = 0.0
    Z = Z.tocsr()
    for fn in (krylov_amd.gauss_seidel, krylov_amd.sor, krylov_amd.ssor):
        with pytest.raises(np.linalg.LinAlgError):
            fn(Z, b)
    with pytest.raises(np.linalg.LinAlgError):
        krylov_amd.TriangularOperator(sp.tril(Z))
    with pytest.raises(np.linalg.LinAlgError):  # a missing diagonal entry
        canonical_triangle(sp.tril(A, -1) + sp.diags(np.r_[np.ones(63), 0.0]), True)
    with pytest.raises(ValueError):
        canonical_triangle(A, True)  # not triangular
    # a CsrOperator keeps neither diagonal nor triangle (no instance is needed to refuse one)
    op = object.__new__(krylov_amd.CsrOperator)
    for fn in (krylov_amd.jacobi, krylov_amd.gauss_seidel, krylov_amd.sor, krylov_amd.ssor):
        with pytest.raises(TypeError, match="pass the"):
            fn(op, b)
    with pytest.raises(AssertionError):  # chebyshev.py:49
        krylov_amd.chebyshev(A, b, (2.0, 1.0))
    wide = np.ones((A.shape[0], 65))
    for fn in (krylov_amd.richardson, krylov_amd.jacobi, krylov_amd.gauss_seidel, krylov_amd.sor, krylov_amd.ssor):
        with pytest.raises(NotImplementedError):
            fn(A, wide)
    with pytest.raises(NotImplementedError):
        krylov_amd.chebyshev(A, wide, (0.1, 8.0))


def test_stationary_fixture_holds_every_case():
    from krylov_amd import problems
    from tests import gpu_helpers as H
    from tests import stationary_cases as SC

    d = np.load(os.path.join(HERE, "golden", "stationary.npz"))
    assert os.path.getsize(os.path.join(HERE, "golden", "stationary.npz")) < (1 << 20)
    names = [c[0] for c in SC.big_cases(problems)] + [c[0] for c in SC.small_cases(H)]
    assert len(names) == 19 + 5 * 8 + 6
    for name in names:
        for key in ("resnorms", "numsteps", "success", "spread"):
            assert f"{name}_{key}" in d.files, (name, key)
        assert (f"{name}_x" in d.files) != (f"{name}_xs" in d.files), name
        assert d[f"{name}_resnorms"].shape[0] == int(d[f"{name}_numsteps"]) + 1
        assert 0.0 <= float(d[f"{name}_spread"]) < (1e-6 if name.startswith("f32") else 1e-15)
    # the step counts the reference was observed to take
    steps = {"jacobi_rand": 64, "gs_rand_lower": 35, "gs_rand_upper": 36, "sor_p40_lower": 182, "ssor_p40": 128,
             "cheb_p40": 245, "richardson_p40": 60, "sor_p157": 30, "ssor_perm": 20}
    for name, k in steps.items():
        assert int(d[f"{name}_numsteps"]) == k, name
    assert d["sor_p157_xs"].shape == (SC.NSAMPLE,) and d["ssor_perm_xs"].shape == (SC.NSAMPLE,)
