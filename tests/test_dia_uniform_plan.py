"""Uniform slot columns of the SELL-128/DIA image, host side (dia_build
through kry_dia_uniform_plan): the flag and the value of every slot column
against a NumPy restatement built from kry_dia_plan's offsets and masks, and
the same builder stand-alone under the host sanitizers. No kernel is launched
here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dia_uniform_cases as UC

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _plans(A):
    from krylov_amd import _lib

    ip, ix = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    plan = _lib.dia_plan(ip, ix)
    got = _lib.dia_uniform_plan(ip, ix, A.data)
    assert plan is not None and got is not None
    assert got["cols"] == plan["slots"] // 128
    return plan, got


@pytest.mark.parametrize("name", ["stencil15_7", "poisson2d_61", "tridiag_special", "shifted_lap3d_f32"])
def test_uniform_plan_matches_restatement(name):
    A = UC.plan_matrices()[name]
    plan, got = _plans(A)
    flags, values = UC.uniform_py(A, plan)
    np.testing.assert_array_equal(got["flags"], flags)
    assert got["values"].dtype == A.dtype
    np.testing.assert_array_equal(UC._bits(got["values"]), UC._bits(values))
    assert got["uniform"] == int(flags.sum())
    if name in ("stencil15_7", "poisson2d_61"):
        # constant coefficients: every slot column, boundary slices with holes included
        assert got["uniform"] == got["cols"]
        assert set(np.unique(got["values"]).tolist()) == ({14.0, -1.0} if name == "stencil15_7" else {4.0, -1.0})
        assert np.any(plan["masks"] != np.uint64(0xFFFFFFFFFFFFFFFF))  # there are holes
    if name == "tridiag_special":
        assert got["flags"].tolist() == UC.TRIDIAG_FLAGS
        assert np.isnan(got["values"][4]) and UC._bits(got["values"])[4] == UC._bits(np.array([UC.nan_with_payload(0x33)]))[0]
        assert got["values"][5] == 2.5 and got["values"][3] == -1.0
        assert not np.any(UC._bits(got["values"][:3]))  # not flagged: value bits 0
    if name == "shifted_lap3d_f32":
        assert A.dtype == np.float32
        assert 2 * got["uniform"] < got["cols"]  # row-scaled: mostly streamed


def test_uniform_plan_refused_with_the_image():
    """No diagonal-offset image (an unsorted row): no uniform plan either."""
    from krylov_amd import _lib, problems

    A = problems.poisson2d(20).tocsr()
    a = A.indptr[37]
    A.indices[a], A.indices[a + 1] = A.indices[a + 1], A.indices[a]
    assert _lib.dia_uniform_plan(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data) is None


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_uniform_plan_under_host_sanitizers(tmp_path):
    """tools/dia_uniform_check.cpp with host_image.cpp under ASan + UBSan: a
    stand-alone program run directly over the same matrices; it checks the
    flags against the image it built and prints the counts the library gives."""
    from krylov_amd import _lib

    exe = str(tmp_path / "dia_uniform_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-pthread",
                           os.path.join(REPO, "tools", "dia_uniform_check.cpp"),
                           os.path.join(REPO, "krylov_amd", "csrc", "host_image.cpp"), "-o", exe])
    files, want = [], []
    for name, A in UC.plan_matrices().items():
        ip, ix = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            f.write(np.array([A.shape[0], A.nnz, A.dtype.itemsize], dtype=np.int64).tobytes())
            f.write(ip.tobytes())
            f.write(ix.tobytes())
            f.write(np.ascontiguousarray(A.data).tobytes())
        p = _lib.dia_uniform_plan(ip, ix, A.data)
        files.append(path)
        want.append([p["cols"], p["uniform"]])
    out = subprocess.run([exe] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(files)
    for line, path, w in zip(lines, files, want):
        parts = line.split()
        assert parts[0] == path and [int(v) for v in parts[1:]] == w
