"""aigar_selftest_sem's C-ABI (include/aigar.h): declared, exported, its op codes and column
counts the same in the header, the ctypes mirror and the Python wrapper, and every bad argument
refused with a message that names it.  CPU only: the refusals and n == 0 return before any
device call (what the ops compute is in tests/test_gpu_sem.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
OPS = ("MOD_POS", "TRUNC_DIV_POS", "PY_MOD", "ROUND3", "SUM", "RADIUS", "BUCKET", "FOOTPRINT", "MOVE", "MOMENTUM",
       "MERGE_TIME", "PHILOX", "TRIG_FORMS")


def test_header_declares_the_call_and_the_ops_match_the_mirror():
    txt = open(HEADER).read()
    assert re.search(r"^int aigar_selftest_sem\(int op, const double \*in, int in_cols, double \*out, int out_cols, "
                     r"int n\);", txt, re.M)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # an addition only
    codes = {k: int(v) for k, v in re.findall(r"#define AIGAR_SEM_(\w+) (\d+)", txt)}
    assert codes.pop("N_OPS") == len(OPS) == len(_abi.SEM_COLS)
    assert codes == {name: getattr(_abi, "SEM_" + name) for name in OPS}
    assert sorted(codes.values()) == list(range(len(OPS)))
    # the column counts of the kernel's table, in the ops' order
    api = open(os.path.join(ROOT, "aigar_amd", "csrc", "api.hip")).read()
    table = api[api.index("kSemOps[AIGAR_SEM_N_OPS]"):]
    rows = re.findall(r"\{(\d+), (\d+)\},\s*// (\w+)", table[:table.index("};")])
    assert [r[2] for r in rows] == list(OPS)
    assert [(int(a), int(b)) for a, b, _ in rows] == [_abi.SEM_COLS[getattr(_abi, "SEM_" + n)] for n in OPS]


def _call(L, op, in_cols, out_cols, n, null_in=False, null_out=False):
    src = np.zeros(max(1, in_cols * max(n, 0)))
    dst = np.zeros(max(1, out_cols * max(n, 0)))
    dp = C.POINTER(C.c_double)
    rc = L.aigar_selftest_sem(op, None if null_in else src.ctypes.data_as(dp), in_cols,
                              None if null_out else dst.ctypes.data_as(dp), out_cols, n)
    return rc, L.aigar_last_error().decode()


def test_library_exports_the_call_and_refuses_bad_arguments_by_name():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    assert re.search(r" T aigar_selftest_sem\b", syms)
    assert L.aigar_abi_version() == 7
    for op, (n_in, n_out) in _abi.SEM_COLS.items():
        assert _call(L, op, n_in, n_out, 0)[0] == 0  # n == 0 succeeds
        rc, msg = _call(L, op, n_in + 1, n_out, 0)
        assert rc < 0 and "in_cols" in msg, msg
        rc, msg = _call(L, op, n_in, n_out + 1, 0)
        assert rc < 0 and "out_cols" in msg, msg
        rc, msg = _call(L, op, n_in, n_out, 4, null_in=True)
        assert rc < 0 and "in is null" in msg, msg
        rc, msg = _call(L, op, n_in, n_out, 4, null_out=True)
        assert rc < 0 and "out is null" in msg, msg
        rc, msg = _call(L, op, n_in, n_out, -1)
        assert rc < 0 and re.search(r"\bn -1\b", msg), msg
    for op in (-1, len(OPS), 1000):
        rc, msg = _call(L, op, 2, 1, 0)
        assert rc < 0 and "op %d" % op in msg, msg


def test_python_wrapper_checks_its_columns_and_returns_empty_columns_for_no_elements():
    for op, (n_in, n_out) in _abi.SEM_COLS.items():
        out = _lib.selftest_sem(op, *[np.zeros(0)] * n_in)
        assert isinstance(out, tuple) and len(out) == n_out and all(o.shape == (0,) and o.dtype == np.float64 for o in out)
    with pytest.raises(ValueError, match="takes 2 columns"):
        _lib.selftest_sem(_abi.SEM_PY_MOD, np.zeros(3))
    with pytest.raises(ValueError, match="unequal length"):
        _lib.selftest_sem(_abi.SEM_PY_MOD, np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError, match="SEM_"):
        _lib.selftest_sem(99, np.zeros(3))
