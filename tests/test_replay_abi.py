"""The replay memory's C-ABI (include/aigar.h, aigar_exp_*): declared, laid out as the
ctypes mirror has it, exported, and refused loudly without a memory.  CPU only."""
import ctypes as C
import os
import re
import subprocess

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_exp_config", "aigar_exp_info", "aigar_exp_add", "aigar_exp_sample", "aigar_exp_gather",
         "aigar_exp_update_priorities")


def test_header_declares_the_replay_calls():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_exp_params \{", txt)
    assert re.search(r"#define AIGAR_EXP_PRIORITIZED 0x1\b", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_exp_params_layout_matches_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%zu %%d\\n", ' \
          'sizeof(aigar_exp_params), offsetof(aigar_exp_params, flags), offsetof(aigar_exp_params, alpha), ' \
          'offsetof(aigar_exp_params, seed), AIGAR_EXP_PRIORITIZED);return 0;}' % HEADER
    exe = str(tmp_path / "exp_hdr_check")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    size, o_flags, o_alpha, o_seed, flag = map(int, subprocess.check_output([exe]).split())
    assert size == C.sizeof(_abi.ExpParams)
    assert o_flags == _abi.ExpParams.flags.offset
    assert o_alpha == _abi.ExpParams.alpha.offset
    assert o_seed == _abi.ExpParams.seed.offset
    assert flag == _abi.EXP_PRIORITIZED
    assert _abi.ABI_VERSION == 7


def test_library_exports_the_replay_calls():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    assert L.aigar_abi_version() == 7
    for n in CALLS:
        assert getattr(L, n).argtypes is not None


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("exp_config", "exp_info", "exp_add", "exp_sample", "exp_gather", "exp_update_priorities"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("sample", "update_priorities", "memory_size"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["memory"].default is None  # off unless asked for
