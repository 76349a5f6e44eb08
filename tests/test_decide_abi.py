"""The action selection's C-ABI (include/aigar.h, aigar_decide*): declared, laid out as
the ctypes mirror has it, exported, and refused loudly without a handle that has a
config.  CPU only (the refusal on a live handle without a config is in
tests/test_gpu_decide.py)."""
import ctypes as C
import os
import re
import subprocess

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_decide_config", "aigar_decide", "aigar_env_step_q")


def test_header_declares_the_decide_calls():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS + ("aigar_warnings",):
        assert need in names, need
    assert re.search(r"typedef struct aigar_decide_params \{", txt)
    assert re.search(r"#define AIGAR_WARN_Q_NONFINITE 0x8\b", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_decide_params_layout_and_constants_match_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%d %%d\\n", ' \
          'sizeof(aigar_decide_params), offsetof(aigar_decide_params, strategy), ' \
          'offsetof(aigar_decide_params, q_dtype), offsetof(aigar_decide_params, pad), ' \
          'offsetof(aigar_decide_params, seed), AIGAR_WARN_Q_NONFINITE, AIGAR_ABI_VERSION);return 0;}' % HEADER
    exe = str(tmp_path / "decide_hdr_check")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    size, o_strategy, o_dtype, o_pad, o_seed, warn, abi = map(int, subprocess.check_output([exe]).split())
    assert size == C.sizeof(_abi.DecideParams) == 24
    assert o_strategy == _abi.DecideParams.strategy.offset
    assert o_dtype == _abi.DecideParams.q_dtype.offset
    assert o_pad == _abi.DecideParams.pad.offset
    assert o_seed == _abi.DecideParams.seed.offset
    assert warn == _abi.WARN_Q_NONFINITE
    assert abi == _abi.ABI_VERSION == 7
    assert _abi.STRATEGIES == {"e-Greedy": 0, "Boltzmann": 1} and _abi.DECIDE_MAX_OUT == 1024
    # the device's copy of the warn bit and the stream word of the own draws
    dev = open(os.path.join(ROOT, "aigar_amd", "csrc", "aigar_dev.h")).read()
    assert re.search(r"WARN_Q_NONFINITE = 8\b", dev)
    sem = open(os.path.join(ROOT, "aigar_amd", "csrc", "aigar_sem.h")).read()
    assert re.search(r"ST_DECIDE = 10\b", sem)


def test_library_exports_the_decide_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS + ("aigar_warnings",) if n not in exported]
    assert L.aigar_abi_version() == 7
    for n in CALLS:
        assert getattr(L, n).argtypes is not None
    # nothing to decide with: error returns, with a message
    prm = _abi.RewardParams.from_parameters(None)
    assert L.aigar_decide(None, None, None, None, None, None, None) < 0
    assert L.aigar_last_error()
    assert L.aigar_env_step_q(None, None, None, None, 0, 0, C.byref(prm), None, None, 0, None, None) < 0
    assert L.aigar_decide_config(None, None, None) < 0


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("decide_config", "decide", "env_step_q", "warnings"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("step_q", "step_q_calls", "set_exploration"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["discrete"].default is None  # off unless asked for
