"""The acting network's C-ABI (include/aigar.h, aigar_net*, aigar_env_step_net): declared,
laid out as the ctypes mirror has it, exported, additions only (ABI 7), and refused loudly.
CPU only: aigar_net_config checks its parameters before its handle, so every bad parameter
set is seen here with its own message; the refusals that need a live handle (a tiled handle,
a head without its decide / noise config or with the wrong dtype, n_out != n_act) are in
tests/test_gpu_net.py and tests/test_gpu_env_net.py, as the noise's and the selection's are."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_net_config", "aigar_net_set_weights", "aigar_net_forward", "aigar_net_output", "aigar_env_step_net")
FIELDS = ("n_layers", "n_in", "x_dtype", "hidden_act", "out_act", "pad", "units")
MACROS = ("AIGAR_NET_MAX_LAYERS", "AIGAR_NET_MAX_UNITS", "AIGAR_NET_MAX_IN", "AIGAR_ACT_LINEAR", "AIGAR_ACT_RELU",
          "AIGAR_ACT_SIGMOID", "AIGAR_ACT_ELU", "AIGAR_ACT_TANH", "AIGAR_NET_HEAD_Q", "AIGAR_NET_HEAD_ACTOR",
          "AIGAR_ABI_VERSION")


def test_header_declares_the_network_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_net_params \{", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_net_params_layout_and_constants_match_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_net_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_net_params, %s));\n' % f
    src += 'printf("%s\\n", %s);return 0;}' % (" %d" * len(MACROS), ", ".join(MACROS))
    exe = str(tmp_path / "net_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.NetParams) == 56
    for f, off in zip(FIELDS, v[1:1 + len(FIELDS)]):
        assert off == getattr(_abi.NetParams, f).offset, f
    assert v[1 + len(FIELDS):] == [_abi.NET_MAX_LAYERS, _abi.NET_MAX_UNITS, _abi.NET_MAX_IN, _abi.ACT_LINEAR,
                                   _abi.ACT_RELU, _abi.ACT_SIGMOID, _abi.ACT_ELU, _abi.ACT_TANH, _abi.NET_HEAD_Q,
                                   _abi.NET_HEAD_ACTOR, _abi.ABI_VERSION]
    assert (_abi.NET_MAX_LAYERS, _abi.NET_MAX_UNITS, _abi.NET_MAX_IN, _abi.ABI_VERSION) == (5, 256, 16384, 7)
    inc = open(os.path.join(ROOT, "aigar_amd", "csrc", "net.inc")).read()
    assert re.search(r"kNetMaxLayers = 5\b", inc) and re.search(r"kNetMaxUnits = 256\b", inc)
    assert re.search(r"kNetMaxIn = 16384\b", inc)
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"net.inc"' in build  # (stale() sees the kernel's file)


def test_library_exports_the_network_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    assert L.aigar_abi_version() == 7
    prm = _abi.RewardParams.from_parameters(None)
    good = _abi.NetParams(3, 365, 0, _abi.ACT_RELU, _abi.ACT_LINEAR, 0)
    good.units[0], good.units[1], good.units[2] = 100, 100, 25
    assert L.aigar_net_config(None, None) < 0
    assert L.aigar_net_config(None, C.byref(good)) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_net_set_weights(None, 0, None, None, 0) < 0
    assert L.aigar_net_forward(None, None, 0, 1, None) < 0
    assert L.aigar_net_output(None, None) < 0
    assert L.aigar_env_step_net(None, 0, None, None, 0, 0, 0, C.byref(prm), None, None, 0, None, None, None, 1) < 0
    assert L.aigar_last_error()


def _params(units, n_in=12, x_dtype=0, hidden=_abi.ACT_RELU, out=_abi.ACT_LINEAR):
    p = _abi.NetParams(len(units), n_in, x_dtype, hidden, out, 0)
    for i, v in enumerate(units[:8]):
        p.units[i] = v
    return p


@pytest.mark.parametrize("p, word", [
    (_params([4] * 6), b"n_layers = 6"), (_params([]), b"n_layers = 0"),
    (_params([4, 257, 4]), b"257 units"), (_params([4, 0]), b"0 units"),
    (_params([4], n_in=0), b"n_in = 0"), (_params([4], n_in=16385), b"n_in = 16385"),
    (_params([4], x_dtype=2), b"x_dtype"),
    (_params([4, 4], hidden=_abi.ACT_ELU), b"elu"), (_params([4, 4], hidden=_abi.ACT_TANH), b"tanh"),
    (_params([4, 4], hidden=_abi.ACT_SIGMOID), b"sigmoid"), (_params([4, 4], out=_abi.ACT_RELU), b"relu"),
    (_params([4, 4], out=_abi.ACT_ELU), b"elu"), (_params([4, 4], out=9), b"unknown"),
])
def test_net_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_net_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"net_config" in msg and word in msg, msg


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd import net
    from aigar_amd.env import AgarVecEnv
    for m in ("net_config", "net_set_weights", "net_forward", "net_output", "env_step_net"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("set_weights", "step_net", "collect"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["network"].default is None  # off unless asked for
    assert callable(net.mlp_spec) and callable(net.weights_from_torch)
