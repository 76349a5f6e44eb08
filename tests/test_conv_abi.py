"""The conv part's C-ABI (include/aigar.h, aigar_net_config_cnn, aigar_net_set_conv_weights):
declared, laid out as the ctypes mirror has it, exported, additions only (ABI 7), and refused
loudly.  CPU only: aigar_net_config_cnn checks both parameter sets before its handle, so every
bad set is seen here with its own message and a NULL handle; the refusals that need a live
handle (a tiled handle, conv weights of the wrong shape, a pixel state that does not fit) are in
tests/test_gpu_conv.py and tests/test_gpu_env_conv.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_net_config_cnn", "aigar_net_set_conv_weights")
FIELDS = ("side", "channels", "n_conv", "k", "stride", "filters")
MACROS = ("AIGAR_CONV_MAX_LAYERS", "AIGAR_CONV_MAX_SIDE", "AIGAR_CONV_MAX_CHANNELS", "AIGAR_CONV_MAX_KERNEL",
          "AIGAR_CONV_MAX_FILTERS", "AIGAR_NET_MAX_IN", "AIGAR_ABI_VERSION")


def test_header_declares_the_conv_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_conv_params \{", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_conv_params_layout_and_constants_match_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu %%zu", ' \
          'sizeof(aigar_conv_params), sizeof(aigar_net_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_conv_params, %s));\n' % f
    src += 'printf("%s\\n", %s);return 0;}' % (" %d" * len(MACROS), ", ".join(MACROS))
    exe = str(tmp_path / "conv_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.ConvParams) == 48
    assert v[1] == C.sizeof(_abi.NetParams) == 56  # (aigar_net_params keeps its layout)
    for f, off in zip(FIELDS, v[2:2 + len(FIELDS)]):
        assert off == getattr(_abi.ConvParams, f).offset, f
    assert v[2 + len(FIELDS):] == [_abi.CONV_MAX_LAYERS, _abi.CONV_MAX_SIDE, _abi.CONV_MAX_CHANNELS,
                                   _abi.CONV_MAX_KERNEL, _abi.CONV_MAX_FILTERS, _abi.NET_MAX_IN, _abi.ABI_VERSION]
    assert v[2 + len(FIELDS):] == [3, 128, 8, 8, 64, 16384, 7]
    inc = open(os.path.join(ROOT, "aigar_amd", "csrc", "conv.inc")).read()
    for pat in (r"kConvMax = 3\b", r"kConvMaxSide = 128\b", r"kConvMaxCh = 8\b", r"kConvMaxK = 8\b", r"kConvMaxF = 64\b"):
        assert re.search(pat, inc), pat
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"conv.inc"' in build  # (stale() sees the kernel's file)


def _conv(side=42, channels=1, convs=((8, 4, 32), (4, 2, 64))):
    p = _abi.ConvParams(side, channels, len(convs))
    for i, (k, s, f) in enumerate(convs[:3]):
        p.k[i], p.stride[i], p.filters[i] = k, s, f
    return p


def _dense(n_in=576, units=(100, 100, 25), x_dtype=1, hidden=_abi.ACT_RELU, out=_abi.ACT_LINEAR):
    p = _abi.NetParams(len(units), n_in, x_dtype, hidden, out, 0)
    for i, v in enumerate(units[:8]):
        p.units[i] = v
    return p


def test_library_exports_the_conv_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    assert L.aigar_abi_version() == 7
    good_c, good_d = _conv(), _dense()
    assert L.aigar_net_config_cnn(None, C.byref(good_c), C.byref(good_d)) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_net_config_cnn(None, None, C.byref(good_d)) < 0 and b"null argument" in L.aigar_last_error()
    assert L.aigar_net_config_cnn(None, C.byref(good_c), None) < 0 and b"null argument" in L.aigar_last_error()
    assert L.aigar_net_set_conv_weights(None, 0, None, None, 0) < 0
    assert L.aigar_last_error()


@pytest.mark.parametrize("c, d, word", [
    (_conv(side=0), _dense(), b"side = 0"), (_conv(side=129), _dense(), b"side = 129"),
    (_conv(channels=0), _dense(), b"channels = 0"), (_conv(channels=9), _dense(), b"channels = 9"),
    (_conv(convs=()), _dense(), b"n_conv = 0"),
    (_abi.ConvParams(42, 1, 4), _dense(), b"n_conv = 4"),
    (_conv(convs=((0, 4, 32),)), _dense(), b"k = 0"), (_conv(convs=((9, 4, 32),)), _dense(), b"k = 9"),
    (_conv(convs=((8, 0, 32),)), _dense(), b"stride = 0"), (_conv(convs=((8, 9, 32),)), _dense(), b"stride = 9"),
    (_conv(convs=((8, 4, 0),)), _dense(), b"filters = 0"), (_conv(convs=((8, 4, 65),)), _dense(), b"filters = 65"),
    (_conv(convs=((8, 4, 32), (4, 2, 64), (4, 1, 64))), _dense(), b"no output"),  # 3 x 3 under a 4 x 4 kernel
    (_conv(side=7, convs=((8, 4, 32),)), _dense(), b"no output"),
    (_conv(side=84, convs=((4, 2, 64),)), _dense(n_in=107584), b"flattened length 107584"),  # only CNN_L2 at 84 x 84
    (_conv(), _dense(n_in=575), b"n_in = 575"),
    # the dense part's own refusals arrive through the same call
    (_conv(), _dense(units=(4,) * 6), b"n_layers = 6"), (_conv(), _dense(units=(257, 4)), b"257 units"),
    (_conv(), _dense(x_dtype=2), b"x_dtype"), (_conv(), _dense(hidden=_abi.ACT_ELU), b"elu"),
    (_conv(), _dense(out=_abi.ACT_TANH), b"tanh"),
])
def test_net_config_cnn_refuses_bad_parameters_with_a_message(c, d, word):
    L = _lib.load()
    assert L.aigar_net_config_cnn(None, C.byref(c), C.byref(d)) < 0
    msg = L.aigar_last_error()
    assert b"net_config" in msg and word in msg, msg


def test_good_parameters_reach_the_handle_check():
    L = _lib.load()
    for c, d in ((_conv(), _dense()), (_conv(42, 6), _dense()), (_conv(3, 4, ((1, 1, 64),)), _dense(576)),
                 (_conv(84), _dense(5184)), (_conv(128, 8, ((8, 8, 64), (8, 8, 64), (2, 1, 64))), _dense(64))):
        assert L.aigar_net_config_cnn(None, C.byref(c), C.byref(d)) < 0
        assert b"null handle" in L.aigar_last_error(), L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    from aigar_amd import net
    assert callable(net.cnn_spec) and callable(net.cnn_weights_from_torch)
    assert net.CnnSpec._fields == ("side", "channels", "convs", "n_flat", "units", "hidden", "out")
    assert callable(net.mlp_spec) and net.NetSpec._fields == ("n_in", "units", "hidden", "out")
