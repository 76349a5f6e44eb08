"""The CNN trainer's C-ABI (include/aigar.h, aigar_train_config_cnn, aigar_net_get_conv_weights):
declared, exported, mirrored, additions only (ABI 7), and refused loudly.  CPU only:
aigar_train_config_cnn checks its parameters before its handle, so every bad parameter set is
seen here with its own message under its own name; the refusals that need a live handle are in
tests/test_gpu_cnn_train.py.  Also aigar_amd.net.cnn_weights_to_torch, the inverse of
cnn_weights_from_torch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import conv_model as CM
import net_model as M
from aigar_amd import _abi, _lib, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_train_config_cnn", "aigar_net_get_conv_weights")
FIELDS = ("batch", "min_size", "target_steps", "pad", "lr", "beta1", "beta2", "epsilon", "discount")


def test_header_declares_the_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"int aigar_train_config_cnn\(aigar_handle \*h, const aigar_train_params \*p\);", txt)
    assert re.search(r"int aigar_net_get_conv_weights\(aigar_handle \*h, int which, int layer, float \*W, float \*b, "
                     r"int on_device\);", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"convtrain.inc"' in build  # (stale() sees the kernels' file)
    api = open(os.path.join(ROOT, "aigar_amd", "csrc", "api.hip")).read()
    assert api.index('#include "train.inc"') < api.index('#include "convtrain.inc"') < api.index('#include "actrain.inc"')


def test_library_exports_the_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    good = _abi.TrainParams(32, 32, 1500, 0, 1e-3, 0.9, 0.999, 1e-7, 0.9)
    assert L.aigar_train_config_cnn(None, None) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_train_config_cnn(None, C.byref(good)) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_net_get_conv_weights(None, 0, 0, None, None, 0) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_train_config_cnn.argtypes[1] == C.POINTER(_abi.TrainParams)  # the same parameter struct
    assert len(L.aigar_net_get_conv_weights.argtypes) == 6


def _p(**kw):
    d = dict(batch=32, min_size=0, target_steps=0, pad=0, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9)
    d.update(kw)
    return _abi.TrainParams(*[d[f] for f in FIELDS])


BAD = [
    (_p(batch=0), b"batch = 0"), (_p(batch=257), b"batch = 257"), (_p(batch=-3), b"batch = -3"),
    (_p(min_size=-1), b"min_size = -1"), (_p(target_steps=-1), b"target_steps = -1"),
    (_p(lr=0.0), b"lr = 0"), (_p(lr=-1e-3), b"lr = -0.001"), (_p(lr=float("nan")), b"lr = nan"),
    (_p(lr=float("inf")), b"lr = inf"),
    (_p(beta1=1.0), b"beta1 = 1"), (_p(beta1=-0.1), b"beta1 = -0.1"), (_p(beta2=1.0), b"beta2 = 1"),
    (_p(beta2=float("nan")), b"beta2 = nan"),
    (_p(epsilon=0.0), b"epsilon = 0"), (_p(epsilon=-1e-7), b"epsilon = -1e-07"),
    (_p(discount=1.5), b"discount = 1.5"), (_p(discount=-0.1), b"discount = -0.1"),
]


@pytest.mark.parametrize("p, word", BAD)
def test_train_config_cnn_refuses_bad_parameters_with_the_dense_trainers_message_under_its_own_name(p, word):
    L = _lib.load()
    assert L.aigar_train_config_cnn(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert msg.startswith(b"train_config_cnn: ") and word in msg, msg
    assert L.aigar_train_config(None, C.byref(p)) < 0
    assert L.aigar_last_error() == msg.replace(b"train_config_cnn: ", b"train_config: ", 1)  # the same message


def test_edge_values_pass_the_parameter_checks():
    L = _lib.load()
    for p in (_p(batch=1), _p(batch=256), _p(beta1=0.0, beta2=0.0), _p(discount=0.0), _p(discount=1.0)):
        assert L.aigar_train_config_cnn(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    from aigar_amd.env import AgarVecEnv
    for m in ("train_config_cnn", "net_get_weights", "train_step", "train_sync_target", "train_reset"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("train", "train_info", "train_td", "get_weights", "sync_target"):
        assert callable(getattr(AgarVecEnv, m))
    assert callable(net.cnn_weights_to_torch)


SPECS = [net.CnnSpec(12, 1, ((4, 2, 5), (2, 2, 17)), 68, (6, 25), "relu", "linear"),
         net.CnnSpec(10, 2, ((3, 1, 4), (4, 2, 6), (3, 1, 8)), 8, (7, 3), "relu", "linear"),
         net.CnnSpec(8, 3, ((3, 1, 4),), 144, (5,), "relu", "linear")]


@pytest.mark.parametrize("spec", SPECS, ids=["two", "three", "one"])
def test_cnn_weights_to_torch_is_the_inverse_of_cnn_weights_from_torch(spec):
    import torch
    rng = np.random.default_rng(spec.side)
    pairs = CM.pairs(CM.make_convs(rng, spec.channels, spec.convs), M.make_weights(rng, spec.n_flat, spec.units))
    sd = net.cnn_weights_to_torch(pairs, spec)
    nc = len(spec.convs)
    assert list(sd)[:2] == ["conv0.weight", "conv0.bias"] and list(sd)[2 * nc] == "fc0.weight"
    k, _, f = spec.convs[0]
    assert tuple(sd["conv0.weight"].shape) == (f, spec.channels, k, k) and sd["conv0.weight"].dtype == torch.float32
    assert tuple(sd["fc0.weight"].shape) == (spec.units[0], spec.n_flat)
    back = net.cnn_weights_from_torch(sd, spec)
    for (Wp, bp), (Wb, bb) in zip(pairs, back):
        assert np.array_equal(Wp.view(np.uint32), Wb.view(np.uint32)) and np.array_equal(bp.view(np.uint32), bb.view(np.uint32))
    # ... into a module: torch's own forward (Flatten of NCHW) on it is the model's, up to float64 against float32 chains
    layers, cin, side = [], spec.channels, spec.side
    for k, s, f in spec.convs:
        layers += [torch.nn.Conv2d(cin, f, k, s), torch.nn.ReLU()]
        cin = f
    layers.append(torch.nn.Flatten())
    n = spec.n_flat
    for i, u in enumerate(spec.units):
        layers += [torch.nn.Linear(n, u)] + ([torch.nn.ReLU()] if i + 1 < len(spec.units) else [])
        n = u
    mod = torch.nn.Sequential(*layers)
    assert net.cnn_weights_to_torch(pairs, spec, mod) is mod
    for (Wp, bp), (Wb, bb) in zip(pairs, net.cnn_weights_from_torch(mod, spec)):
        assert np.array_equal(Wp.view(np.uint32), Wb.view(np.uint32)) and np.array_equal(bp.view(np.uint32), bb.view(np.uint32))
    with pytest.raises(ValueError, match="pairs given"):
        net.cnn_weights_to_torch(pairs[:-1], spec)
    with pytest.raises(ValueError, match="expected kernels of shapes"):
        net.cnn_weights_to_torch([(W.T if W.ndim == 2 else W, b) for W, b in pairs], spec)
