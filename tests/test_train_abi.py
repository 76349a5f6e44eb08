"""The trainer's C-ABI (include/aigar.h, aigar_train*, aigar_net_get_weights): declared, laid
out as the ctypes mirror has it, exported, additions only (ABI 7), and refused loudly.  CPU
only: aigar_train_config checks its parameters before its handle, so every bad parameter set
is seen here with its own message; the refusals that need a live handle (no network, a
sigmoid head, a conv part, no memory, a tiled handle) are in tests/test_gpu_train.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_train_config", "aigar_train_step", "aigar_train_info", "aigar_train_td", "aigar_train_sync_target",
         "aigar_train_reset", "aigar_net_get_weights", "aigar_net_pad_check")
FIELDS = ("batch", "min_size", "target_steps", "pad", "lr", "beta1", "beta2", "epsilon", "discount")


def test_header_declares_the_trainer_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_train_params \{", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_train_params_layout_and_constants_match_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_train_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_train_params, %s));\n' % f
    src += 'printf(" %d %d\\n", AIGAR_WARN_TRAIN_NONFINITE, AIGAR_ABI_VERSION);return 0;}'
    exe = str(tmp_path / "train_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.TrainParams) == 56
    for f, off in zip(FIELDS, v[1:1 + len(FIELDS)]):
        assert off == getattr(_abi.TrainParams, f).offset, f
    assert v[1 + len(FIELDS):] == [_abi.WARN_TRAIN_NONFINITE, _abi.ABI_VERSION] == [0x40, 7]
    inc = open(os.path.join(ROOT, "aigar_amd", "csrc", "train.inc")).read()
    assert re.search(r"kTrainMaxBatch = %d\b" % _abi.TRAIN_MAX_BATCH, inc)
    dev = open(os.path.join(ROOT, "aigar_amd", "csrc", "aigar_dev.h")).read()
    assert re.search(r"WARN_TRAIN_NONFINITE = 64\b", dev)
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"train.inc"' in build  # (stale() sees the kernels' file)


def test_library_exports_the_trainer_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    good = _abi.TrainParams(32, 32, 1500, 0, 1e-3, 0.9, 0.999, 1e-7, 0.9)
    assert L.aigar_train_config(None, None) < 0 and b"null handle" in L.aigar_last_error()
    assert L.aigar_train_config(None, C.byref(good)) < 0 and b"null handle" in L.aigar_last_error()
    info = (C.c_int64 * 4)()
    n = C.c_int64()
    for r in (L.aigar_train_step(None, 1, None), L.aigar_train_info(None, info), L.aigar_train_td(None, None, None),
              L.aigar_train_sync_target(None), L.aigar_train_reset(None),
              L.aigar_net_get_weights(None, 0, 0, None, None, 0), L.aigar_net_pad_check(None, 0, C.byref(n))):
        assert r < 0 and b"null handle" in L.aigar_last_error()


def _p(**kw):
    d = dict(batch=32, min_size=0, target_steps=0, pad=0, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9)
    d.update(kw)
    return _abi.TrainParams(*[d[f] for f in FIELDS])


@pytest.mark.parametrize("p, word", [
    (_p(batch=0), b"batch = 0"), (_p(batch=257), b"batch = 257"), (_p(batch=-3), b"batch = -3"),
    (_p(min_size=-1), b"min_size = -1"), (_p(target_steps=-1), b"target_steps = -1"),
    (_p(lr=0.0), b"lr = 0"), (_p(lr=-1e-3), b"lr = -0.001"), (_p(lr=float("nan")), b"lr = nan"),
    (_p(lr=float("inf")), b"lr = inf"),
    (_p(beta1=1.0), b"beta1 = 1"), (_p(beta1=-0.1), b"beta1 = -0.1"), (_p(beta2=1.0), b"beta2 = 1"),
    (_p(beta2=float("nan")), b"beta2 = nan"),
    (_p(epsilon=0.0), b"epsilon = 0"), (_p(epsilon=-1e-7), b"epsilon = -1e-07"),
    (_p(discount=1.5), b"discount = 1.5"), (_p(discount=-0.1), b"discount = -0.1"),
])
def test_train_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_train_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"train_config" in msg and word in msg, msg


def test_edge_values_pass_the_parameter_checks():
    L = _lib.load()
    for p in (_p(batch=1), _p(batch=256), _p(beta1=0.0, beta2=0.0), _p(discount=0.0), _p(discount=1.0)):
        assert L.aigar_train_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("train_config", "train_step", "train_info", "train_td", "train_sync_target", "train_reset",
              "net_get_weights", "net_pad_check"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("train", "train_info", "train_td", "get_weights"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["train"].default is None  # off unless asked for
    assert callable(net.weights_to_torch) and callable(net.train_params)


def test_train_params_reads_the_reference_defaults_and_refuses_by_name():
    assert net.train_params(None) == dict(batch=32, min_size=32, target_steps=1500, lr=0.001, beta1=0.9, beta2=0.999,
                                          epsilon=1e-7, discount=0.9)
    got = net.train_params(dict(ALPHA=0.01, DISCOUNT=0.5, MEMORY_BATCH_LEN=8, TARGET_NETWORK_STEPS=0,
                                NUM_EXPS_BEFORE_TRAIN=100))
    assert (got["lr"], got["discount"], got["batch"], got["target_steps"], got["min_size"]) == (0.01, 0.5, 8, 0, 100)
    for kw, word in ((dict(OPTIMIZER="SGD"), "OPTIMIZER"), (dict(AMSGRAD=True), "AMSGRAD"),
                     (dict(GRADIENT_CLIP=0.5), "GRADIENT_CLIP"), (dict(GRADIENT_CLIP_NORM=1), "GRADIENT_CLIP_NORM"),
                     (dict(Q_WEIGHT_DECAY=1e-3), "Q_WEIGHT_DECAY"), (dict(DROPOUT=0.2), "DROPOUT"),
                     (dict(ENABLE_QV=True), "ENABLE_QV"), (dict(USE_ACTION_AS_INPUT=True), "USE_ACTION_AS_INPUT"),
                     (dict(END_DISCOUNT=0.85), "END_DISCOUNT"), (dict(NEURON_TYPE="LSTM"), "LSTM"), (dict(TD=1), "TD"),
                     (dict(CNN_REPR=True), "CNN_REPR")):
        with pytest.raises(ValueError, match=word):
            net.train_params(kw)


def test_weights_to_torch_is_the_inverse_of_weights_from_torch():
    import numpy as np
    import torch
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    w = net.weights_from_torch(m)
    m2 = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))
    assert net.weights_to_torch(w, m2) is m2
    for (W, b), (W2, b2) in zip(w, net.weights_from_torch(m2)):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)
    assert torch.equal(m[0].weight, m2[0].weight) and torch.equal(m[2].bias, m2[2].bias)
    with pytest.raises(ValueError, match="2 layers given"):
        net.weights_to_torch(w, torch.nn.Linear(3, 5))
    with pytest.raises(ValueError, match="the layer takes"):
        net.weights_to_torch(w, torch.nn.Sequential(torch.nn.Linear(4, 5), torch.nn.Linear(5, 2)))
