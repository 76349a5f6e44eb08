"""The SPG trainer's C-ABI (include/aigar.h, aigar_spg*): declared, laid out as the ctypes mirror
has it, exported, additions only (ABI 7), and refused loudly.  CPU only: aigar_spg_config checks
its parameters before its handle, so every bad parameter set is seen here with its own message;
the refusals that need a live handle are in tests/test_gpu_spg.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_spg_config", "aigar_spg_step", "aigar_spg_info", "aigar_spg_td", "aigar_spg_noise", "aigar_spg_sync_target",
         "aigar_spg_reset")
FIELDS = ("batch", "min_size", "target_steps", "reserved", "critic_lr", "actor_lr", "beta1", "beta2", "epsilon",
          "discount", "tau", "q_increase", "samples", "moving", "replace", "prio_evals", "fused", "pad", "noise",
          "noise_decay", "seed")


def test_header_declares_the_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_spg_params \{", txt)
    assert re.search(r"#define AIGAR_SPG_MAX_SAMPLES 8\b", txt) and _abi.SPG_MAX_SAMPLES == 8
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_spg_params_layout_matches_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_spg_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_spg_params, %s));\n' % f
    src += 'printf(" %d\\n", AIGAR_ABI_VERSION);return 0;}'
    exe = str(tmp_path / "spg_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.SpgParams) == 128
    for f, off in zip(FIELDS, v[1:1 + len(FIELDS)]):
        assert off == getattr(_abi.SpgParams, f).offset, f
    # the fields of aigar_dpg_params come first, where aigar_dpg_params has them
    for f, _ in _abi.DpgParams._fields_:
        assert getattr(_abi.SpgParams, f).offset == getattr(_abi.DpgParams, f).offset, f
    assert v[1 + len(FIELDS):] == [_abi.ABI_VERSION] == [7]
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"spg.inc"' in build  # (stale() sees the kernels' file)
    assert "static_assert(sizeof(aigar_spg_params) == 128" in open(os.path.join(ROOT, "aigar_amd", "csrc", "api.hip")).read()


def test_library_exports_the_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    good = _p()
    info = (C.c_int64 * 8)()
    ptr = C.c_void_p()
    for r in (L.aigar_spg_config(None, None), L.aigar_spg_config(None, C.byref(good)), L.aigar_spg_step(None, 1, None, None),
              L.aigar_spg_info(None, info), L.aigar_spg_td(None, None, None), L.aigar_spg_noise(None, C.byref(ptr)),
              L.aigar_spg_sync_target(None), L.aigar_spg_reset(None)):
        assert r < 0 and b"null handle" in L.aigar_last_error()


def _p(**kw):
    d = dict(batch=32, min_size=0, target_steps=0, reserved=0, critic_lr=5e-4, actor_lr=1e-4, beta1=0.9, beta2=0.999,
             epsilon=1e-7, discount=0.9, tau=0.001, q_increase=0.0, samples=5, moving=1, replace=1, prio_evals=1, fused=0,
             pad=0, noise=1.0, noise_decay=0.999, seed=0)
    d.update(kw)
    return _abi.SpgParams(*[d[f] for f in FIELDS])


@pytest.mark.parametrize("p, word", [
    (_p(batch=0), b"batch = 0"), (_p(batch=257), b"batch = 257"), (_p(min_size=-1), b"min_size = -1"),
    (_p(target_steps=-1), b"target_steps = -1"), (_p(reserved=1), b"reserved = 1"),
    (_p(samples=-1), b"samples = -1"), (_p(samples=9), b"samples = 9"), (_p(moving=2), b"moving = 2"),
    (_p(replace=-1), b"replace = -1"), (_p(prio_evals=2), b"prio_evals = 2"), (_p(fused=-1), b"fused = -1"),
    (_p(fused=2), b"fused = 2"), (_p(pad=1), b"pad = 1"),
    (_p(critic_lr=0.0), b"critic_lr = 0"), (_p(critic_lr=float("nan")), b"critic_lr = nan"),
    (_p(actor_lr=0.0), b"actor_lr = 0"), (_p(actor_lr=float("inf")), b"actor_lr = inf"),
    (_p(beta1=1.0), b"beta1 = 1"), (_p(beta2=float("nan")), b"beta2 = nan"), (_p(epsilon=0.0), b"epsilon = 0"),
    (_p(discount=1.5), b"discount = 1.5"), (_p(tau=-0.001), b"tau = -0.001"), (_p(tau=float("nan")), b"tau = nan"),
    (_p(q_increase=float("inf")), b"q_increase = inf"),
    (_p(noise=-0.5), b"noise = -0.5"), (_p(noise=float("inf")), b"noise = inf"), (_p(noise=float("nan")), b"noise = nan"),
    (_p(noise_decay=0.0), b"noise_decay = 0"), (_p(noise_decay=1.5), b"noise_decay = 1.5"),
    (_p(noise_decay=float("nan")), b"noise_decay = nan"),
])
def test_spg_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_spg_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"spg_config" in msg and word in msg, msg


def test_edge_values_pass_the_parameter_checks():
    L = _lib.load()
    for p in (_p(batch=1), _p(batch=256), _p(samples=0), _p(samples=8), _p(moving=0, replace=0, prio_evals=0), _p(fused=1), _p(noise=0.0),
              _p(noise_decay=1.0), _p(noise_decay=5e-324), _p(tau=0.0), _p(tau=1.0), _p(seed=2 ** 64 - 1)):
        assert L.aigar_spg_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    from aigar_amd.env import AgarSpgEnv, AgarVecEnv
    for m in ("spg_config", "spg_step", "spg_info", "spg_td", "spg_noise_ptr", "spg_sync_target", "spg_reset"):
        assert callable(getattr(_lib.Stepper, m))
    assert issubclass(AgarSpgEnv, AgarVecEnv)
    sig = inspect.signature(AgarSpgEnv.__init__).parameters
    assert sig["search"].default is None and sig["search"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(AgarSpgEnv.train).parameters) == ["self", "n", "u", "zu"]
    assert isinstance(AgarSpgEnv.search_noise, property)
    # AgarVecEnv's own recorded surface stays: the keyword is the new class's
    assert "search" not in inspect.signature(AgarVecEnv.__init__).parameters
    assert list(inspect.signature(AgarVecEnv.train).parameters) == ["self", "n", "u"]
    assert list(inspect.signature(_lib.Stepper.spg_step).parameters) == ["self", "n", "u", "zu"]


def test_spg_params_reads_the_reference_defaults_and_refuses_by_name():
    want = dict(batch=32, min_size=32, target_steps=1500, critic_lr=0.0005, actor_lr=0.0001, beta1=0.9, beta2=0.999,
                epsilon=1e-7, discount=0.9, tau=0.001, samples=5, moving=True, replace=False, prio_evals=True, fused=True,
                noise=1.0, noise_decay=0.0004 ** (1.0 / 500000), seed=0)
    assert net.spg_params(None) == want
    assert net.spg_params(dict(ALGORITHM="SPG", OCACLA_ENABLED=True)) == want
    assert set(want) == set(inspect.signature(_lib.Stepper.spg_config).parameters) - {"self"}  # (what spg_config takes)
    got = net.spg_params(dict(OCACLA_EXPL_SAMPLES=8, OCACLA_MOVING_GAUSSIAN=False, OCACLA_REPLACE_TRANSITIONS=True,
                              OCACLA_NOISE=0.25, OCACLA_NOISE_DECAY=0.5, DPG_CRITIC_ALPHA=0.01, DPG_ACTOR_ALPHA=0.02,
                              DISCOUNT=0.5, MEMORY_BATCH_LEN=8, TARGET_NETWORK_STEPS=7, NUM_EXPS_BEFORE_TRAIN=100,
                              DPG_TAU=0.5, DPG_Q_VAL_INCREASE=3))
    assert got == dict(want, batch=8, min_size=100, target_steps=7, critic_lr=0.01, actor_lr=0.02, discount=0.5, tau=0.5,
                       samples=8, moving=False, replace=True, noise=0.25, noise_decay=0.5)
    assert net.spg_params(dict(SOFT_TARGET_UPDATES=False))["tau"] == 0.0
    for kw, word in ((dict(ALGORITHM="DPG"), "ALGORITHM"), (dict(ALGORITHM="CACLA"), "ALGORITHM"),
                     (dict(OCACLA_ONLINE_SAMPLES=3), "OCACLA_ONLINE_SAMPLES"), (dict(NOISE_TYPE="Orn-Uhl"), "NOISE_TYPE"),
                     (dict(CNN_REPR=True), "CNN_REPR"), (dict(OCACLA_EXPL_SAMPLES=9), "OCACLA_EXPL_SAMPLES"),
                     (dict(ACTOR_IS=True), "ACTOR_IS"), (dict(AMSGRAD=True), "AMSGRAD"), (dict(OPTIMIZER="SGD"), "OPTIMIZER"),
                     (dict(AC_ACTOR_TRAINING_START=100), "AC_ACTOR_TRAINING_START"), (dict(DROPOUT=0.2), "DROPOUT"),
                     (dict(DPG_FEED_ACTION_IN_LAYER=2), "DPG_FEED_ACTION_IN_LAYER"),
                     (dict(DPG_USE_TARGET_MODELS=False), "DPG_USE_TARGET_MODELS"), (dict(DPG_USE_CACLA=True), "DPG_USE_CACLA"),
                     (dict(NEURON_TYPE="LSTM"), "NEURON_TYPE"), (dict(TD=1), "TD")):
        with pytest.raises(ValueError, match="^spg: .*" + word):
            net.spg_params(kw)
    with pytest.raises(ValueError, match="OCACLA_ENABLED"):  # the DPG trainer still refuses it by name
        net.dpg_params(dict(OCACLA_ENABLED=True))
