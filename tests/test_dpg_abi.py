"""The DPG trainer's C-ABI (include/aigar.h, aigar_qcritic_config, aigar_dpg*): declared, laid out
as the ctypes mirror has it, exported, additions only (ABI 7), and refused loudly.  CPU only:
aigar_qcritic_config and aigar_dpg_config check their parameters before their handle, so every
bad parameter set is seen here with its own message; the refusals that need a live handle are in
tests/test_gpu_dpg.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_qcritic_config", "aigar_dpg_config", "aigar_dpg_step", "aigar_dpg_info", "aigar_dpg_td",
         "aigar_dpg_sync_target", "aigar_dpg_reset")
FIELDS = ("batch", "min_size", "target_steps", "reserved", "critic_lr", "actor_lr", "beta1", "beta2", "epsilon",
          "discount", "tau", "q_increase")


def test_header_declares_the_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_dpg_params \{", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_dpg_params_layout_matches_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_dpg_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_dpg_params, %s));\n' % f
    src += 'printf(" %d\\n", AIGAR_ABI_VERSION);return 0;}'
    exe = str(tmp_path / "dpg_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.DpgParams) == 80
    for f, off in zip(FIELDS, v[1:1 + len(FIELDS)]):
        assert off == getattr(_abi.DpgParams, f).offset, f
    assert v[1 + len(FIELDS):] == [_abi.ABI_VERSION] == [7]
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"dpg.inc"' in build  # (stale() sees the kernels' file)


def test_library_exports_the_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    good = _p()
    crit = _c()
    info = (C.c_int64 * 8)()
    for r in (L.aigar_qcritic_config(None, None), L.aigar_qcritic_config(None, C.byref(crit)),
              L.aigar_dpg_config(None, None), L.aigar_dpg_config(None, C.byref(good)), L.aigar_dpg_step(None, 1, None),
              L.aigar_dpg_info(None, info), L.aigar_dpg_td(None, None, None), L.aigar_dpg_sync_target(None),
              L.aigar_dpg_reset(None)):
        assert r < 0 and b"null handle" in L.aigar_last_error()


def _p(**kw):
    d = dict(batch=32, min_size=0, target_steps=0, reserved=0, critic_lr=5e-4, actor_lr=1e-4, beta1=0.9, beta2=0.999,
             epsilon=1e-7, discount=0.9, tau=0.001, q_increase=2.0)
    d.update(kw)
    return _abi.DpgParams(*[d[f] for f in FIELDS])


def _c(n_layers=3, n_in=66, x_dtype=0, hidden=_abi.ACT_RELU, out=_abi.ACT_LINEAR, units=(100, 100, 1)):
    p = _abi.NetParams(n_layers, n_in, x_dtype, hidden, out, 0)
    for i, v in enumerate(units):
        p.units[i] = v
    return p


@pytest.mark.parametrize("p, word", [
    (_p(batch=0), b"batch = 0"), (_p(batch=257), b"batch = 257"), (_p(batch=-3), b"batch = -3"),
    (_p(min_size=-1), b"min_size = -1"), (_p(target_steps=-1), b"target_steps = -1"), (_p(reserved=1), b"reserved = 1"),
    (_p(critic_lr=0.0), b"critic_lr = 0"), (_p(critic_lr=float("nan")), b"critic_lr = nan"),
    (_p(critic_lr=float("inf")), b"critic_lr = inf"),
    (_p(actor_lr=0.0), b"actor_lr = 0"), (_p(actor_lr=-1e-3), b"actor_lr = -0.001"), (_p(actor_lr=float("inf")), b"actor_lr = inf"),
    (_p(beta1=1.0), b"beta1 = 1"), (_p(beta1=-0.1), b"beta1 = -0.1"), (_p(beta2=1.0), b"beta2 = 1"),
    (_p(beta2=float("nan")), b"beta2 = nan"),
    (_p(epsilon=0.0), b"epsilon = 0"), (_p(epsilon=-1e-7), b"epsilon = -1e-07"),
    (_p(discount=1.5), b"discount = 1.5"), (_p(discount=-0.1), b"discount = -0.1"),
    (_p(tau=-0.001), b"tau = -0.001"), (_p(tau=1.5), b"tau = 1.5"), (_p(tau=float("nan")), b"tau = nan"),
    (_p(q_increase=float("inf")), b"q_increase = inf"), (_p(q_increase=float("-inf")), b"q_increase = -inf"),
    (_p(q_increase=float("nan")), b"q_increase = nan"),
])
def test_dpg_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_dpg_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"dpg_config" in msg and word in msg, msg


@pytest.mark.parametrize("p, word", [
    (_c(n_layers=0), b"n_layers = 0"), (_c(n_layers=6, units=(4, 4, 4, 4, 4, 1)), b"n_layers = 6"),
    (_c(n_in=0), b"n_in = 0"), (_c(n_in=16385), b"n_in = 16385"),
    (_c(units=(100, 257, 1)), b"layer 1 has 257 units"), (_c(units=(0, 100, 1)), b"layer 0 has 0 units"),
    (_c(x_dtype=2), b"x_dtype"), (_c(hidden=_abi.ACT_TANH), b"hidden activation 4 (tanh)"),
    (_c(units=(100, 100, 2)), b"the head has 2 units"), (_c(out=_abi.ACT_SIGMOID), b"activation 2 (sigmoid)"),
])
def test_qcritic_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_qcritic_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"qcritic_config" in msg and word in msg, msg
    assert L.aigar_critic_config(None, C.byref(p)) < 0  # ... and the V(s) entry keeps its own name
    assert b"qcritic_config" not in L.aigar_last_error() and b"critic_config" in L.aigar_last_error()


def test_edge_values_pass_the_parameter_checks():
    L = _lib.load()
    for p in (_p(batch=1), _p(batch=256), _p(beta1=0.0, beta2=0.0), _p(discount=0.0), _p(discount=1.0), _p(tau=0.0),
              _p(tau=1.0), _p(tau=5e-324), _p(q_increase=0.0), _p(q_increase=-1e300)):
        assert L.aigar_dpg_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()
    for p in (_c(n_layers=1, units=(1,)), _c(n_layers=5, units=(256, 256, 256, 256, 1)), _c(hidden=_abi.ACT_LINEAR, x_dtype=1)):
        assert L.aigar_qcritic_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("qcritic_config", "dpg_config", "dpg_step", "dpg_info", "dpg_td", "dpg_sync_target", "dpg_reset"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("set_critic_weights", "get_critic_weights", "q_value", "train", "train_info", "train_td"):
        assert callable(getattr(AgarVecEnv, m))
    sig = inspect.signature(AgarVecEnv.__init__).parameters
    assert sig["train"].default is None and sig["critic"].default is None
    assert list(inspect.signature(AgarVecEnv.q_value).parameters) == ["self", "states", "actions"]
    assert 'train="dpg"' in inspect.getmodule(AgarVecEnv).__doc__


def test_dpg_params_reads_the_reference_defaults_and_refuses_by_name():
    want = dict(batch=32, min_size=32, target_steps=1500, critic_lr=0.0005, actor_lr=0.0001, beta1=0.9, beta2=0.999,
                epsilon=1e-7, discount=0.9, tau=0.001, q_increase=2.0)
    assert net.dpg_params(None) == want
    assert net.dpg_params(dict(ALGORITHM="DPG")) == want
    assert set(want) | {"reserved"} == set(FIELDS)  # (what Stepper.dpg_config takes)
    got = net.dpg_params(dict(DPG_CRITIC_ALPHA=0.01, DPG_ACTOR_ALPHA=0.02, DISCOUNT=0.5, MEMORY_BATCH_LEN=8,
                              TARGET_NETWORK_STEPS=7, NUM_EXPS_BEFORE_TRAIN=100, DPG_TAU=0.5, DPG_Q_VAL_INCREASE=0))
    assert got == dict(batch=8, min_size=100, target_steps=7, critic_lr=0.01, actor_lr=0.02, beta1=0.9, beta2=0.999,
                       epsilon=1e-7, discount=0.5, tau=0.5, q_increase=0.0)
    hard = net.dpg_params(dict(SOFT_TARGET_UPDATES=False, DPG_TAU=0.5, TARGET_NETWORK_STEPS=7))
    assert hard["tau"] == 0.0 and hard["target_steps"] == 7
    for kw, word in ((dict(ALGORITHM="CACLA"), "ALGORITHM"), (dict(ALGORITHM="Q-learning"), "ALGORITHM"),
                     (dict(OCACLA_ENABLED=True), "OCACLA_ENABLED"),
                     (dict(CACLA_UPDATE_ON_NEGATIVE_TD=True), "CACLA_UPDATE_ON_NEGATIVE_TD"),
                     (dict(CACLA_CRITIC_WEIGHT_DECAY=1e-3), "CACLA_CRITIC_WEIGHT_DECAY"),
                     (dict(CACLA_OFF_POLICY_CORR=1), "CACLA_OFF_POLICY_CORR"), (dict(ACTOR_IS=True), "ACTOR_IS"),
                     (dict(AC_ACTOR_TDE=0.5), "AC_ACTOR_TDE"), (dict(AC_DELAY_ACTOR_TRAINING=0.1), "AC_DELAY_ACTOR_TRAINING"),
                     (dict(AMSGRAD=True), "AMSGRAD"), (dict(OPTIMIZER_POLICY="SGD"), "OPTIMIZER_POLICY"),
                     (dict(OPTIMIZER="SGD"), "OPTIMIZER"), (dict(END_DISCOUNT=0.85), "END_DISCOUNT"),
                     (dict(DROPOUT=0.2), "DROPOUT"), (dict(GRADIENT_CLIP=0.5), "GRADIENT_CLIP"),
                     (dict(GRADIENT_CLIP_NORM=1), "GRADIENT_CLIP_NORM"),
                     (dict(DPG_FEED_ACTION_IN_LAYER=2), "DPG_FEED_ACTION_IN_LAYER"),
                     (dict(DPG_USE_TARGET_MODELS=False), "DPG_USE_TARGET_MODELS"),
                     (dict(DPG_USE_DPG_ACTOR_TRAINING=False), "DPG_USE_DPG_ACTOR_TRAINING"),
                     (dict(DPG_USE_CACLA=True), "DPG_USE_CACLA"), (dict(DPG_CACLA_ALTERNATION=0.5), "DPG_CACLA_ALTERNATION"),
                     (dict(DPG_CACLA_INV_ALTERNATION=0.5), "DPG_CACLA_INV_ALTERNATION"),
                     (dict(DPG_CRITIC_WEIGHT_DECAY=1e-3), "DPG_CRITIC_WEIGHT_DECAY"),
                     (dict(DPG_ACTOR_OPTIMIZER="SGD"), "DPG_ACTOR_OPTIMIZER"), (dict(DPG_ACTOR_NESTEROV=0.9), "DPG_ACTOR_NESTEROV")):
        with pytest.raises(ValueError, match=word):
            net.dpg_params(kw)
    with pytest.raises(ValueError, match="ALGORITHM.*train='dpg'"):  # the CACLA trainer's refusal names the way here
        net.actrain_params(dict(ALGORITHM="DPG"))


def test_qcritic_spec_reads_the_reference_defaults():
    assert net.qcritic_spec(None, n_in=854, n_act=2) == net.NetSpec(856, (100, 100, 1), "relu", "linear")
    assert net.qcritic_spec(dict(DPG_CRITIC_LAYERS=(50, 0, 20), DPG_CRITIC_FUNC="linear")) == \
        net.NetSpec(None, (50, 20, 1), "linear", "linear")
    # the critic's activation is its own setting, not the actor's
    assert net.qcritic_spec(dict(ACTIVATION_FUNC_HIDDEN="elu", CACLA_CRITIC_LAYERS=(7,)), 10, 4).units == (100, 100, 1)
    with pytest.raises(ValueError, match="DPG_CRITIC_FUNC"):
        net.qcritic_spec(dict(DPG_CRITIC_FUNC="elu"))
    with pytest.raises(ValueError, match="hidden layers"):
        net.qcritic_spec(dict(DPG_CRITIC_LAYERS=(4, 4, 4, 4, 4)))
    with pytest.raises(ValueError, match="actions"):
        net.qcritic_spec(None, 10, 5)
