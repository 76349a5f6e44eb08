"""The CACLA trainer's C-ABI (include/aigar.h, aigar_critic*, aigar_actrain*): declared, laid out
as the ctypes mirror has it, exported, additions only (ABI 7), and refused loudly.  CPU only:
aigar_critic_config and aigar_actrain_config check their parameters before their handle, so
every bad parameter set is seen here with its own message; the refusals that need a live
handle are in tests/test_gpu_actrain.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aigar_amd import _abi, _lib, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_critic_config", "aigar_critic_set_weights", "aigar_critic_forward", "aigar_actrain_config",
         "aigar_actrain_step", "aigar_actrain_info", "aigar_actrain_td", "aigar_actrain_var", "aigar_actrain_sync_target",
         "aigar_actrain_reset")
FIELDS = ("batch", "min_size", "target_steps", "var_epochs", "critic_lr", "actor_lr", "beta1", "beta2", "epsilon",
          "discount", "var_start", "var_beta")


def test_header_declares_the_calls_and_is_still_abi_7():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_actrain_params \{", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_actrain_params_layout_and_constants_match_header(tmp_path):
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_actrain_params));\n' % HEADER
    for f in FIELDS:
        src += 'printf(" %%zu", offsetof(aigar_actrain_params, %s));\n' % f
    src += 'printf(" %d %d\\n", AIGAR_ACTRAIN_MAX_EPOCHS, AIGAR_ABI_VERSION);return 0;}'
    exe = str(tmp_path / "actrain_hdr_check")
    subprocess.run(["cc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.ActrainParams) == 80
    for f, off in zip(FIELDS, v[1:1 + len(FIELDS)]):
        assert off == getattr(_abi.ActrainParams, f).offset, f
    assert v[1 + len(FIELDS):] == [_abi.ACTRAIN_MAX_EPOCHS, _abi.ABI_VERSION] == [8, 7]
    build = open(os.path.join(ROOT, "aigar_amd", "_build.py")).read()
    assert '"actrain.inc"' in build  # (stale() sees the kernels' file)
    assert (_abi.NET_CRITIC, _abi.NET_CRITIC_TARGET, _abi.NET_CRITIC_M, _abi.NET_CRITIC_V) == (4, 5, 6, 7)


def test_library_exports_the_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    good = _p()
    crit = _c()
    info = (C.c_int64 * 8)()
    var = C.c_double()
    n = C.c_int64()
    for r in (L.aigar_critic_config(None, None), L.aigar_critic_config(None, C.byref(crit)),
              L.aigar_critic_set_weights(None, 0, None, None, 0), L.aigar_critic_forward(None, None, 0, 1, None),
              L.aigar_actrain_config(None, None), L.aigar_actrain_config(None, C.byref(good)),
              L.aigar_actrain_step(None, 1, None), L.aigar_actrain_info(None, info),
              L.aigar_actrain_td(None, None, None, None), L.aigar_actrain_var(None, C.byref(var)),
              L.aigar_actrain_sync_target(None), L.aigar_actrain_reset(None),
              L.aigar_net_get_weights(None, 4, 0, None, None, 0), L.aigar_net_pad_check(None, 5, C.byref(n))):
        assert r < 0 and b"null handle" in L.aigar_last_error()


def _p(**kw):
    d = dict(batch=32, min_size=0, target_steps=0, var_epochs=8, critic_lr=7.5e-5, actor_lr=5e-4, beta1=0.9, beta2=0.999,
             epsilon=1e-7, discount=0.9, var_start=1.0, var_beta=0.001)
    d.update(kw)
    return _abi.ActrainParams(*[d[f] for f in FIELDS])


def _c(n_layers=3, n_in=64, x_dtype=0, hidden=_abi.ACT_RELU, out=_abi.ACT_LINEAR, units=(100, 100, 1)):
    p = _abi.NetParams(n_layers, n_in, x_dtype, hidden, out, 0)
    for i, v in enumerate(units):
        p.units[i] = v
    return p


@pytest.mark.parametrize("p, word", [
    (_p(batch=0), b"batch = 0"), (_p(batch=257), b"batch = 257"), (_p(batch=-3), b"batch = -3"),
    (_p(min_size=-1), b"min_size = -1"), (_p(target_steps=-1), b"target_steps = -1"),
    (_p(var_epochs=-1), b"var_epochs = -1"), (_p(var_epochs=9), b"var_epochs = 9"),
    (_p(critic_lr=0.0), b"critic_lr = 0"), (_p(critic_lr=float("nan")), b"critic_lr = nan"),
    (_p(critic_lr=float("inf")), b"critic_lr = inf"),
    (_p(actor_lr=0.0), b"actor_lr = 0"), (_p(actor_lr=-1e-3), b"actor_lr = -0.001"), (_p(actor_lr=float("inf")), b"actor_lr = inf"),
    (_p(beta1=1.0), b"beta1 = 1"), (_p(beta1=-0.1), b"beta1 = -0.1"), (_p(beta2=1.0), b"beta2 = 1"),
    (_p(beta2=float("nan")), b"beta2 = nan"),
    (_p(epsilon=0.0), b"epsilon = 0"), (_p(epsilon=-1e-7), b"epsilon = -1e-07"),
    (_p(discount=1.5), b"discount = 1.5"), (_p(discount=-0.1), b"discount = -0.1"),
    (_p(var_start=0.0), b"var_start = 0"), (_p(var_start=-1.0), b"var_start = -1"), (_p(var_start=float("inf")), b"var_start = inf"),
    (_p(var_beta=1.0), b"var_beta = 1"), (_p(var_beta=-0.5), b"var_beta = -0.5"), (_p(var_beta=float("nan")), b"var_beta = nan"),
])
def test_actrain_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_actrain_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"actrain_config" in msg and word in msg, msg


@pytest.mark.parametrize("p, word", [
    (_c(n_layers=0), b"n_layers = 0"), (_c(n_layers=6, units=(4, 4, 4, 4, 4, 1)), b"n_layers = 6"),
    (_c(n_in=0), b"n_in = 0"), (_c(n_in=16385), b"n_in = 16385"),
    (_c(units=(100, 257, 1)), b"layer 1 has 257 units"), (_c(units=(0, 100, 1)), b"layer 0 has 0 units"),
    (_c(x_dtype=2), b"x_dtype"), (_c(hidden=_abi.ACT_TANH), b"hidden activation 4 (tanh)"),
    (_c(units=(100, 100, 2)), b"the head has 2 units"), (_c(out=_abi.ACT_SIGMOID), b"activation 2 (sigmoid)"),
])
def test_critic_config_refuses_bad_parameters_with_a_message(p, word):
    L = _lib.load()
    assert L.aigar_critic_config(None, C.byref(p)) < 0
    msg = L.aigar_last_error()
    assert b"critic_config" in msg and word in msg, msg


def test_edge_values_pass_the_parameter_checks():
    L = _lib.load()
    for p in (_p(batch=1), _p(batch=256), _p(var_epochs=0), _p(beta1=0.0, beta2=0.0), _p(discount=0.0), _p(discount=1.0),
              _p(var_beta=0.0), _p(var_start=5e-324)):
        assert L.aigar_actrain_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()
    for p in (_c(n_layers=1, units=(1,)), _c(n_layers=5, units=(256, 256, 256, 256, 1)), _c(hidden=_abi.ACT_LINEAR, x_dtype=1)):
        assert L.aigar_critic_config(None, C.byref(p)) < 0 and b"null handle" in L.aigar_last_error()


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("critic_config", "critic_set_weights", "critic_get_weights", "critic_forward", "actrain_config", "actrain_step",
              "actrain_info", "actrain_td", "actrain_var", "actrain_sync_target", "actrain_reset"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("set_critic_weights", "get_critic_weights", "critic_value", "cacla_var"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["critic"].default is None


def test_actrain_params_reads_the_reference_defaults_and_refuses_by_name():
    assert net.actrain_params(None) == dict(batch=32, min_size=32, target_steps=1500, var_epochs=8, critic_lr=0.000075,
                                            actor_lr=0.0005, beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9,
                                            var_start=1.0, var_beta=0.001)
    got = net.actrain_params(dict(CACLA_CRITIC_ALPHA=0.01, CACLA_ACTOR_ALPHA=0.02, DISCOUNT=0.5, MEMORY_BATCH_LEN=8,
                                  TARGET_NETWORK_STEPS=0, NUM_EXPS_BEFORE_TRAIN=100, CACLA_VAR_ENABLED=False,
                                  CACLA_VAR_START=2, CACLA_VAR_BETA=0.01))
    assert got == dict(batch=8, min_size=100, target_steps=0, var_epochs=0, critic_lr=0.01, actor_lr=0.02, beta1=0.9,
                       beta2=0.999, epsilon=1e-7, discount=0.5, var_start=2.0, var_beta=0.01)
    for kw, word in ((dict(ALGORITHM="DPG"), "ALGORITHM"), (dict(ALGORITHM="Q-learning"), "ALGORITHM"),
                     (dict(OCACLA_ENABLED=True), "OCACLA_ENABLED"),
                     (dict(CACLA_UPDATE_ON_NEGATIVE_TD=True), "CACLA_UPDATE_ON_NEGATIVE_TD"),
                     (dict(CACLA_CRITIC_WEIGHT_DECAY=1e-3), "CACLA_CRITIC_WEIGHT_DECAY"),
                     (dict(CACLA_OFF_POLICY_CORR=1), "CACLA_OFF_POLICY_CORR"), (dict(ACTOR_IS=True), "ACTOR_IS"),
                     (dict(AC_ACTOR_TDE=0.5), "AC_ACTOR_TDE"), (dict(AC_DELAY_ACTOR_TRAINING=0.1), "AC_DELAY_ACTOR_TRAINING"),
                     (dict(AMSGRAD=True), "AMSGRAD"), (dict(OPTIMIZER_POLICY="SGD"), "OPTIMIZER_POLICY"),
                     (dict(OPTIMIZER="SGD"), "OPTIMIZER"), (dict(END_DISCOUNT=0.85), "END_DISCOUNT"),
                     (dict(DROPOUT=0.2), "DROPOUT"), (dict(GRADIENT_CLIP=0.5), "GRADIENT_CLIP"),
                     (dict(GRADIENT_CLIP_NORM=1), "GRADIENT_CLIP_NORM")):
        with pytest.raises(ValueError, match=word):
            net.actrain_params(kw)


def test_critic_spec_reads_the_reference_defaults():
    assert net.critic_spec(None, n_in=854) == net.NetSpec(854, (100, 100, 1), "relu", "linear")
    assert net.critic_spec(dict(CACLA_CRITIC_LAYERS=(50, 0, 20), ACTIVATION_FUNC_HIDDEN="linear")) == \
        net.NetSpec(None, (50, 20, 1), "linear", "linear")
    with pytest.raises(ValueError, match="elu"):
        net.critic_spec(dict(ACTIVATION_FUNC_HIDDEN="elu"))
    with pytest.raises(ValueError, match="hidden layers"):
        net.critic_spec(dict(CACLA_CRITIC_LAYERS=(4, 4, 4, 4, 4)))
