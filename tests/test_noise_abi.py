"""The exploration noise's and the replay memory's fifth field's C-ABI (include/aigar.h,
aigar_noise*, aigar_env_step_ac, aigar_exp_extra_*, aigar_selftest_log): declared, laid out
as the ctypes mirror has it, exported, and refused loudly without a handle that has a
config.  CPU only (the refusals on a live handle -- no config, a tiled handle, a memory
without the flag -- are in tests/test_gpu_noise.py and tests/test_gpu_env_ac.py, as the
action selection's are in tests/test_gpu_decide.py: a handle needs a device)."""
import ctypes as C
import os
import re
import subprocess

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")
CALLS = ("aigar_noise_config", "aigar_noise", "aigar_env_step_ac", "aigar_exp_extra_get", "aigar_exp_extra_set",
         "aigar_selftest_log")


def test_header_declares_the_noise_calls():
    txt = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(aigar_\w+)\s*\(", txt, re.M))
    for need in CALLS:
        assert need in names, need
    assert re.search(r"typedef struct aigar_noise_params \{", txt)
    assert re.search(r"#define AIGAR_WARN_NOISE_NONFINITE 0x10\b", txt)
    assert re.search(r"#define AIGAR_WARN_NOISE_EXHAUSTED 0x20\b", txt)
    assert re.search(r"#define AIGAR_EXP_EXTRA\s+0x2\b", txt)
    assert re.search(r"#define AIGAR_ABI_VERSION 7\b", txt)  # additions only


def test_noise_params_layout_and_constants_match_header(tmp_path):
    fields = ("type", "mu_dtype", "store_raw", "theta", "ou_mu", "dt", "seed")
    src = '#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(aigar_noise_params));\n' % HEADER
    for f in fields:
        src += 'printf(" %%zu", offsetof(aigar_noise_params, %s));\n' % f
    src += 'printf(" %d %d %d %d %d %d\\n", AIGAR_NOISE_GAUSSIAN, AIGAR_NOISE_ORN_UHL, AIGAR_WARN_NOISE_NONFINITE, ' \
           'AIGAR_WARN_NOISE_EXHAUSTED, AIGAR_EXP_EXTRA, AIGAR_ABI_VERSION);return 0;}'
    exe = str(tmp_path / "noise_hdr_check")
    subprocess.run(["gcc", "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[0] == C.sizeof(_abi.NoiseParams) == 48
    for f, off in zip(fields, v[1:8]):
        assert off == getattr(_abi.NoiseParams, f).offset, f
    assert v[8:] == [_abi.NOISE_GAUSSIAN, _abi.NOISE_ORN_UHL, _abi.WARN_NOISE_NONFINITE, _abi.WARN_NOISE_EXHAUSTED,
                     _abi.EXP_EXTRA, _abi.ABI_VERSION]
    assert _abi.NOISE_TYPES == {"Gaussian": 0, "Orn-Uhl": 1} and _abi.NOISE_MAX_T == 16
    # the device's copy of the warn bits, the stream word of the own draws, the attempt bound
    dev = open(os.path.join(ROOT, "aigar_amd", "csrc", "aigar_dev.h")).read()
    assert re.search(r"WARN_NOISE_NONFINITE = 16\b", dev) and re.search(r"WARN_NOISE_EXHAUSTED = 32\b", dev)
    sem = open(os.path.join(ROOT, "aigar_amd", "csrc", "aigar_sem.h")).read()
    assert re.search(r"ST_NOISE = 11\b", sem)
    inc = open(os.path.join(ROOT, "aigar_amd", "csrc", "noise.inc")).read()
    assert re.search(r"kNoiseMaxT = 16\b", inc) and re.search(r"kNoiseOwnT = 16\b", inc)
    import noise_model
    assert (noise_model.ST_NOISE, noise_model.MAX_T, noise_model.OWN_T) == (11, 16, 16)


def test_library_exports_the_noise_calls_and_refuses_a_missing_handle():
    L = _lib.load()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.SO_PATH]).decode()
    exported = set(re.findall(r" T (aigar_\w+)", syms))
    assert not [n for n in CALLS if n not in exported]
    assert L.aigar_abi_version() == 7
    for n in CALLS:
        assert getattr(L, n).argtypes is not None
    # nothing to perturb with: error returns, with a message
    prm = _abi.RewardParams.from_parameters(None)
    assert L.aigar_noise_config(None, None) < 0
    assert L.aigar_noise(None, None, 1, None, None, 0, None, None, None) < 0
    assert L.aigar_last_error()
    assert L.aigar_env_step_ac(None, None, None, None, 0, 0, 0, C.byref(prm), None, None, 0, None) < 0
    assert L.aigar_exp_extra_get(None, None, 1, None, None) < 0
    assert L.aigar_exp_extra_set(None, None, None, 1) < 0
    assert L.aigar_selftest_log(None, None, 0) < 0


def test_stepper_and_env_have_the_python_surface():
    import inspect

    from aigar_amd.env import AgarVecEnv
    for m in ("noise_config", "noise", "env_step_ac", "exp_extra_get", "exp_extra_set", "selftest_log"):
        assert callable(getattr(_lib.Stepper, m))
    for m in ("step_ac", "step_ac_calls", "set_noise", "perturb", "sample_extra", "update_actions"):
        assert callable(getattr(AgarVecEnv, m))
    assert inspect.signature(AgarVecEnv.__init__).parameters["continuous"].default is None  # off unless asked for
    assert inspect.signature(_lib.Stepper.exp_config).parameters["extra"].default is False
