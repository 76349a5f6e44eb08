"""The pixel-state entry points of the C ABI (aigar_pixel_config, aigar_pixel_state_len,
aigar_observe_pixel_state): declared, bound, and mapped from the reference's parameters.
CPU-only: no device call is reached."""
import ctypes as C
import os
import re

import numpy as np

from aigar_amd import _abi, _lib
from aigar_amd import model as M
from test_facade import reference_like_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")


def test_header_declares_the_pixel_state_and_keeps_abi_7():
    txt = open(HEADER).read()
    assert re.search(r"^#define AIGAR_ABI_VERSION 7\b", txt, re.M)
    assert re.search(r"^#define AIGAR_PIX_RGB\s+0x1\b", txt, re.M)
    assert re.search(r"^#define AIGAR_PIX_LAST\s+0x2\b", txt, re.M)
    assert (_abi.PIX_RGB, _abi.PIX_LAST, _abi.ABI_VERSION) == (0x1, 0x2, 7)
    assert re.search(r"^int aigar_pixel_config\(aigar_handle \*h, const aigar_pixel_params \*p\);", txt, re.M)
    assert re.search(r"^int aigar_pixel_state_len\(aigar_handle \*h\);", txt, re.M)
    assert re.search(r"^int aigar_observe_pixel_state\(aigar_handle \*h, void \*out, int dtype, int on_device, "
                     r"const uint8_t \*mask,\s+int mask_on_device\);", txt, re.M)
    L = _lib.load()
    assert L.aigar_abi_version() == 7
    assert L.aigar_pixel_config.argtypes[1]._type_ is _abi.PixelParams
    assert len(L.aigar_observe_pixel_state.argtypes) == 6 and L.aigar_pixel_state_len.argtypes == [C.c_void_p]


def test_pixel_params_struct_has_the_header_layout():
    txt = open(HEADER).read()
    m = re.search(r"typedef struct aigar_pixel_params \{(.*?)\} aigar_pixel_params;", txt, re.S)
    assert m
    fields = re.findall(r"^\s*(int32_t|uint64_t)\s+(\w+);", m.group(1), re.M)
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(_abi.PixelParams._fields_)
    assert C.sizeof(_abi.PixelParams) == 16
    assert [getattr(_abi.PixelParams, n).offset for n, _ in _abi.PixelParams._fields_] == [0, 4, 8]


def _cnn(**kw):
    p = reference_like_parameters(True, True, False, 16)
    p.GRID_VIEW_ENABLED = True
    p.CNN_REPR = p.CNN_P_REPR = True
    p.CNN_USE_L1, p.CNN_USE_L2, p.CNN_USE_L3 = True, False, False
    p.CNN_INPUT_DIM_1, p.CNN_INPUT_DIM_2, p.CNN_INPUT_DIM_3 = 42, 84, 41
    p.CNN_P_RGB = p.CNN_LAST_GRID = False
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_pixel_params_follow_the_reference_parameters():
    assert M.pixel_params(_cnn()) == (42, False, False)
    assert M.pixel_params(_cnn(CNN_USE_L1=False, CNN_USE_L2=True)) == (84, False, False)
    assert M.pixel_params(_cnn(CNN_USE_L1=False, CNN_USE_L3=True)) == (41, False, False)
    assert M.pixel_params(_cnn(CNN_USE_L1=True, CNN_USE_L2=True)) == (42, False, False)  # L1 wins (rgbGenerator.py:16)
    assert M.pixel_params(_cnn(CNN_P_RGB=True)) == (42, True, False)
    assert M.pixel_params(_cnn(CNN_LAST_GRID=True)) == (42, False, True)
    assert M.pixel_params(_cnn(CNN_P_RGB=True, CNN_LAST_GRID=True, CNN_USE_L1=False, CNN_USE_L2=True)) == \
        (84, True, True)
    # every other state: the grid view, the CNN grid view, the simple state, no parameters
    assert M.pixel_params(reference_like_parameters(True, True, False, 16)) is None
    assert M.pixel_params(_cnn(CNN_P_REPR=False)) is None
    assert M.pixel_params(_cnn(CNN_REPR=False)) is None
    assert M.pixel_params(_cnn(GRID_VIEW_ENABLED=False)) is None
    assert M.pixel_params(None) is None
    # and obs_masks is as before for them (the grid view the env still allocates)
    assert M.obs_masks(_cnn(CNN_P_REPR=False))[2] == 42


def test_rgb_state_is_numpy_uint8_wraparound():
    """bot.py:276-282 subtracts 255 from the uint8 frame: numpy wraps, so white is 0.0 and
    black 0.01.  The device computes ((b + 1) & 255) / 100.0."""
    b = np.arange(256, dtype=np.uint8)
    ref = (b - 255) / 100
    assert ref.dtype == np.float64
    want = ((b.astype(np.int64) + 1) & 255) / 100.0
    assert np.array_equal(ref, want)
    assert ref[0] == 0.01 and ref[1] == 0.02 and ref[254] == 2.55 and ref[255] == 0.0
    # the zero state is the white frame in grayscale too
    white = np.full((1, 3), 255, np.uint8)
    gray = np.average(white.astype(np.float64), axis=-1, weights=[0.298, 0.587, 0.114])
    assert ((gray - 255) / 100 == 0.0).all()
