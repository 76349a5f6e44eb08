"""The score entry points of the C ABI (AIGAR_FLAG_SCORE, ABI 7): declared, bound, and
refused on a tiled handle by the config validation (CPU-only: no device call is reached)."""
import ctypes as C
import os
import re

from aigar_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aigar.h")


def test_flag_version_and_declarations():
    assert _abi.FLAG_SCORE == 0x2
    assert _abi.ABI_VERSION == 7
    txt = open(HEADER).read()
    assert re.search(r"^#define AIGAR_FLAG_SCORE 0x2\b", txt, re.M)
    assert re.search(r"^#define AIGAR_ABI_VERSION 7\b", txt, re.M)
    for name in ("aigar_score", "aigar_score_reset", "aigar_score_trace"):
        assert re.search(r"^int %s\(aigar_handle \*h" % name, txt, re.M), name
    L = _lib.load()
    assert L.aigar_abi_version() == 7
    assert L.aigar_score.argtypes[0] is C.c_void_p and L.aigar_score_trace.argtypes[2] is C.c_int64


def test_create_refuses_the_flag_on_a_tiled_handle():
    L = _lib.load()
    cfg = _abi.Config()
    cfg.n_arenas, cfg.bots_per_arena, cfg.rng_mode = 1, 8, _abi.RNG_PHILOX
    cfg.flags, cfg.tile_x, cfg.tile_y = _abi.FLAG_SCORE, 2, 1
    h = C.c_void_p()
    assert L.aigar_create(C.byref(cfg), C.byref(h)) < 0
    assert b"score" in L.aigar_last_error()
    cfg.tile_x, cfg.tile_flags = 1, _abi.TILE_FORCE  # the one-tile tiled handle is a tiled handle
    assert L.aigar_create(C.byref(cfg), C.byref(h)) < 0
    assert b"score" in L.aigar_last_error()
