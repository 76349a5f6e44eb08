"""Why the parallel playerPlayerOverlap pass took the path it took on each built world of
tests/pp_worlds.py (diagnostics build, -DAIGAR_PP_DIAG): per case, the first tick's
counts of arenas with too few / too many pending players, closures over the player /
cell caps or not settling, fall-backs after the closures, parallel passes, and the
sizes of the settled closures (players 0..7+).  "bad" counts every fall-back after
the closures: a closure that gave up (the three counts before it), a union of merged
closures above the player cap, or two roots that share a player (conflict).
build: bash tools/build_variant.sh tools/var/lib_ppdiag.so -DAIGAR_PP_DIAG"""
import os, sys, ctypes as C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["AIGAR_SO"] = os.path.join(ROOT, "tools", "var", "lib_ppdiag.so")
from aigar_amd import _lib
from oracle_lib import Oracle
import pp_worlds as pw

NAMES = ("nw<min", "nw>max", "ovf_pl", "ovf_cells", "noconv", "bad", "par")


def read(L):
    out = (C.c_ulonglong * 16)()
    L.aigar_debug_ppdiag(out)
    return list(out)


L = _lib.load()
total = [0] * 16
for name in pw.CASES:
    cfg = pw.config(name)
    g, o = _lib.Stepper(cfg), Oracle(cfg)
    cmd = pw.start(name, g, o)
    g.sync()
    v0 = read(L)
    g.set_commands(cmd)
    g.step(1)
    g.sync()
    dv = [b - a for a, b in zip(v0, read(L))]
    total = [t + x for t, x in zip(total, dv)]
    print("%-11s %s | closure players hist %s" % (name, " ".join("%s %d" % (n, x) for n, x in zip(NAMES, dv)), dv[8:16]))
    g.close()
    o.close()
print("%-11s %s | closure players hist %s" % ("all", " ".join("%s %d" % (n, x) for n, x in zip(NAMES, total)), total[8:16]))
