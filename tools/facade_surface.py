#!/usr/bin/env python3
"""The public surface of the Python facade, as tests/test_facade_surface.py pins it: every public
callable of aigar_amd._lib and aigar_amd.env, of Stepper and of AgarVecEnv with its signature, and
Batch's fields.  Needs no device.

    python tools/facade_surface.py            print the surface as JSON
    python tools/facade_surface.py --write    record it in tests/golden/facade_surface.json

Record it at the commit whose surface is to be kept, before the facade is reworked."""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "facade_surface.json")


def _callables(owner, module):
    """name -> signature of owner's public callables that module defines (classes: by their constructor)."""
    out = {}
    for name, obj in sorted(vars(owner).items()):
        if name.startswith("_"):
            continue
        if isinstance(obj, (staticmethod, classmethod)):
            obj = obj.__func__
        if not callable(obj) or getattr(obj, "__module__", None) != module:
            continue
        out[name] = str(inspect.signature(obj))
    return out


def surface():
    from aigar_amd import _lib, env
    return {"aigar_amd._lib": _callables(_lib, _lib.__name__),
            "aigar_amd._lib.Stepper": _callables(_lib.Stepper, _lib.__name__),
            "aigar_amd.env": _callables(env, env.__name__),
            "aigar_amd.env.AgarVecEnv": _callables(env.AgarVecEnv, env.__name__),
            "aigar_amd.env.Batch._fields": list(env.Batch._fields)}


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    text = json.dumps(surface(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
