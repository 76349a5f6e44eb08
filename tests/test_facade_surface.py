"""CPU: the public surface of the Python facade stays.  tests/golden/facade_surface.json holds every
public callable of aigar_amd._lib and aigar_amd.env, of Stepper and of AgarVecEnv with
str(inspect.signature(...)), and Batch's fields, as tools/facade_surface.py recorded them; every
recorded entry must still be there with the same signature.  What has been added since passes, so a
new feature does not touch the fixture.  Importing the two modules needs no device."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import facade_surface  # noqa: E402


def test_every_recorded_public_name_is_there_with_its_signature(golden_dir):
    with open(os.path.join(golden_dir, "facade_surface.json")) as f:
        want = json.load(f)
    got = facade_surface.surface()
    assert len(want["aigar_amd._lib.Stepper"]) == 97 and len(want["aigar_amd.env.AgarVecEnv"]) == 32
    assert got["aigar_amd.env.Batch._fields"] == want.pop("aigar_amd.env.Batch._fields")
    differ = ["%s.%s: %s, recorded %s" % (owner, name, got[owner].get(name, "missing"), sig)
              for owner, names in sorted(want.items()) for name, sig in sorted(names.items())
              if got[owner].get(name) != sig]
    assert not differ, "\n".join(differ)
