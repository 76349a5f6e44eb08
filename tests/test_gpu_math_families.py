"""GPU: the device's pow and trig on every input family of the host checks (tools/gen/check_pow.cpp,
check_decide_pow.cpp, check_glibc_trig.cpp, restated in tests/math_cases.py), against math.pow,
math.atan2, math.sin and math.cos element by element -- the C library's functions, which the
host tests pin to the same headers -- by bit pattern, at tolerance 0, no element skipped.  The
branchy and the wavefront-shaped forms of the trig (atan2_glibc / atan2_glibc_flat, sin_glibc and
cos_glibc / sincos_glibc) must also agree with each other on all of them.  Finite angles from
105414350 on are outside aigar_glibc_trig.h's domain (math_cases.in_sin_domain): the forms are
compared with each other there, not with the C library."""
import numpy as np
import pytest

from aigar_amd import _abi
import math_cases as mc
from math_cases import fl, same

pytestmark = pytest.mark.gpu

_lib = pytest.importorskip("aigar_amd._lib")


def same_or_nan(name, got, want, *operands):
    """Bit for bit, except that a NaN result only has to be a NaN (the sign and payload of one
    are the operation's own business: the C library's differ between its variants too)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN where the reference has none, or none where it has: %s" % (
        name, [tuple(float(o[i]).hex() for o in operands) for i in np.flatnonzero(np.isnan(got) != nan)[:5]])
    same(name, np.where(nan, 0.0, got), np.where(nan, 0.0, want), *operands)


@pytest.mark.parametrize("family", ["pow_path", "pow_edges", "pow_decide"])
def test_device_pow_families_are_glibc_pow(family):
    x, y = getattr(mc, family)()
    got = _lib.selftest_pow(x, y)
    same("pow_glibc", got, fl([mc.py_pow(a, b) for a, b in zip(x.tolist(), y.tolist())]), x, y)


def test_device_atan2_families_are_glibc_atan2():
    y, x = mc.atan2_all()
    ref = mc.atan2_reference()
    at, _, _ = _lib.selftest_trig(y, x)
    same_or_nan("trig_atan2", at, ref, y, x)
    forms = _lib.selftest_sem(_abi.SEM_TRIG_FORMS, y, x)
    same_or_nan("atan2_glibc", forms[0], ref, y, x)
    same_or_nan("atan2_glibc_flat", forms[1], ref, y, x)
    same_or_nan("atan2_glibc_flat vs atan2_glibc", forms[1], forms[0], y, x)


def test_device_sincos_families_are_glibc_sin_and_cos():
    """On the header's domain (math_cases.in_sin_domain: the 600 angles of the sweep past the
    105414350 bound are outside it) every form equals the C library's; on every angle, those
    included, the forms equal each other."""
    a = mc.sincos_angles()
    dom = mc.in_sin_domain(a)
    assert 300 <= (~dom).sum() <= 2000
    ad = a[dom]
    rs, rc = fl([mc.py_sin(v) for v in ad.tolist()]), fl([mc.py_cos(v) for v in ad.tolist()])
    assert np.isnan(rs[~np.isfinite(ad)]).all() and np.isnan(rc[~np.isfinite(ad)]).all()
    _, s, c = _lib.selftest_trig(np.zeros_like(a), a)
    forms = _lib.selftest_sem(_abi.SEM_TRIG_FORMS, np.zeros_like(a), a)
    same_or_nan("trig_sincos sin", s[dom], rs, ad)
    same_or_nan("trig_sincos cos", c[dom], rc, ad)
    same_or_nan("sin_glibc", forms[2][dom], rs, ad)
    same_or_nan("cos_glibc", forms[3][dom], rc, ad)
    same_or_nan("sincos_glibc sin", forms[4][dom], rs, ad)
    same_or_nan("sincos_glibc cos", forms[5][dom], rc, ad)
    same_or_nan("sincos_glibc sin vs sin_glibc", forms[4], forms[2], a)
    same_or_nan("sincos_glibc cos vs cos_glibc", forms[5], forms[3], a)
    same_or_nan("trig_sincos sin vs sincos_glibc", s, forms[4], a)
    same_or_nan("trig_sincos cos vs sincos_glibc", c, forms[5], a)


def test_trig_forms_agree_on_the_atan2_operands_as_angles():
    """TRIG_FORMS takes sin / cos of its x operand: the atan2 families' x -- every special operand,
    2^+-1000, subnormals -- are angles no family of sincos_angles holds."""
    y, x = mc.atan2_all()
    forms = _lib.selftest_sem(_abi.SEM_TRIG_FORMS, y, x)
    same_or_nan("sincos_glibc sin vs sin_glibc", forms[4], forms[2], x)
    same_or_nan("sincos_glibc cos vs cos_glibc", forms[5], forms[3], x)
    dom = mc.in_sin_domain(x)
    xs = x[dom].tolist()
    same_or_nan("sin_glibc", forms[2][dom], fl([mc.py_sin(v) for v in xs]), x[dom])
    same_or_nan("cos_glibc", forms[3][dom], fl([mc.py_cos(v) for v in xs]), x[dom])
