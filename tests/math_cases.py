"""Input families for the device's math and per-entity helpers, in numpy, from fixed seeds.

The pow / trig / mod / trunc-div families restate those of tools/gen/check_pow.cpp,
check_decide_pow.cpp, check_glibc_trig.cpp, check_mod.cpp and check_trunc_div.cpp: every
deterministic sweep in full, the random parts cut to a few thousand elements per branch, so
that a GPU test compares at most about 5 * 10^5 elements.  The helper families follow the
operands the stepper feeds aigar_sem.h.  tests/test_math_cases.py asserts that every family
holds what it aims at; tests/test_gpu_sem.py and tests/test_gpu_math_families.py run them on
the device against Python's own operators.

Every function returns float64 columns (Philox: uint64) and is cached: the arrays are shared
and must not be written to.
"""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 2.718281828459045  # math.e
# s_sin.c's range bounds and the two angles check_glibc_trig.cpp adds to them
SIN_BOUNDS = (2.0 ** -27, 2.0 ** -26, 0.126, 0.855469, 2.426265, 3.14159, 6.2831853, 105414350.0)
# ... and the bounds as __sin / __cos test them, on the high word alone (2^-27, 2^-26, 0.855469, 2.426265 and
# 105414350 cut to 32 bits: up to 2^-21 below the decimal constants, so +-300 ulps of those do not straddle them)
SIN_WORD_BOUNDS = (0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb)
SPECIALS = (0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan, 2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1022,
            float.fromhex("0x1.fffffffffffffp+1023"), -float.fromhex("0x1.fffffffffffffp+1023"), 1e-300, 1e300, 3.0,
            -7.5)


def _frozen(*cols):
    out = []
    for c in cols:
        c = np.ascontiguousarray(c)
        c.setflags(write=False)
        out.append(c)
    return tuple(out) if len(out) > 1 else out[0]


def cached(fn):
    return functools.lru_cache(maxsize=None)(fn)


def step(x, k):
    """x moved by k doubles away from zero (k < 0: towards zero; x != 0 and no zero crossing)."""
    x = np.asarray(x, np.float64)
    return (x.view(np.int64) + np.int64(k)).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(name, got, want, *operands):
    """Bit for bit; the message shows the first five differing operands and both results in hex."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    if len(bad):
        rows = ["(%s): device %s, reference %s" % (", ".join(float(o[i]).hex() for o in operands),
                                                    float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
        raise AssertionError("%s: %d of %d elements differ\n  %s" % (name, len(bad), len(got), "\n  ".join(rows)))


def fl(values):
    return np.array(values, dtype=np.float64)


def kat():
    return np.load(os.path.join(GOLDEN, "kat_numeric.npz"))


# --------------------------------------------------------------------------- pow
POW_YS = (0.475, -0.35, 0.32)


def _path_y(rng, n):
    """check_pow.cpp's exponents: the path's three, and a random one in [-2, 2), in turn."""
    y = np.resize(np.array(POW_YS + (0.0,)), n)
    rnd = (rng.random(n) - 0.5) * 4.0
    return np.where(y == 0.0, rnd, y)


@cached
def pow_path(n=20000):
    """check_pow.cpp's six kinds, n of each: masses, radii, near 1, 2^+-40, cell counts, dense [1, 2)."""
    rng = np.random.default_rng(42)
    xs = [10.0 * 2250.0 ** rng.random(n),
          np.sqrt(10.0 * 2250.0 ** rng.random(n) / math.pi),
          1.0 + (rng.random(n) - 0.5) * 1e-3,
          np.ldexp(0.5 + rng.random(n), (rng.random(n) * 80).astype(np.int64) - 40),
          (1 + (rng.random(n) * 16).astype(np.int64)).astype(np.float64),
          1.0 + rng.integers(0, 2 ** 24, n).astype(np.float64) * 2.0 ** -24]
    x = np.concatenate(xs)
    return _frozen(x, _path_y(rng, len(x)))


@cached
def pow_edges(n=4000):
    """What check_pow.cpp leaves out of the header's domain (x >= 0 finite, 2^-65 <= |y| < 2^63):
    subnormal x, x == 0, x == 1, x a few ulps from 1, the ends of the y range."""
    rng = np.random.default_rng(43)
    sub = np.concatenate([np.ldexp(0.5 + rng.random(n), rng.integers(-1073, -1022, n)),
                          [2.0 ** -1074, 2.0 ** -1073, step(2.0 ** -1022, -1), 2.0 ** -1022]])
    zero = np.zeros(64)
    one = np.ones(64)
    near1 = np.concatenate([step(np.ones(n // 2), rng.integers(1, 400, n // 2)),
                            step(np.ones(n // 2), -rng.integers(1, 400, n // 2))])
    x = np.concatenate([sub, zero, one, near1])
    y = _path_y(rng, len(x))
    y[len(sub):len(sub) + 64] = np.concatenate([POW_YS, -np.array(POW_YS), rng.uniform(-2, 2, 58)])
    # the ends of the y range: tiny |y| on the path's x, large |y| on x next to 1 (finite results,
    # overflow and underflow)
    ny = n // 2
    x_t = 10.0 * 2250.0 ** rng.random(ny)
    y_t = np.ldexp(1.0 + rng.random(ny), rng.integers(-65, -55, ny)) * rng.choice([-1.0, 1.0], ny)
    x_l = step(np.ones(ny), rng.integers(-300, 300, ny) * 2 + 1)
    y_l = np.ldexp(1.0 + rng.random(ny), rng.integers(40, 63, ny)) * rng.choice([-1.0, 1.0], ny)
    return _frozen(np.concatenate([x, x_t, x_l]), np.concatenate([y, y_t, y_l]))


@cached
def pow_decide(n_wide=40000, n_sub=20000):
    """check_decide_pow.cpp: pow(e, y) for y spread over [-760, 0] and inside [-746, -708]
    (subnormal results, glibc's special-case re-rounding, the flush to zero)."""
    rng = np.random.default_rng(7)
    i = np.arange(n_wide)
    wide = np.where(i % 2 == 1, -760.0 * rng.random(n_wide), -760.0 * i / n_wide)
    j = np.arange(n_sub)
    sub = np.where(j % 2 == 1, -746.0 + 38.0 * rng.random(n_sub), -746.0 + 38.0 * j / n_sub)
    y = np.concatenate([wide, sub])
    return _frozen(np.full(len(y), E), y)


def py_pow(x, y):
    """math.pow as the C library's pow returns it: CPython raises on the library's range and pole
    errors (an overflow; a zero to a negative power), where pow itself returns an infinity."""
    try:
        return math.pow(x, y)
    except OverflowError:
        return math.inf
    except ValueError:
        if x == 0.0 and y < 0:
            return math.inf
        raise


# --------------------------------------------------------------------------- trig
ATAN2_KINDS = ("field", "tiny", "mixed", "grid", "cij", "diag", "expdiff", "huge", "rescaled", "sixteenth",
               "cij_switch")


def _signs(rng, n):
    return rng.choice([-1.0, 1.0], n)


@cached
def atan2_kind(kind, n=10000):
    """(y, x) of one of check_glibc_trig.cpp's kinds (and three more aimed at single seams)."""
    rng = np.random.default_rng(100 + ATAN2_KINDS.index(kind))
    u = rng.random
    if kind == "field":  # cell -> command point differences (field-sized)
        x, y = (u(n) - 0.5) * 9600.0, (u(n) - 0.5) * 9600.0
    elif kind == "tiny":  # command point next to the centre
        x, y = (u(n) - 0.5) * 1e-3, (u(n) - 0.5) * 1e-3
    elif kind == "mixed":
        x = np.ldexp(u(n) - 0.5, (u(n) * 60).astype(np.int64) - 30)
        y = np.ldexp(u(n) - 0.5, (u(n) * 60).astype(np.int64) - 30)
    elif kind == "grid":  # one axis zero or an integer grid point
        x = np.floor((u(n) - 0.5) * 200.0)
        y = np.where(np.arange(n) % 2 == 1, 0.0, np.floor((u(n) - 0.5) * 200.0))
    elif kind in ("cij", "cij_switch", "sixteenth"):
        # |y| / |x| next to the cij rows' centres (i + 16) / 256 (u - cij[i][0] ~ 0: the EADD select),
        # next to where the row changes, (i + 16.5) / 256, and next to the 1/16 Taylor / table switch
        i = (u(n) * 241).astype(np.int64)
        if kind == "cij":
            c = (16 + i) / 256.0
        elif kind == "cij_switch":
            c = (16.5 + np.minimum(i, 239)) / 256.0
        else:
            c = np.full(n, 1.0 / 16)
        r = c * (1.0 + (u(n) - 0.5) * 1e-12)
        x = (u(n) + 0.1) * 1000.0 * _signs(rng, n)
        y = x * r * _signs(rng, n)
        swap = u(n) < 0.5
        x, y = np.where(swap, y, x), np.where(swap, x, y)
    elif kind == "diag":  # |y| ~ |x|
        x = (u(n) + 0.01) * 500.0 * _signs(rng, n)
        y = x * (1.0 + (u(n) - 0.5) * 1e-9) * _signs(rng, n)
    elif kind == "expdiff":  # exponent differences near the 57 * 16^5 cut-offs
        x = np.ldexp(1.0 + u(n), (u(n) * 140).astype(np.int64) - 70) * _signs(rng, n)
        y = np.ldexp(1.0 + u(n), (u(n) * 140).astype(np.int64) - 70) * _signs(rng, n)
    elif kind == "huge":  # huge / tiny operands
        x = np.ldexp(u(n) - 0.5, (u(n) * 2000).astype(np.int64) - 1000)
        y = np.ldexp(u(n) - 0.5, (u(n) * 2000).astype(np.int64) - 1000)
    elif kind == "rescaled":  # both operands past 2^+-500, exponents close: the rescaled regular path
        base = rng.integers(505, 1000, n) * rng.choice([-1, 1], n)
        x = np.ldexp(u(n) - 0.5, base + rng.integers(-8, 9, n))
        y = np.ldexp(u(n) - 0.5, base + rng.integers(-8, 9, n))
    else:
        raise KeyError(kind)
    return _frozen(y, x)


@cached
def atan2_specials():
    s = np.array(SPECIALS)
    return _frozen(np.repeat(s, len(s)), np.tile(s, len(s)))


@cached
def atan2_all():
    ys, xs = zip(*([atan2_specials()] + [atan2_kind(k) for k in ATAN2_KINDS]))
    return _frozen(np.concatenate(ys), np.concatenate(xs))


@cached
def atan2_reference():
    y, x = atan2_all()
    return _frozen(np.array([math.atan2(b, a) for b, a in zip(y.tolist(), x.tolist())]))


@cached
def sincos_bounds():
    """Each s_sin.c range bound b, b + k * 2^-52 b for |k| <= 300, both signs; and the same 300 doubles
    on each side of where the code's high-word comparisons actually switch."""
    k = np.arange(-300, 301)
    a = np.concatenate([b + k * math.ldexp(b, -52) for b in SIN_BOUNDS])
    w = np.concatenate([(np.int64(h << 32) + k).view(np.float64) for h in SIN_WORD_BOUNDS])  # the tests' own bounds
    a = np.concatenate([a, w])
    return _frozen(np.concatenate([a, -a]))


@cached
def sincos_table_seams():
    """k / 128 + e 2^-53 (the sincostab rows' centres, where xr ~ 0) and (k + 0.5) / 128 + e 2^-53
    (where the row changes), k < 110, |e| <= 64."""
    k = np.repeat(np.arange(110), 129)
    e = np.tile(np.arange(-64, 65), 110)
    return _frozen(np.concatenate([k / 128.0 + e * 2.0 ** -53, (k + 0.5) / 128.0 + e * 2.0 ** -53]))


@cached
def sincos_angles(n=30000):
    """Every angle family of check_glibc_trig.cpp: the bounds, the table seams, integer degrees
    (numpy.deg2rad(randint(0, 360)), field.py:363), what atan2 returns, wider angles, specials."""
    rng = np.random.default_rng(200)
    ref = atan2_reference()
    return _frozen(np.concatenate([sincos_bounds(), sincos_table_seams(), np.arange(360) * (math.pi / 180.0),
                                   kat()["deg2rad"], ref, (rng.random(n) - 0.5) * 16.0, rng.uniform(-0.9, 0.9, n),
                                   np.array(SPECIALS)]))


def py_sin(v):
    try:
        return math.sin(v)
    except ValueError:  # an infinity: the C library returns NaN
        return math.nan


def py_cos(v):
    try:
        return math.cos(v)
    except ValueError:
        return math.nan


SIN_DOMAIN_END = float.fromhex("0x1.921fbp+26")  # high word 0x419921fb: where __sin / __cos turn to __branred


def in_sin_domain(a):
    """aigar_glibc_trig.h's sin / cos domain: |x| below the __branred range (105414350 on the high
    word), and the infinities and NaNs.  The finite angles beyond -- which no angle of the stepper
    reaches -- go to aigar_trig.h and from there to the platform's own sin / cos, which nothing pins."""
    a = np.asarray(a)
    return ~(np.isfinite(a) & (np.abs(a) >= SIN_DOMAIN_END))


def sin_range(a):
    """Which s_sin.c range each angle takes, by the high word as __sin does: 0 |x| < 2^-26,
    1 < 0.855469, 2 < 2.426265, 3 < 105414350, 4 beyond (finite), 5 inf / NaN."""
    k = ((np.asarray(a).view(np.uint64) >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
    return np.searchsorted(np.array([0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb, 0x7ff00000]), k, side="right")


def atan2_branch(y, x):
    """e_atan2.c's branch of every (y, x), as a string array: 'nan', 'y0', 'x0', 'xinf', 'yinf'
    (the special operands, in the source's order), 'de_hi' / 'de_lo+' / 'de_lo-' (the exponent
    cut-offs), else quadrant form 'i'..'iv' + 'T' (Taylor, u < 1/16) or 'B' (table)."""
    y, x = np.asarray(y), np.asarray(x)
    out = np.empty(len(x), dtype="U8")
    hx = (x.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7ff
    hy = (y.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7ff
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        yx = ay < ax
        u = np.where(yx, ay / ax, ax / ay)
    form = np.where(x > 0, np.where(yx, "i", "ii"), np.where(ax < ay, "iii", "iv"))
    out[:] = np.char.add(form, np.where(u < 1.0 / 16, "T", "B"))
    de = hy - hx
    out[(de <= -57) & (x > 0)] = "de_lo+"
    out[(de <= -57) & ~(x > 0)] = "de_lo-"
    out[de >= 57] = "de_hi"
    out[np.isinf(y)] = "yinf"
    out[np.isinf(x)] = "xinf"
    out[x == 0] = "x0"
    out[y == 0] = "y0"
    out[np.isnan(x) | np.isnan(y)] = "nan"
    return out


def atan2_rescaled(y, x):
    """+1 where e_atan2.c scales the operands up by 2^500 on the regular path, -1 where down, else 0."""
    b = atan2_branch(y, x)
    reg = np.char.startswith(b, "i")
    ax, ay = np.abs(x), np.abs(y)
    up = reg & ((ax < 2.0 ** -500) | (ay < 2.0 ** -500))
    down = reg & ~up & ((ax > 2.0 ** 500) | (ay > 2.0 ** 500))
    return up.astype(np.int64) - down.astype(np.int64)


# --------------------------------------------------------------------------- mod_pos, trunc_div_pos
@cached
def mod_pos_cases(n=20000):
    """check_mod.cpp: random a, exact multiples of b and their neighbours, the axis-mask loop's
    values; b the bucket size and random grid-square sizes.  a >= 0, b > 0 throughout."""
    rng = np.random.default_rng(12345)
    b = np.where(np.arange(n) % 2 == 1, 20.0, rng.uniform(0.05, 400.0, n))
    a = rng.uniform(0.0, 6000.0, n)
    m = np.floor(rng.random(n) * 300) * b
    x = a - np.array([p % q for p, q in zip(a.tolist(), b.tolist())])
    cols = [a, m, np.nextafter(m, 0.0), np.nextafter(m, 1e9), np.nextafter(np.nextafter(m, 1e9), 1e9), x, x + b,
            np.maximum(0.0, a - 0.5 * b)]
    aa = np.concatenate(cols + [[0.0]])
    bb = np.concatenate([b] * len(cols) + [[20.0]])
    keep = (aa >= 0) & (bb > 0)
    return _frozen(aa[keep], bb[keep])


@cached
def trunc_div_mask_loops(n=6000):
    """check_trunc_div.cpp's random part: the observation's mask loops (x runs from a multiple of
    the square size by repeated addition) and the nine doubles around a random k * b."""
    rng = np.random.default_rng(11)
    u = rng.random
    it = np.arange(n)
    fs = (0.5 + u(n) * 60.0) ** 0.475 * (1 + (u(n) * 16).astype(np.int64)) ** 0.32 * 35
    G = np.where(it % 8 == 0, 3 + (u(n) * 60).astype(np.int64), 11)
    gs = fs / G
    r = np.where(it % 2 == 1, np.sqrt((1 + (u(n) * 3).astype(np.int64)) / math.pi), u(n) * fs * 0.3)
    p = -r + u(n) * (fs + 2 * r)
    cl = np.maximum(0.0, p - r)
    bl = cl - np.array([a % b for a, b in zip(cl.tolist(), gs.tolist())])
    lx = np.minimum(fs - 1, p + r)
    xs, bs = [], []
    x = bl.copy()
    live = x <= lx
    while live.any():
        xs.append(x[live])
        bs.append(gs[live])
        x = x + gs
        live &= x <= lx
    xk = (u(n) * 140).astype(np.int64) * gs
    lo = xk.copy()
    for _ in range(4):
        lo = np.nextafter(lo, 0.0)
    for _ in range(9):
        ok = lo >= 0
        xs.append(lo[ok])
        bs.append(gs[ok])
        lo = np.nextafter(lo, 1e300)
    return _frozen(np.concatenate(xs), np.concatenate(bs))


def _around_multiples(b, k):
    """The seven doubles from three below k * b to three above, for every pair (x >= 0 kept)."""
    x = k * b
    for _ in range(3):
        x = np.nextafter(x, 0.0)
    xs, bs = [], []
    for _ in range(7):
        ok = x >= 0
        xs.append(x[ok])
        bs.append(b[ok])
        x = np.nextafter(x, 1e300)
    return np.concatenate(xs), np.concatenate(bs)


@cached
def trunc_div_pow2():
    """check_trunc_div.cpp: b = 2^e for |e| <= 8, the seven doubles around every k * b, 0 < k < 4096
    (exact quotients: x / b sits on an integer and on the doubles next to it)."""
    b = np.repeat(np.ldexp(1.0, np.arange(-8, 9)), 4095)
    k = np.tile(np.arange(1, 4096, dtype=np.float64), 17)
    return _frozen(*_around_multiples(b, k))


@cached
def trunc_div_decimal():
    """check_trunc_div.cpp: b = bi * 0.1 + 0.013 for 0 < bi < 200, the seven doubles around every
    k * b, k < 200."""
    b = np.repeat(np.arange(1, 200) * 0.1 + 0.013, 200)
    k = np.tile(np.arange(200, dtype=np.float64), 199)
    return _frozen(*_around_multiples(b, k))


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker; a below 2^26 in magnitude and an integer, so a * b's halves are exact)."""
    p = a * b
    c = 134217729.0 * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((a * bh - p) + a * bl)


def trunc_div_residual(x, b):
    """What trunc_div_pos tests, per operand pair: n = rint(x * (1 / b)), the correctly rounded
    residual d = fma(-n, b, x) and the threshold t = b * (n - pred(n)) / 2, in plain numpy
    (n >= 1 rows only; the others return before the test).  Returns (n, d, t, rows)."""
    x, b = np.asarray(x), np.asarray(b)
    n = np.rint(x * (1.0 / b))
    rows = n > 0
    x, b, n = x[rows], b[rows], n[rows]
    assert n.max() < 2.0 ** 26
    t = (n - step(n, -1)) * 0.5 * b
    p, e = _two_prod(n, b)
    d = (x - p) - e  # x - p is exact (p / 2 <= x <= 2 p), so this rounds x - n b once
    return n, d, t, rows


# --------------------------------------------------------------------------- the helpers of aigar_sem.h
def is_round3_tie(v):
    """1000 v is exactly half an integer: 2000 v is an odd integer, i.e. v is an odd multiple of 1/16."""
    w = np.asarray(v) * 16.0  # exact
    return np.isfinite(w) & (np.abs(w) < 2.0 ** 52) & (w == np.floor(w)) & (np.mod(w, 2.0) == 1.0)


@cached
def round3_cases(n=20000):
    rng = np.random.default_rng(300)
    k = np.arange(-2000, 2001, dtype=np.float64)
    grid = np.concatenate([k / 1000.0, (k + 0.5) / 1000.0])
    grid = grid[grid != 0]
    near = np.concatenate([step(grid, d) for d in range(-3, 4)])
    odd = np.arange(1, 4002, 2, dtype=np.float64) / 16.0  # the exact ties: 1000 v = 62.5 j, j odd
    v = np.concatenate([near, rng.uniform(-1, 1, n), rng.uniform(-1e-3, 1e-3, n), rng.uniform(-1e6, 1e6, n),
                        [0.0, -0.0, 0.0004, -0.0004, 0.0005, -0.0005, 0.0625, 0.125, 0.5, -0.0625, -0.125, -0.5],
                        step(np.array([0.0004, -0.0004, 0.0005, -0.0005]), 1),
                        step(np.array([0.0004, -0.0004, 0.0005, -0.0005]), -1),
                        odd, -odd, kat()["round_in"]])
    return _frozen(v)


@cached
def py_mod_cases(n=8000):
    rng = np.random.default_rng(301)
    bs = (20.0, -20.0, 7.3, 1e-3, 2.0)
    mult = np.arange(-250, 251) * 20.0
    a = np.concatenate([rng.uniform(-5000, 5000, n), mult, np.nextafter(mult, -1e9), np.nextafter(mult, 1e9),
                        rng.uniform(-1, 1, n // 8) * 1e-300, [0.0, -0.0]])
    return _frozen(np.tile(a, len(bs)), np.repeat(np.array(bs), len(a)))


@cached
def bucket_cases(n=40000):
    """(c, cols): uniform [0, 10000), every 20 k for k < 520 with its two neighbours, and the
    negatives of all of these (bucket_floor_s); cols cycles through grids the clamp does and does
    not cut."""
    rng = np.random.default_rng(302)
    edges = np.arange(520) * 20.0
    pos = np.concatenate([rng.uniform(0, 10000, n), edges, np.nextafter(edges, -1.0), np.nextafter(edges, 1e9)])
    c = np.concatenate([pos, -pos])
    cols = np.resize(np.array([1.0, 22.0, 50.0, 212.0, 500.0, 521.0]), len(c))
    return _frozen(c, cols)


@cached
def sum_cases(rows=1500):
    """(terms [16, n], count [n]): every count 0..16, terms uniform(0, 22500) scaled by 1, 1e-8 or
    1e8 per term; and kat_numeric.npz's segments of at most 16 terms."""
    rng = np.random.default_rng(303)
    cnt = np.repeat(np.arange(17), rows)
    t = rng.uniform(0, 22500, (16, len(cnt))) * rng.choice([1.0, 1e-8, 1e8], (16, len(cnt)))
    t[:, ::3] = rng.uniform(0, 22500, (16, len(cnt[::3])))  # a third of the rows: masses as they are
    z = kat()
    off = z["sum_off"]
    seg = [(off[i], off[i + 1]) for i in range(len(off) - 1) if off[i + 1] - off[i] <= 16]
    kt = np.zeros((16, len(seg)))
    for j, (a, b) in enumerate(seg):
        kt[:b - a, j] = z["sum_in"][a:b]
    kc = np.array([b - a for a, b in seg])
    return _frozen(np.concatenate([t, kt], axis=1), np.concatenate([cnt, kc]).astype(np.float64))


@cached
def radius_cases(n=40000):
    rng = np.random.default_rng(304)
    m = np.concatenate([22500.0 * (1.0 - rng.random(n)), [0.0, 1.0, 2.0, 3.0, -1.0, -0.0, 22500.0],
                        step(np.array([1.0, 2.0, 3.0]), 1), step(np.array([1.0, 2.0, 3.0]), -1),
                        np.arange(1, 200, dtype=np.float64)])
    return _frozen(m)


@cached
def footprint_cases(n=30000):
    """(px, py, rad, size): cells and pellets over fields of three sizes, some past the field's
    edge, and left / top edges px - rad put on and next to every bucket boundary."""
    rng = np.random.default_rng(305)
    size = rng.choice([424.0, 1000.0, 10000.0], n)
    rad = np.sqrt(np.where(rng.random(n) < 0.3, rng.integers(1, 4, n), 10.0 * 2250.0 ** rng.random(n)) / math.pi)
    px = rng.uniform(-0.05, 1.05, n) * size
    py = rng.uniform(-0.05, 1.05, n) * size
    ne = 520
    edge = np.arange(ne) * 20.0
    er = np.sqrt(rng.integers(1, 4, ne) / math.pi)
    ex = np.concatenate([edge + er, np.nextafter(edge + er, 0.0), np.nextafter(edge + er, 1e9),
                         edge - er - 1, np.nextafter(edge - er - 1, 1e9)])
    ey = rng.uniform(0, 10000, len(ex))
    flip = np.arange(len(ex)) % 2 == 1
    px = np.concatenate([px, np.where(flip, ey, ex)])
    py = np.concatenate([py, np.where(flip, ex, ey)])
    rad = np.concatenate([rad, np.tile(er, 5)])
    size = np.concatenate([size, np.full(len(ex), 10000.0)])
    return _frozen(px, py, rad, size)


def _offsets(rng, n, size):
    """Command points of every shape relative to cells at (x, y): field-sized, tiny and zero
    offsets, and points outside the field."""
    x, y = rng.uniform(0, size, n), rng.uniform(0, size, n)
    kind = np.arange(n) % 5
    dx = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                   [rng.uniform(-size, size, n), rng.uniform(-1e-3, 1e-3, n), np.zeros(n), rng.uniform(-3, 3, n)],
                   rng.uniform(-2 * size, 2 * size, n))
    dy = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                   [rng.uniform(-size, size, n), rng.uniform(-1e-3, 1e-3, n),
                    np.where(np.arange(n) % 10 == 2, 0.0, rng.uniform(-50, 50, n)), rng.uniform(-3, 3, n)],
                   rng.uniform(-2 * size, 2 * size, n))
    return x, y, x + dx, y + dy


@cached
def move_cases(n=30000):
    """(x, y, m, r, cpx, cpy): masses 10 to 22500 with their radii; command points far away, a few
    units or less from the centre (inside the radius: the hyp < r2 division), on it, and outside
    the field."""
    rng = np.random.default_rng(306)
    size = 4800.0
    x, y, cpx, cpy = _offsets(rng, n, size)
    m = 10.0 * 2250.0 ** rng.random(n)
    m[::50] = 22500.0
    m[1::50] = 10.0
    r = np.sqrt(m / math.pi)
    inside = np.arange(n) % 5 == 4  # (a fifth of the rest too: points inside the radius, any size)
    ang, frac = rng.uniform(0, 2 * math.pi, n), rng.random(n)
    cpx = np.where(inside, x + frac * r * np.cos(ang), cpx)
    cpy = np.where(inside, y + frac * r * np.sin(ang), cpy)
    return _frozen(x, y, m, r, cpx, cpy)


@cached
def momentum_cases(n=30000):
    """(x, y, cpx, cpy, w, h, orig_r): as move_cases; the command point is clamped to the field."""
    rng = np.random.default_rng(307)
    size = 4800.0
    x, y, cpx, cpy = _offsets(rng, n, size)
    w = np.full(n, size)
    h = np.where(np.arange(n) % 7 == 0, 1000.0, size)
    orig_r = np.sqrt(10.0 * 2250.0 ** rng.random(n) / math.pi)
    return _frozen(x, y, cpx, cpy, w, h, orig_r)


@cached
def merge_time_cases(n=20000):
    rng = np.random.default_rng(308)
    f = rng.choice([1.0, 0.85, 0.5, 2.0], n)
    m = np.concatenate([10.0 * 2250.0 ** rng.random(n - 4), [0.0, 5.0, 10.0, 22500.0]])
    return _frozen(f, m)


@cached
def philox_cases(n=3000):
    """(c0..c3, k0, k1 as uint64; lo, hi as float64): random counters and keys; ranges of every
    width, some empty or reversed (hi <= lo), some with fractions (int() truncates)."""
    rng = np.random.default_rng(309)
    ctr = rng.integers(0, 2 ** 63, (4, n), dtype=np.uint64)
    ctr[:, :8] = 0
    ctr[0, :8] = np.arange(1, 9, dtype=np.uint64)
    ctr[0] = np.maximum(ctr[0], np.uint64(1))  # (c0 >= 1: the test hands numpy the counter before)
    key = rng.integers(0, 2 ** 64, (2, n), dtype=np.uint64)
    lo = np.floor(rng.uniform(-1000, 1000, n))
    width = np.select([np.arange(n) % 4 == 0, np.arange(n) % 4 == 1, np.arange(n) % 4 == 2],
                      [rng.integers(1, 10, n), rng.integers(1, 10 ** 6, n), rng.integers(-50, 1, n)], 360).astype(np.float64)
    hi = lo + width
    frac = np.arange(n) % 9 == 0
    lo = np.where(frac, lo + 0.75, lo)
    hi = np.where(frac, hi + 0.25, hi)
    return _frozen(*ctr, *key, lo, hi)
