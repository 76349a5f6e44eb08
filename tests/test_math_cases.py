"""The families of tests/math_cases.py hold what they aim at (CPU only, Python's own values for
the counts), so that a later edit cannot hollow out tests/test_gpu_sem.py and
tests/test_gpu_math_families.py: every branch of the device's pow, trig and helpers that those
tests mean to reach has a few hundred inputs here, every special operand is present, and the
Python references reproduce the reference-made known answers of tests/golden/kat_numeric.npz."""
import math

import numpy as np

import math_cases as mc

FEW = 300  # "a few hundred" inputs per branch


def test_families_stay_within_the_gpu_tests_budget():
    sizes = {"pow_path": len(mc.pow_path()[0]), "pow_edges": len(mc.pow_edges()[0]),
             "pow_decide": len(mc.pow_decide()[0]), "atan2_all": len(mc.atan2_all()[0]),
             "sincos_angles": len(mc.sincos_angles()), "mod_pos": len(mc.mod_pos_cases()[0]),
             "trunc_div_mask_loops": len(mc.trunc_div_mask_loops()[0]), "trunc_div_pow2": len(mc.trunc_div_pow2()[0]),
             "trunc_div_decimal": len(mc.trunc_div_decimal()[0]), "round3": len(mc.round3_cases()),
             "py_mod": len(mc.py_mod_cases()[0]), "bucket": len(mc.bucket_cases()[0]), "sum": len(mc.sum_cases()[1]),
             "radius": len(mc.radius_cases()), "footprint": len(mc.footprint_cases()[0]),
             "move": len(mc.move_cases()[0]), "momentum": len(mc.momentum_cases()[0]),
             "merge_time": len(mc.merge_time_cases()[0]), "philox": len(mc.philox_cases()[0])}
    print(sizes)
    assert all(1000 <= n <= 500000 for n in sizes.values()), sizes


def test_sincos_angles_reach_every_range_and_both_sides_of_every_seam():
    a = mc.sincos_angles()
    rng = mc.sin_range(a)
    counts = np.bincount(rng, minlength=6)
    print("s_sin.c ranges (tiny, < 0.855469, < 2.426265, < 105414350, beyond, inf / NaN):", counts.tolist())
    assert (counts[:5] >= FEW).all(), counts
    assert np.isinf(a).sum() >= 2 and np.isnan(a).sum() >= 1  # (the special operands: a short table)
    for s in (0.0, -0.0, 2.0 ** -1074, -2.0 ** -1074, 2.0 ** -1022):
        assert (a.view(np.uint64) == np.float64(s).view(np.uint64)).any(), s
    for b in mc.SIN_BOUNDS:  # 300 ulps on each side of each bound, both signs
        near = np.abs(np.abs(a) - b) <= 301 * math.ldexp(b, -52)
        assert (near & (np.abs(a) < b)).sum() >= 2 * FEW - 2 and (near & (np.abs(a) >= b)).sum() >= 2 * FEW - 2, b
    for h in mc.SIN_WORD_BOUNDS:  # ... and of where the high-word comparisons switch
        b = np.array([h << 32], dtype=np.int64).view(np.float64)[0]
        near = np.abs(np.abs(a) - b) <= 301 * math.ldexp(b, -52)
        assert (near & (np.abs(a) < b)).sum() >= 2 * FEW and (near & (np.abs(a) >= b)).sum() >= 2 * FEW, hex(h)
    # the top of the 2.426265 range (the hp0 - |x| forms, whose table row is the last ones)
    top = (rng == 2) & (np.abs(a) > 2.42)
    assert top.sum() >= FEW, top.sum()
    # the 1/128 grid of __sincostab: the rows' centres and where the row changes, both sides of each
    aa = np.abs(a)
    for k in range(110):
        for c in (k / 128.0, (k + 0.5) / 128.0):
            near = np.abs(aa - c) <= 65 * 2.0 ** -53
            assert (near & (aa < c)).sum() >= (64 if c else 0) and (near & (aa > c)).sum() >= 64, (k, c)
    # the last row of the table (|x| rounds to 109 / 128) and the Taylor / table switch at 0.126
    assert ((aa >= 108.5 / 128) & (aa < 0.855469)).sum() >= FEW
    assert ((aa < 0.126) & (rng == 1)).sum() >= FEW and ((aa >= 0.126) & (rng == 1)).sum() >= FEW
    deg = np.arange(360) * (math.pi / 180.0)
    assert np.isin(deg, a).all() and np.array_equal(deg, mc.kat()["deg2rad"])
    # every quadrant of the reduction (n & 3) in the 105414350 range
    quad = np.rint(a[rng == 3] * (2 / math.pi)).astype(np.int64) & 3
    assert (np.bincount(quad, minlength=4) >= FEW).all()


def test_atan2_operands_reach_every_branch():
    y, x = mc.atan2_all()
    br = mc.atan2_branch(y, x)
    names, counts = np.unique(br, return_counts=True)
    have = dict(zip(names.tolist(), counts.tolist()))
    print("e_atan2.c branches:", have)
    for form in ("i", "ii", "iii", "iv"):  # each quadrant form, Taylor and table
        assert have.get(form + "T", 0) >= FEW and have.get(form + "B", 0) >= FEW, (form, have)
    for cut in ("de_hi", "de_lo+", "de_lo-"):  # the exponent-difference cut-offs
        assert have.get(cut, 0) >= FEW, (cut, have)
    # each side of the cut-offs, next to them
    hx = (x.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7ff
    hy = (y.view(np.uint64) >> np.uint64(52)).astype(np.int64) & 0x7ff
    regular = np.char.startswith(br, "i")
    for d in (56, -56):
        assert (regular & (hy - hx == d)).sum() >= 30, d
    for d, name in ((57, "de_hi"), (-57, "de_lo+"), (-57, "de_lo-")):
        assert ((br == name) & (hy - hx == d)).sum() >= 10, (d, name)
    # every special operand against every special operand, and each special branch
    sy, sx = mc.atan2_specials()
    assert len(sx) == len(mc.SPECIALS) ** 2
    for name in ("nan", "y0", "x0", "xinf", "yinf"):
        assert have.get(name, 0) >= 10, (name, have)
    # the 2^+-500 rescaling, on the regular path
    scaled = mc.atan2_rescaled(y, x)
    assert (scaled == 1).sum() >= FEW and (scaled == -1).sum() >= FEW, np.bincount(scaled + 1)
    # the seams: the ratio u on each side of 1/16, of every cij row's centre and of every row change
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        u = np.where(ay < ax, ay / ax, ax / ay)
    u = np.where(regular, u, -1.0)
    near = np.abs(u - 1.0 / 16) <= 1e-12
    assert (near & (u < 1.0 / 16)).sum() >= FEW and (near & (u >= 1.0 / 16)).sum() >= FEW
    for form in ("i", "ii", "iii", "iv"):  # ... in each quadrant form
        assert (near & (br == form + "T")).sum() >= 50 and (near & (br == form + "B")).sum() >= 50, form
    below = above = sw_below = sw_above = 0
    for i in range(241):
        c = (16 + i) / 256.0
        near = np.abs(u - c) <= 1e-12 * c
        lo, hi = int((near & (u < c)).sum()), int((near & (u >= c)).sum())
        assert lo >= 5 and hi >= 5, (i, lo, hi)
        below, above = below + lo, above + hi
        if i < 240:
            c = (16.5 + i) / 256.0
            near = np.abs(u - c) <= 1e-12 * c
            lo, hi = int((near & (u < c)).sum()), int((near & (u >= c)).sum())
            assert lo >= 5 and hi >= 5, (i, lo, hi)
            sw_below, sw_above = sw_below + lo, sw_above + hi
    assert min(below, above, sw_below, sw_above) >= 10 * FEW
    # |y| ~ |x|: ratios that round to the last row (u * 256 rounds to 256), u == 1 among them
    last = regular & (u >= 255.5 / 256)
    assert last.sum() >= FEW and (u == 1.0).sum() >= 1


def test_pow_families_reach_the_subnormal_results_and_the_flush_to_zero():
    x, y = mc.pow_decide()
    assert (x == mc.E).all() and y.min() >= -760.0 and y.max() <= 0.0
    r = np.array([mc.py_pow(a, b) for a, b in zip(x.tolist(), y.tolist())])
    sub = (r != 0) & (r < 2.0 ** -1022)
    print("pow(e, y): %d subnormal results, %d zeros, %d normal" % (sub.sum(), (r == 0).sum(), (~sub & (r != 0)).sum()))
    assert sub.sum() >= FEW and (r == 0).sum() >= FEW and (~sub & (r != 0)).sum() >= FEW
    # glibc's special case (|y ln x| large, the result not far from the underflow bound) on the normal side too
    assert ((r >= 2.0 ** -1022) & (r < 2.0 ** -1000)).sum() >= FEW
    x, y = mc.pow_path()
    assert ((np.abs(y) <= 2) & (x > 0)).all()
    for name, sel in (("near 1", np.abs(x - 1) < 1e-3), ("above 2^20", x > 2.0 ** 20), ("below 2^-20", x < 2.0 ** -20),
                      ("cell counts", (x == np.floor(x)) & (x <= 16)), ("masses", (x >= 10) & (x <= 22500))):
        assert sel.sum() >= FEW, name
    x, y = mc.pow_edges()
    assert ((x >= 0) & np.isfinite(x) & (np.abs(y) >= 2.0 ** -65) & (np.abs(y) < 2.0 ** 63)).all()  # the header's domain
    r = np.array([mc.py_pow(a, b) for a, b in zip(x.tolist(), y.tolist())])
    sub_x = (x > 0) & (x < 2.0 ** -1022)
    assert sub_x.sum() >= FEW and (x == 2.0 ** -1074).any()
    assert ((x == 0) & (y > 0)).sum() >= 10 and ((x == 0) & (y < 0)).sum() >= 10 and (x == 1).sum() >= 10
    assert np.isinf(r[(x == 0) & (y < 0)]).all() and (r[(x == 0) & (y > 0)] == 0).all()
    assert (np.abs(y) < 2.0 ** -55).sum() >= FEW and (np.abs(y) >= 2.0 ** 40).sum() >= FEW
    big = np.abs(y) >= 2.0 ** 40
    assert (big & np.isinf(r)).sum() >= 50 and (big & (r == 0)).sum() >= 50 and (big & np.isfinite(r) & (r != 0)).sum() >= FEW


def test_mod_pos_families():
    a, b = mc.mod_pos_cases()
    assert ((a >= 0) & (b > 0)).all()
    m = np.array([p % q for p, q in zip(a.tolist(), b.tolist())])
    assert (m == 0).sum() >= FEW  # exact multiples
    q = a / b
    assert ((m > 0) & (m < b * 1e-12)).sum() >= FEW and ((m > 0) & (b - m < b * 1e-12)).sum() >= FEW  # each side of them
    assert (b == 20.0).sum() >= FEW and (b != 20.0).sum() >= FEW and q.max() < 2.0 ** 50


def test_trunc_div_pos_families_sit_on_both_sides_of_the_midpoint():
    """trunc_div_pos returns n = rint(x / b) or n - 1 by comparing the residual d = fl(x - n b) with
    -t, the midpoint between n and its predecessor scaled by b, and divides only where d == -t.
    No pair of doubles gets there: x - n b = -t means x = b (n - ulp / 2), a product of b's
    significand with a 54-bit odd number, which no double holds; and x - n b and t are both whole
    multiples of ulp(t), so a residual that is not -t is at least one ulp(t) away from it and does
    not round to it.  So the families cannot hold such an operand (asserted: none does); what they
    can and do hold is residuals next to the midpoint on either side, where the answer changes."""
    for fam in (mc.trunc_div_mask_loops, mc.trunc_div_pow2, mc.trunc_div_decimal):
        x, b = fam()
        assert ((x >= 0) & (b > 0)).all()
        n, d, t, rows = mc.trunc_div_residual(x, b)
        want = np.array([int(p / q) for p, q in zip(x[rows].tolist(), b[rows].tolist())])
        assert (d == -t).sum() == 0
        hi_side, lo_side = (d > -t), (d < -t)
        assert np.array_equal(want[hi_side], n[hi_side]) and np.array_equal(want[lo_side], n[lo_side] - 1)
        near_hi, near_lo = hi_side & (d <= -t / 4), lo_side & (d >= -4 * t)
        print(fam.__name__, len(x), "near the midpoint: above", near_hi.sum(), "below", near_lo.sum(), "n == 0:", (~rows).sum())
        # (2^e divisors: the quotients are exact, so a residual is 0 or at most -2 t -- below only)
        assert near_lo.sum() >= FEW and (near_hi.sum() >= FEW or fam is mc.trunc_div_pow2)
        assert (d == 0).sum() >= FEW  # x an exact multiple
    x, b = mc.trunc_div_pow2()
    assert sorted(set(np.log2(b).tolist())) == list(range(-8, 9)) and len(x) == 17 * 4095 * 7
    x, b = mc.trunc_div_decimal()
    assert len(set(b.tolist())) == 199


def test_round3_inputs_hold_exact_ties_and_the_shortcut_bound():
    v = mc.round3_cases()
    ties = mc.is_round3_tie(v)
    r = np.array([round(p, 3) for p in v.tolist()])
    k = np.rint(r[ties] * 1000)
    down, up = (np.abs(k) < np.abs(v[ties] * 1000)).sum(), (np.abs(k) > np.abs(v[ties] * 1000)).sum()
    print("round: %d inputs, %d exact ties (%d resolved towards zero, %d away)" % (len(v), ties.sum(), down, up))
    assert ties.sum() >= FEW and down >= FEW // 2 and up >= FEW // 2 and (k % 2 == 0).all()
    for s in (0.0, -0.0, 0.0004, -0.0004, 0.0005, -0.0005, 0.0625, 0.125, 0.5):
        assert (v.view(np.uint64) == np.float64(s).view(np.uint64)).any(), s
    small = np.abs(v) < 0.0004  # the shortcut: a zero with v's sign
    assert small.sum() >= FEW and (r[small] == 0).all() and np.array_equal(np.signbit(r[small]), np.signbit(v[small]))
    assert ((np.abs(v) >= 0.0004) & (np.abs(v) < 0.0005)).sum() >= FEW and (r == 0).sum() > small.sum()
    # next to every k / 1000 and (k + 0.5) / 1000, |k| <= 2000: both roundings occur within 3 ulps
    assert (np.abs(v) > 1000).sum() >= FEW and (v < 0).sum() >= FEW
    z = mc.kat()
    assert np.isin(z["round_in"], v).all()
    got = np.array([round(float(p), 3) for p in z["round_in"]])
    assert np.array_equal(got.view(np.uint64), z["round_out"].view(np.uint64))


def test_sums_hold_every_count_and_numpy_reproduces_the_known_answers():
    terms, cnt = mc.sum_cases()
    assert terms.shape == (16, len(cnt))
    counts = np.bincount(cnt.astype(np.int64), minlength=17)
    print("sums per count:", counts.tolist())
    assert len(counts) == 17 and (counts >= FEW).all()
    spread = terms.max(axis=0) / np.maximum(terms.min(axis=0), 1e-300)
    assert (spread > 1e10).sum() >= FEW and (spread < 1e6).sum() >= FEW  # mixed scales, and masses as they are
    z = mc.kat()
    off = z["sum_off"]
    got = np.array([np.sum(np.ascontiguousarray(z["sum_in"][off[i]:off[i + 1]])) for i in range(len(off) - 1)])
    assert np.array_equal(got.view(np.uint64), z["sum_out"].view(np.uint64))
    short = int((np.diff(off) <= 16).sum())
    assert short >= FEW and len(cnt) == 17 * 1500 + short


def test_helper_families_hold_their_edges():
    a, b = mc.py_mod_cases()
    assert set(b.tolist()) == {20.0, -20.0, 7.3, 1e-3, 2.0}
    m = np.array([p % q for p, q in zip(a.tolist(), b.tolist())])
    assert (m == 0).sum() >= FEW and (a < 0).sum() >= FEW and (np.abs(a) < 1e-299).sum() >= FEW
    assert ((m == 0) & np.signbit(m)).sum() >= 50  # a zero remainder takes b's sign
    c, cols = mc.bucket_cases()
    k = np.arange(520) * 20.0
    for e in (k, np.nextafter(k, -1.0), np.nextafter(k, 1e9)):
        assert np.isin(e, c).all() and np.isin(-e, c).all()
    assert ((c >= 0) & (c < 10000)).sum() >= FEW and (c < 0).sum() >= FEW
    fl = np.array([int(p // 20) for p in c.tolist()])
    assert ((c >= 0) & (fl > cols - 1)).sum() >= FEW and ((c >= 0) & (fl < cols - 1)).sum() >= FEW  # the clamp cuts, and not
    m = mc.radius_cases()
    for s in (0.0, 1.0, 2.0, 3.0, -1.0, 22500.0):
        assert (m == s).any(), s
    assert ((m > 0) & (m <= 22500)).sum() >= FEW and m.max() == 22500.0
    px, py, rad, size = mc.footprint_cases()
    assert ((px - rad < 0) | (py - rad < 0)).sum() >= FEW and ((px + rad + 1 > size) | (py + rad + 1 > size)).sum() >= FEW
    edge = (np.mod(px - rad, 20.0) == 0) | (np.mod(py - rad, 20.0) == 0)
    assert edge.sum() >= FEW  # a left / top edge exactly on a bucket boundary
    x, y, mm, r, cpx, cpy = mc.move_cases()
    hyp = (cpx - x) ** 2 + (cpy - y) ** 2
    assert ((hyp < r * r) & (hyp > 0)).sum() >= FEW and (hyp == 0).sum() >= FEW and (hyp >= r * r).sum() >= FEW
    assert mm.min() == 10.0 and mm.max() == 22500.0 and np.array_equal(r, np.sqrt(mm / math.pi))
    assert ((cpx < 0) | (cpx > 4800) | (cpy < 0) | (cpy > 4800)).sum() >= FEW
    x, y, cpx, cpy, w, h, orig_r = mc.momentum_cases()
    assert ((cpx < 0) | (cpx > w)).sum() >= FEW and ((cpy < 0) | (cpy > h)).sum() >= FEW  # the clamp to the field
    assert ((cpx == x) & (cpy == y)).sum() >= FEW and (np.hypot(cpx - x, cpy - y) < 1e-2).sum() >= FEW
    cols = mc.philox_cases()
    lo, hi = cols[6], cols[7]
    assert (hi <= lo).sum() >= FEW and (hi > lo).sum() >= FEW and (lo != np.floor(lo)).sum() >= FEW
    assert all(c.dtype == np.uint64 for c in cols[:6]) and (cols[0] >= 1).all()
