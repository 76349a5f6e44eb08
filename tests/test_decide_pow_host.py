"""Host check of aigar_math::pow_glibc(e, y) on the Boltzmann selection's exponents
(decide.inc: y = (q_i - max) / temperature <= 0) against the C library's pow, which the
reference's `math.e ** y` calls: bit for bit on 10^6 values of y over [-760, 0], 2 * 10^5
inside [-746, -708] -- where the result is below 2^-1022 and glibc's specialcase re-rounds
it around 1.0 before scaling, restated in aigar_math.h -- and every y the GPU tests'
rows give (tests/decide_cases.py).  CPU only."""
import os
import subprocess

import numpy as np

import decide_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pow_glibc_matches_libm_on_the_boltzmann_exponents(tmp_path):
    exe = str(tmp_path / "check_decide_pow")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "aigar_amd", "csrc"),
                           os.path.join(ROOT, "tools", "gen", "check_decide_pow.cpp"), "-o", exe])
    ys = str(tmp_path / "ys.f64")
    n = n_sub = 0
    with open(ys, "wb") as f:
        for n_out, A, B, dtype in dc.all_shapes():
            q = dc.q_rows(n_out, A * B, dtype)
            for t in dc.TEMPERATURES:
                if t == 0.0:
                    continue
                y = dc.exponents(q, t)
                n += len(y)
                n_sub += int(((y > -745.0) & (y < -708.5)).sum())
                y.tofile(f)
    assert n > 10 ** 6 and n_sub > 1000  # the GPU tests do reach the subnormal range
    out = subprocess.run([exe, "1000000", "200000", ys], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout, out.stdout
    total = int(out.stdout.split("n=")[1].split()[0])
    assert total == 1200000 + n, out.stdout
