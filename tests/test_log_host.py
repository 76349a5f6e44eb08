"""Host check of the stepper's log (aigar_math.h log_glibc): the glibc restatement against
the C library's log, which numpy's legacy Gaussian -- the reference's exploration noise --
calls."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_log_glibc_matches_libm_log(tmp_path):
    """aigar_math::log_glibc == libm log on > 10^7 inputs: the polar method's r2 on the
    53-bit grid (small r2 included), 1 - k 2^-53 and 1 + k 2^-52, both ends of the branch
    near 1 +- 300 ulps, every power of two, 2^-104, subnormals, random values over
    2^+-1000.  -fno-builtin-log: the comparison is with the library's routine, not with a
    constant the compiler folded."""
    exe = str(tmp_path / "check_log")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin-log", "-I",
                           os.path.join(ROOT, "aigar_amd", "csrc"), os.path.join(ROOT, "tools", "gen", "check_log.cpp"),
                           "-o", exe])
    out = subprocess.run([exe, "12000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mismatches=0" in out.stdout, out.stdout
    assert int(out.stdout.split("n=")[1].split()[0]) >= 10 ** 7, out.stdout
