// Host check of aigar_math::log_glibc (the device's restatement of glibc 2.35's log)
// against the C library's log, which numpy's legacy Gaussian calls: the r2 = x1^2 + x2^2
// of the polar method on the 53-bit uniform grid, 1 - k 2^-53 and 1 + k 2^-52 for small k,
// both ends of the branch near 1 +- 300 ulps, every power of two, 2^-104 (the smallest
// non-zero r2 of the polar method), subnormals, and random values over 2^+-1000.  Any
// mismatch fails.  Host libm must be the glibc whose table aigar_glibc_log_tables.h holds.
// g++ -O2 -std=c++17 -ffp-contract=off -fno-builtin-log -I aigar_amd/csrc tools/gen/check_log.cpp -o /tmp/check_log
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "aigar_math.h"

using namespace aigar_math;

static long g_n = 0, g_bad = 0;

static void check(double x) {
  const double a = log_glibc(x), b = log(x);
  g_n++;
  if (as_u64(a) != as_u64(b) && !(a != a && b != b)) {
    if (++g_bad < 10) printf("MISMATCH x=%a log_glibc=%a libm=%a\n", x, a, b);
  }
}

static void around(double x, int ulps) {
  const uint64_t u = as_u64(x);
  for (int d = -ulps; d <= ulps; d++) check(as_double(u + (uint64_t)(int64_t)d));
}

int main(int argc, char **argv) {
  const long n = argc > 1 ? atol(argv[1]) : 10000000;
  std::mt19937_64 g(42);
  const double grid = 1.0 / 9007199254740992.0;  // 2^-53
  for (int k = 0; k <= 4096; k++) {
    check(1.0 - (double)k * 0x1p-53);
    check(1.0 + (double)k * 0x1p-52);
  }
  around(1.0 - 0x1p-4, 300);     // the near-1 branch's lower end
  around(1.0 + 0x1.09p-4, 300);  // ... and its upper end
  for (int e = -1074; e <= 1023; e++) check(ldexp(1.0, e));
  check(0x1p-104);
  around(0x1p-104, 8);
  for (int k = 1; k <= 4096; k++) check((double)k * 0x1p-1074);           // the smallest subnormals
  for (int k = 0; k < 4096; k++) check(as_double(g() >> 12));             // random subnormals
  around(0x1p-1022, 300);
  check(0x1.fffffffffffffp1023);
  const long per = (n - g_n) / 4 + 1;
  for (long it = 0; it < per; it++) {  // accepted r2 of the polar method
    double r2;
    do {
      const double x1 = 2.0 * ((double)(g() >> 11) * grid) - 1.0, x2 = 2.0 * ((double)(g() >> 11) * grid) - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    check(r2);
  }
  for (long it = 0; it < per; it++) {  // ... with both draws near 1/2: small r2
    const int s = 12 + (int)(g() % 52);  // offsets of +-2^51 .. +-1 grid steps
    const double x1 = 2.0 * (0.5 + (double)((int64_t)(g() >> s) - (int64_t)(1ull << (63 - s))) * grid) - 1.0;
    const double x2 = 2.0 * (0.5 + (double)((int64_t)(g() >> s) - (int64_t)(1ull << (63 - s))) * grid) - 1.0;
    const double r2 = x1 * x1 + x2 * x2;
    if (r2 != 0.0) check(r2);
  }
  for (long it = 0; it < per; it++)  // the near-1 branch, dense
    check(as_double(0x3fee000000000000ull + g() % 0x0003090000000000ull));
  for (long it = 0; it < per; it++)  // random values over 2^+-1000
    check(ldexp(1.0 + (double)(g() >> 12) * 0x1p-52, (int)(g() % 2001) - 1000));
  printf("n=%ld mismatches=%ld\n", g_n, g_bad);
  return g_bad ? 1 : 0;
}
