// Host check of aigar_math::pow_glibc(e, y) on the Boltzmann selection's domain
// (decide.inc: d_i = pow(e, (q_i - max) / temperature), y <= 0) against the C
// library's pow, bit for bit: n_wide values of y spread over [-760, 0], n_sub inside
// [-746, -708] (results below 2^-1022, glibc's specialcase re-rounding, and the flush
// to zero), and every double of the optional file (the y of the GPU tests' rows).
// g++ -O2 -std=c++17 -ffp-contract=off -I aigar_amd/csrc tools/gen/check_decide_pow.cpp -o /tmp/check_decide_pow
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "aigar_math.h"

using namespace aigar_math;

static long bad = 0, n_sub_seen = 0, n_zero_seen = 0;
static void check(double y) {
  const double e = 2.718281828459045;  // math.e
  const double a = pow_glibc(e, y), b = pow(e, y);
  if (b != 0.0 && b < 0x1p-1022) n_sub_seen++;
  if (b == 0.0) n_zero_seen++;
  if (as_u64(a) != as_u64(b)) {
    if (++bad < 10) printf("MISMATCH y=%a pow_glibc=%a libm=%a\n", y, a, b);
  }
}

int main(int argc, char **argv) {
  const long n_wide = argc > 1 ? atol(argv[1]) : 1000000, n_sub = argc > 2 ? atol(argv[2]) : 100000;
  std::mt19937_64 g(7);
  std::uniform_real_distribution<double> um(0.0, 1.0);
  long n = 0;
  for (long i = 0; i < n_wide; i++, n++) check(i % 2 ? -760.0 * um(g) : -760.0 * (double)i / (double)n_wide);
  for (long i = 0; i < n_sub; i++, n++) check(i % 2 ? -746.0 + 38.0 * um(g) : -746.0 + 38.0 * (double)i / (double)n_sub);
  if (argc > 3) {
    FILE *f = fopen(argv[3], "rb");
    if (!f) {
      printf("cannot open %s\n", argv[3]);
      return 2;
    }
    std::vector<double> buf(1 << 16);
    size_t k;
    while ((k = fread(buf.data(), sizeof(double), buf.size(), f)) > 0)
      for (size_t j = 0; j < k; j++, n++) check(buf[j]);
    fclose(f);
  }
  printf("n=%ld subnormal=%ld zero=%ld mismatches=%ld\n", n, n_sub_seen, n_zero_seen, bad);
  return bad ? 1 : 0;
}
