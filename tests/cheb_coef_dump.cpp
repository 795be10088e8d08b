// Host-only driver of the Chebyshev coefficients (csrc/nk_cheb.h) for tests/test_cheb_coef.py.
//   cheb_coef_dump steps lmin lmax [lmin lmax …]   (the bounds as C hexadecimal floats: exact)
// Per interval: the line "interval lmin lmax 1/θ", then one line "c1 c2" for every step after the first, all as %a.
#include "nk_cheb.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
  if (argc < 4 || (argc & 1) != 0) {
    fprintf(stderr, "usage: cheb_coef_dump steps lmin lmax [lmin lmax ...]\n");
    return 2;
  }
  const int steps = atoi(argv[1]);
  for (int a = 2; a + 1 < argc; a += 2) {
    const double lmin = strtod(argv[a], nullptr), lmax = strtod(argv[a + 1], nullptr);
    nk_cheb_coef co(lmin, lmax);
    printf("interval %a %a %a\n", lmin, lmax, co.inv_theta());
    for (int k = 1; k < steps; ++k) {
      double c1, c2;
      co.next(&c1, &c2);
      printf("%a %a\n", c1, c2);
    }
  }
  return 0;
}
