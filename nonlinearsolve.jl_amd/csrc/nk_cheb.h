// Coefficients of the Chebyshev iteration for A x = b on the interval [lmin, lmax] (Saad, Iterative Methods, Alg. 12.1), in
// plain C++: no HIP in here, so tests/cheb_coef_dump.cpp compiles it with g++ (tests/test_cheb_coef.py). The polynomial
// preconditioner and every multigrid smoother take their numbers from it.
//   step 0: d = r/θ                       → (c1, c2) = (0, inv_theta())
//   step k: d' = c1·d + c2·r, ρ' = 1/(2σ − ρ), (c1, c2) = (ρ'ρ, 2ρ'/δ)     → next()
// with θ = ½(λmax + λmin), δ = ½(λmax − λmin), σ = θ/δ, ρ₀ = 1/σ. The interval may lie on either side of zero (the
// Brusselator hierarchy runs on −[λmax/4, λmax]). The library is built with -ffp-contract=off and the callers' results are
// pinned bit for bit: the order of the operations below is part of the contract.
#pragma once

struct nk_cheb_coef {
  double theta, delta, sigma, rho;
  nk_cheb_coef(double lmin, double lmax)
      : theta(0.5 * (lmax + lmin)), delta(0.5 * (lmax - lmin)), sigma(theta / delta), rho(1.0 / sigma) {}
  double inv_theta() const { return 1.0 / theta; }
  void next(double *c1, double *c2) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    *c1 = rho_new * rho;
    *c2 = 2.0 * rho_new / delta;
    rho = rho_new;
  }
};
