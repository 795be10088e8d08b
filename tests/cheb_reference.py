"""The Chebyshev iteration's coefficient recurrence (csrc/nk_cheb.h) in Python floats, operation for operation: the oracle of
tests/test_cheb_coef.py (bit equality with the header) and the coefficients tests/test_gpu_cheb.py drives the iteration with."""


def coefficients(lmin, lmax, steps):
    """(1/θ, [(c1, c2) of step 1 … steps − 1]) on [lmin, lmax]; the interval may lie on either side of zero."""
    theta = 0.5 * (lmax + lmin)
    delta = 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    out = []
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return 1.0 / theta, out
