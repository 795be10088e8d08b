"""The coefficients of the Chebyshev iteration (csrc/nk_cheb.h) are plain host arithmetic, so they are checked here without a GPU:
tests/cheb_coef_dump.cpp is compiled with g++ (-ffp-contract=off, as the library) against the header and prints them.

Every (c1, c2) must equal, bit for bit, the same recurrence in Python floats (tests/cheb_reference.py), and lie within 256 ε
(ε = 2⁻⁵², relative) of the closed form in numpy.longdouble: ρ_k = T_k(σ)/T_{k+1}(σ), c1 = ρ_k ρ_{k−1}, c2 = 2 ρ_k/δ with
T_k(σ) = sign(σ)^k cosh(k·acosh|σ|). On exactly these inputs the float64 recurrence was measured at 89.8 ε in the worst case;
256 is the next power of two above that."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cheb_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMAX = (8.0, -1234.5, 3.7e6, 1.9999)
RATIO = (1.50000015, 4.0, 30.0, 100.0, 300.0, 1e4)
STEPS = 128                      # steps after the first
INTERVALS = [(lmax / ratio, lmax) for lmax in LMAX for ratio in RATIO]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """{(lmin, lmax): (1/θ, [(c1, c2)] * STEPS)} as the header computes them"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("cheb_coef") / "cheb_coef_dump")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "nonlinearsolve.jl_amd", "csrc"), os.path.join(ROOT, "tests", "cheb_coef_dump.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    args = [x.hex() for iv in INTERVALS for x in iv]
    lines = subprocess.run([exe, str(STEPS + 1)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "interval":
            cur = out[(float.fromhex(w[1]), float.fromhex(w[2]))] = (float.fromhex(w[3]), [])
        else:
            cur[1].append((float.fromhex(w[0]), float.fromhex(w[1])))
    assert list(out) == INTERVALS and all(len(v[1]) == STEPS for v in out.values())
    return out


@pytest.mark.parametrize("lmin,lmax", INTERVALS)
def test_header_equals_the_python_recurrence_bit_for_bit(dumped, lmin, lmax):
    inv_theta, coef = dumped[(lmin, lmax)]
    ref_inv_theta, ref = cheb_reference.coefficients(lmin, lmax, STEPS + 1)
    assert inv_theta.hex() == ref_inv_theta.hex()
    for k, (got, want) in enumerate(zip(coef, ref), start=1):
        assert (got[0].hex(), got[1].hex()) == (want[0].hex(), want[1].hex()), f"step {k}"


@pytest.mark.parametrize("lmin,lmax", INTERVALS)
def test_header_is_within_256_eps_of_the_closed_form(dumped, lmin, lmax):
    LD = np.longdouble
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 here")
    theta, delta = LD(0.5) * (LD(lmax) + LD(lmin)), LD(0.5) * (LD(lmax) - LD(lmin))
    sigma = theta / delta
    alpha, sign = np.arccosh(np.abs(sigma)), np.sign(sigma)
    T = [sign ** k * np.cosh(LD(k) * alpha) for k in range(STEPS + 2)]
    rho = [T[k] / T[k + 1] for k in range(STEPS + 1)]
    inv_theta, coef = dumped[(lmin, lmax)]
    eps = LD(2.0) ** -52
    worst = abs((LD(inv_theta) - 1 / theta) * theta)
    for k, (c1, c2) in enumerate(coef, start=1):
        e1, e2 = rho[k] * rho[k - 1], 2 * rho[k] / delta
        worst = max(worst, abs((LD(c1) - e1) / e1), abs((LD(c2) - e2) / e2))
    print(f"[{lmin!r}, {lmax!r}]: worst relative error {float(worst / eps):.1f} eps")
    assert worst <= 256 * eps
