"""The NumPy restatement of SimpleBroyden / SimpleKlement / SimpleDFSane (simple_jf_reference.py) pinned to the reference's
own known answers (lib/SimpleNonlinearSolve/test/core/rootfind_tests__item3.jl, __item4.jl), to first steps worked out by
hand, and driven through the rare branches: Klement's reset, DFSane's line search cut short by maxiters, σ = 0 or NaN, and
a NaN residual. No GPU."""
import numpy as np
import pytest

import simple_jf_reference as R

METHODS = tuple(R.SOLVERS)
DTYPES = (np.float64, np.float32)


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("u0", [[1.0, 1.0], 1.0], ids=["vector", "scalar"])
def test_quadratic_known_answer(name, u0):
    """quadratic_f from [1, 1] and from 1.0, p = 2, abstol 1e-9: Success with max|f| < 1e-9, at sqrt(2)"""
    n = np.size(u0)
    x, fx, rc, it, _ = R.SOLVERS[name](R.quadratic_f, u0, np.full(n, 2.0), abstol=1e-9)
    assert rc[0] == R.SUCCESS and 0 < it[0] < 1000
    assert np.max(np.abs(R.quadratic_f(x, 2.0))) < 1e-9 and np.max(np.abs(fx)) < 1e-9
    assert np.allclose(x, np.sqrt(2.0))


def test_dfsane_newton_fails_known_answer():
    """SimpleDFSane on newton_fails as one 7-unknown system from [-10, -1, 1, 2, 3, 4, 10] (where Newton fails)"""
    u0 = [-10.0, -1.0, 1.0, 2.0, 3.0, 4.0, 10.0]
    x, fx, rc, it, _ = R.simple_dfsane(R.newton_fails_f, u0, np.zeros(7), abstol=1e-9)
    assert rc[0] == R.SUCCESS
    assert np.max(np.abs(R.newton_fails_f(x, np.zeros((1, 7))))) < 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_steps_by_hand(dtype):
    T = dtype
    u0, p = np.array([1.0, 3.0], dtype=T), np.array([2.0, 5.0], dtype=T)
    f0 = u0 * u0 - p                                                  # [-1, 4]
    # Broyden: x₁ = u0 − init_α·f(u0), init_α = max(‖u0‖₂, 1)/(2‖f(u0)‖₂) (‖f‖ ≥ 1e-5), or 1/alpha
    x, _, rc, it, _ = R.simple_broyden(R.quadratic_f, u0, p, maxiters=1, dtype=T)
    a = np.sqrt(T(10)) / (T(2) * np.sqrt(T(17)))
    assert x.dtype == T and rc[0] == R.MAXITERS and it[0] == 1
    assert (x[0] == u0 - a * f0).all()
    x, *_ = R.simple_broyden(R.quadratic_f, u0, p, maxiters=1, alpha=4.0, dtype=T)
    assert (x[0] == u0 - f0 / T(4)).all()
    # Klement: J = 1, so the first δx is f(u0)
    x, *_ = R.simple_klement(R.quadratic_f, u0, p, maxiters=1, dtype=T)
    assert (x[0] == u0 - f0).all()
    # DFSane: the first trial point is u0 − σ₁·f(u0)
    for s1 in (1.0, 0.5):
        *_, info = R.simple_dfsane(R.quadratic_f, u0, p, maxiters=1, sigma_1=s1, dtype=T)
        assert (info["first_trial"][0] == u0 - T(s1) * f0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_broyden_iszero_shortcut_and_one_step_for_the_others(dtype):
    """iszero(f(u0)) ends Broyden after 0 steps; Klement and DFSane have no such shortcut and pass the check after one"""
    u0, p = [2.0, 3.0], [4.0, 9.0]
    x, _, rc, it, _ = R.simple_broyden(R.quadratic_f, u0, p, dtype=dtype)
    assert rc[0] == R.SUCCESS and it[0] == 0 and (x[0] == u0).all()
    for name in ("SimpleKlement", "SimpleDFSane"):
        x, _, rc, it, _ = R.SOLVERS[name](R.quadratic_f, u0, p, dtype=dtype)
        assert rc[0] == R.SUCCESS and it[0] == 1 and (x[0] == u0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_klement_reset_branch(dtype):
    """flat f = −1 left of 0: each step there leaves J at exactly 0, the next one resets it; from −2.5 and −3.5 the
    iterate walks out of the flat part after 2 and 3 resets and converges"""
    x, _, rc, it, info = R.simple_klement(R.flat_then_quadratic_f, [[-2.5], [-3.5]], [[0.5], [0.5]], dtype=dtype)
    assert list(info["resets"]) == [2, 3]
    assert (rc == R.SUCCESS).all() and np.allclose(x[:, 0], np.sqrt(0.5), rtol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dfsane_line_search_cut_short_by_maxiters(dtype):
    """quadratic from [1, 1], p = 2, maxiters = 1: both first trials fail the non-monotone test, one inner pass brings k
    to maxiters, and the last trial point u0 + α₊·d (d = −σ₁f = [1, 1], α₊ ∈ [τ_min, τ_max]) is taken and checked"""
    x, _, rc, it, info = R.simple_dfsane(R.quadratic_f, [1.0, 1.0], [2.0, 2.0], maxiters=1, dtype=dtype)
    assert info["exhausted"][0] == 1 and info["inner_passes"][0] == 1
    assert rc[0] == R.MAXITERS and it[0] == 1
    assert x[0, 0] == x[0, 1] and 1.1 - 1e-6 <= x[0, 0] <= 1.5 + 1e-6
    # a longer run reaches Success through passes of the inner loop, which count towards k
    _, _, rc, it, info = R.simple_dfsane(R.quadratic_f, [1.0, 1.0], [2.0, 2.0], dtype=dtype)
    assert rc[0] == R.SUCCESS and info["inner_passes"][0] >= 1 and info["exhausted"][0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sigma_1", [0.0, np.nan], ids=["zero", "nan"])
def test_dfsane_sigma_zero_or_nan_propagates_nan(dtype, sigma_1):
    """sign(σ)·clamp(|σ|, σ_min, σ_max) keeps 0 and NaN: σ₁ = 0 gives δx = 0, then σ = 0/0 = NaN; from there every trial
    is NaN and the line search runs k to maxiters (fmin / fmax would have clamped NaN to σ_min and converged)"""
    x, _, rc, it, _ = R.simple_dfsane(R.quadratic_f, [1.0, 1.0], [2.0, 2.0], sigma_1=sigma_1, maxiters=40, dtype=dtype)
    assert rc[0] == R.MAXITERS and it[0] == 40 and np.isnan(x).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_nan_residual_runs_to_maxiters(dtype, name):
    x, fx, rc, it, _ = R.SOLVERS[name](R.quadratic_f, [1.0, 1.0], [np.nan, 2.0], maxiters=25, dtype=dtype)
    assert rc[0] == R.MAXITERS and it[0] == 25 and np.isnan(fx).any()


def test_dfsane_parameters_change_the_run():
    """M, n_exp and σ₁ reach the iteration: each changes the iteration count on the dense coupled system"""
    rng = np.random.default_rng(4)
    P = rng.uniform(1.0, 4.0, (32, 4))
    u0 = rng.uniform(0.5, 2.0, (32, 4)) + rng.standard_normal((32, 4))
    base = R.simple_dfsane(R.dense_f, u0, P, maxiters=300)
    assert (base[2] == R.SUCCESS).mean() > 0.9
    for kw in (dict(M=1), dict(n_exp=1), dict(sigma_1=0.25)):
        other = R.simple_dfsane(R.dense_f, u0, P, maxiters=300, **kw)
        assert (other[3] != base[3]).any(), kw
