"""The NumPy restatement of the least-squares ensemble kernels (simple_nlls_reference.py) against what is known without a
device: the reference's own case (least_squares_tests__item1.jl), numpy.linalg.lstsq at every QR solve, the edge cases, and
the calibration of the device bounds against the same restatement run in long double."""
import numpy as np
import pytest

import simple_nlls_reference as R

METHODS = tuple(R.SOLVERS)
DTYPES = [pytest.param(np.float64, id="float64"), pytest.param(np.float32, id="float32")]


@pytest.mark.parametrize("method", METHODS)
def test_reference_case_known_answer(method):
    """θ₁·exp(θ₂x)·cos(θ₃x + θ₄) at x = −1 … 1, θ_true = (1, 0.1, 2, 0.5), start θ_true + 0.1: Success with
    ‖resid‖∞ < 1e-12 (the reference's assertion); Gauss–Newton in 5 iterations, the trust region in 4"""
    fam = R.expcos_reference_case()
    x, fx, rc, it, _ = fam.run(method, np.float64)
    assert rc[0] == R.SUCCESS and np.max(np.abs(fx)) < 1e-12
    assert it[0] == (5 if method == "SimpleGaussNewton" else 4)
    assert np.allclose(x[0], R.EXPCOS_THETA, rtol=1e-10)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_expcos_family_is_usable_in_full(method, dtype):
    """all 2000 problems end in Success, in both precisions, at the default abstol of the dtype"""
    fam = R.expcos_family()
    x, fx, rc, it, _ = fam.run(method, dtype)
    assert (rc == R.SUCCESS).all()
    assert it.max() <= (8 if method == "SimpleGaussNewton" else 13)
    tol = R.ABSTOL_F32 if dtype is np.float32 else R.ABSTOL_F64
    assert (np.sqrt((fx.astype(float) ** 2).sum(axis=1)) <= tol * 1.001).all()


def test_dual_numbers_give_the_jacobian():
    """the Dual restatement against central differences, and nk_jac's twin against the duals"""
    for fam in (R.expcos_family(nb=20), R.rational_family(nb=20), R.poly_squared_family(nb=20), R.squares_and_products_family(12, nb=5)):
        J = R._dual_jac(fam.f, fam.u0, fam.p, fam.m, np.float64)
        assert J.shape == (fam.u0.shape[0], fam.m, fam.n)
        h = 1e-6
        for k in range(fam.n):
            e = np.zeros(fam.n)
            e[k] = h
            fd = (R._eval(fam.f, fam.u0 + e, fam.p, fam.m, np.float64) - R._eval(fam.f, fam.u0 - e, fam.p, fam.m, np.float64)) / (2 * h)
            assert np.allclose(J[:, :, k], fd, rtol=1e-6, atol=1e-7)
        if fam.jac is not None:
            assert np.allclose(fam.jac(fam.u0, fam.p), J, rtol=1e-14)


@pytest.mark.parametrize("shape", [(5, 4), (8, 3), (16, 2), (8, 8), (24, 12), (3, 1)])
def test_every_qr_solve_agrees_with_lstsq(shape):
    """pivoted Householder QR against numpy.linalg.lstsq on random full-rank J, f (κ₂ up to ~1e3): relative difference of the
    solutions below 1e-11, and the factorisation itself: R upper triangular with non-increasing |r_kk|, ‖Qᵀf‖ = ‖f‖"""
    m, n = shape
    rng = np.random.default_rng(m * 100 + n)
    J = rng.standard_normal((200, m, n)) * np.logspace(0, 2, n)[None, None, :]
    f = rng.standard_normal((200, m))
    fac = R.qr_factor(J)
    dx = R.qr_solve(fac, f)
    for b in range(200):
        want = np.linalg.lstsq(J[b], f[b], rcond=None)[0]
        assert np.max(np.abs(dx[b] - want)) <= 1e-11 * np.max(np.abs(want)), (b, dx[b], want)
    d = np.abs(np.stack([fac[0][:, k, k] for k in range(n)], axis=1))
    assert (d[:, 1:] <= d[:, :-1] * (1 + 1e-12)).all()
    assert (fac[2] >= np.arange(n)).all() and (fac[2] < n).all()


def test_qr_steps_inside_the_solvers_agree_with_lstsq():
    """every Gauss–Newton step of the reference case is lstsq's: re-run the iteration with lstsq in place of the QR"""
    fam = R.expcos_family(nb=50)
    x = fam.u0.copy()
    for _ in range(4):
        fx = R._eval(fam.f, x, fam.p, fam.m, np.float64)
        J = R._dual_jac(fam.f, x, fam.p, fam.m, np.float64)
        dx = R.qr_solve(R.qr_factor(J), fx)
        want = np.stack([np.linalg.lstsq(J[b], fx[b], rcond=None)[0] for b in range(50)])
        assert np.max(np.abs(dx - want)) <= 1e-11 * np.max(np.abs(want))
        x = x - dx


def test_rank_deficient_columns_get_a_zero_step():
    """two identical columns: the second pivot falls below m·eps·|r_11| and its unknown does not move (the basic solution);
    a zero matrix gives a zero step; NaN propagates instead of being masked"""
    rng = np.random.default_rng(0)
    a = rng.standard_normal((50, 8))
    J = np.stack([a, a, rng.standard_normal((50, 8))], axis=2)
    f = rng.standard_normal((50, 8))
    dx = R.qr_solve(R.qr_factor(J), f)
    assert np.isfinite(dx).all() and ((dx[:, 0] == 0) | (dx[:, 1] == 0)).all()
    want = np.stack([np.linalg.lstsq(J[b][:, [0, 2]], f[b], rcond=None)[0] for b in range(50)])
    assert np.allclose(np.stack([dx[:, 0] + dx[:, 1], dx[:, 2]], axis=1), want, rtol=1e-10)
    assert (R.qr_solve(R.qr_factor(np.zeros((2, 5, 3))), np.ones((2, 5))) == 0).all()
    J[0, 3, 2] = np.nan
    assert np.isnan(R.qr_solve(R.qr_factor(J), f)[0]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(dtype):
    sq = R.squares_and_products_family(4, nb=3)
    ut = np.array([[1.0, 2.0, 0.5, 1.5]] * 3)
    p = R._plain(R.squares_and_products_f, ut, np.zeros((3, 8)))
    p[1, 0] = np.nan
    u0 = ut.copy()
    u0[2] += 0.1
    fam = R.Family("edge", sq.source, sq.f, 4, 8, u0, p, maxiters=30)
    # iszero shortcut (Gauss–Newton) and the check before the loop (trust region): 0 iterations, u untouched
    for method in METHODS:
        x, fx, rc, it, _ = fam.run(method, dtype)
        assert rc[0] == R.SUCCESS and it[0] == 0 and (x[0] == ut[0]).all()
        assert rc[2] == R.SUCCESS and 0 < it[2] < 10
    # a NaN residual never terminates: Gauss–Newton runs out of iterations, the trust region shrinks (r is NaN) until
    # maxiters = 30 < max_shrink_times + 1 ends it, or ShrinkThresholdExceeded at iteration 33 given the room
    assert fam.run("SimpleGaussNewton", dtype)[2][1] == R.MAXITERS and fam.run("SimpleGaussNewton", dtype)[3][1] == 30
    assert fam.run("SimpleTrustRegion", dtype)[2][1] == R.MAXITERS
    x, fx, rc, it, _ = fam.run("SimpleTrustRegion", dtype, maxiters=100)
    assert rc[1] == R.SHRINK and it[1] == 33
    # m == n
    quad = lambda u, p: [u[i] * u[i] - p[:, i] for i in range(3)]
    for method in METHODS:
        x, fx, rc, it, _ = R.SOLVERS[method](quad, np.ones(3), np.array([[2.0, 3.0, 4.0]]), 3, dtype=dtype,
                                             abstol=1e-5 if dtype is np.float32 else None)
        assert rc[0] == R.SUCCESS and np.allclose(x[0] ** 2, [2.0, 3.0, 4.0], rtol=1e-5)
    # m < n is refused
    for method in METHODS:
        with pytest.raises(ValueError, match="n <= m <= 64"):
            R.SOLVERS[method](lambda u, p: [u[0] - p[:, 0]], np.ones(2), np.ones((1, 1)), 1, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fits_with_a_nonzero_minimum_never_report_success(dtype):
    """noisy Michaelis–Menten data, maxiters = 20: Gauss–Newton ends in MaxIters at the least-squares solution (Jᵀf at
    rounding level against ‖J‖‖f‖). The trust region, given room, ends in ShrinkThresholdExceeded on most problems — once
    the step stops reducing ‖f‖, r < η₂ shrinks the radius 33 times in a row — and in MaxIters on the rest (476 + 24 of 500
    in Float64, 435 + 65 in Float32), never in Success."""
    fam = R.michaelis_menten_family(16, noise=0.02, maxiters=20)
    x, fx, rc, it, _ = fam.run("SimpleGaussNewton", dtype)
    assert (rc == R.MAXITERS).all() and (it == 20).all()
    u, p = x.astype(float), fam.p.astype(dtype).astype(float)
    f = R._eval(fam.f, u, p, fam.m, np.float64)
    J = R._dual_jac(fam.f, u, p, fam.m, np.float64)
    g = np.einsum("bmn,bm->bn", J, f)
    rel = np.abs(g).max(axis=1) / (np.linalg.norm(J, axis=(1, 2)) * np.linalg.norm(f, axis=1))
    # the returned u is a working-precision fixed point of u −= J \\ f: its gradient is ~ κ·eps·‖J‖‖f‖; κ₂(J) < 100 here
    assert rel.max() <= 1000 * np.finfo(dtype).eps, rel.max()
    assert (np.linalg.norm(f, axis=1) > 1e-2).all()
    x, fx, rc, it, _ = fam.run("SimpleTrustRegion", dtype)
    assert (rc == R.MAXITERS).all()
    x, fx, rc, it, _ = fam.run("SimpleTrustRegion", dtype, maxiters=1000)
    assert int((rc == R.SHRINK).sum()) == (476 if dtype is np.float64 else 435)
    assert int((rc == R.MAXITERS).sum()) == (24 if dtype is np.float64 else 65)


def test_bounds_are_eight_times_the_long_double_deviation_rounded_up():
    """Calibration. For every family, dtype and method: d = max over the problems of ‖u_T − u_ld‖∞/‖u_ld‖∞ between the
    restatement in the working precision T and in long double; BOUNDS holds 8·d rounded up to a power of two, and the
    restatement itself stays at or below a quarter of every bound."""
    seen = set()
    for fam in R.calibrated_families():
        for method in METHODS:
            ld = fam.run(method, np.longdouble)
            for dtype in (np.float64, np.float32):
                key = (fam.name, np.dtype(dtype).name, method)
                d = float(R.rel_dev(fam.run(method, dtype)[0], ld[0]).max())
                print(f"{key}: restatement {d:.3e}, bound {R.BOUNDS[key]:.3e}")
                assert R.BOUNDS[key] == R.bound_from(d), (key, d, R.BOUNDS[key])
                assert d <= R.BOUNDS[key] / 4
                seen.add(key)
    assert seen == set(R.BOUNDS)
