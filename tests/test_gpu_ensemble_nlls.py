"""Ensembles of small nonlinear least-squares problems on the device (nk_batch_solve_gauss_newton,
nk_batch_solve_trust_region_nlls and their _f32 twins; ImmutableNonlinearLeastSquaresProblem + vectorized_solve): the
reference's own case (least_squares_tests__item1.jl), and problem-by-problem parity with the NumPy restatement in
simple_nlls_reference.py. Where the residual is built from + − × ÷ alone, retcodes and iteration counts are equal on every
problem; where exp / cos enter, a problem may differ in its iteration count only if one of the restatement's two deciding
residual norms lies within a factor 2 of abstol, and at most 1 % of a family may. u meets the calibrated bound
(simple_nlls_reference.BOUNDS) against the restatement everywhere. Every test prints the device maximum next to its bound."""
import ctypes as C

import numpy as np
import pytest

import simple_nlls_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32
METHODS = tuple(R.SOLVERS)
DTYPES = [pytest.param(np.float64, id="float64"), pytest.param(np.float32, id="float32")]


def _alg(nls, method, jac=False):
    return nls.SimpleGaussNewton(jac=jac) if method == "SimpleGaussNewton" else nls.SimpleTrustRegion(jac=jac)


def _solve(nls, fam, method, dtype, jac=None, u0=None, **kw):
    jac = (fam.jac is not None) if jac is None else jac
    prob = nls.ImmutableNonlinearLeastSquaresProblem(fam.source, np.asarray(fam.u0 if u0 is None else u0, dtype=dtype),
                                                     np.asarray(fam.p, dtype=dtype), fam.m, eltype=dtype)
    kw.setdefault("maxiters", fam.maxiters)
    kw.setdefault("abstol", fam.abstol(dtype))
    return nls.vectorized_solve(prob, _alg(nls, method, jac), **kw)


def _assert_u(sol, ref, fam, method, dtype, what=""):
    u = np.asarray(sol.u)
    assert u.dtype == dtype and np.asarray(sol.resid).shape == (fam.p.shape[0], fam.m)
    assert np.isfinite(u).all()
    dev = float(R.rel_dev(u, ref[0]).max())
    bound = R.BOUNDS[(fam.name, np.dtype(dtype).name, method)]
    print(f"{fam.name} {np.dtype(dtype).name} {method}{what}: device max {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound, (dev, bound)


def _assert_counts(sol, ref, fam, dtype):
    """retcodes and iteration counts equal — on every problem of an algebraic family; in a transcendental one a problem may
    differ only where a deciding norm of the restatement lies within a factor 2 of abstol, and at most 1 % may"""
    _x, _f, rc, it, info = ref
    diff = (sol.retcode_raw != rc) | (sol.iters != it)
    if not fam.transcendental:
        assert not diff.any(), np.flatnonzero(diff)[:10]
        return
    tol = fam.abstol(dtype) or (R.ABSTOL_F32 if dtype is np.float32 else R.ABSTOL_F64)
    pn, fn = info["pass_norm"].astype(float), info["fail_norm"].astype(float)
    near = ((pn >= tol / 2) & (pn <= 2 * tol)) | ((fn >= tol / 2) & (fn <= 2 * tol))
    print(f"{fam.name}: {int(diff.sum())} of {diff.size} problems left out of the iteration-count comparison")
    assert near[diff].all(), np.flatnonzero(diff & ~near)[:10]
    assert diff.mean() <= 0.01, diff.mean()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_reference_case(nls, method, dtype):
    """least_squares_tests__item1.jl: four parameters of θ₁·exp(θ₂x)·cos(θ₃x + θ₄) from five points, start θ_true + 0.1:
    Success; ‖resid‖∞ < 1e-12 in Float64 as the reference asserts (Float32: below its default abstol)"""
    fam = R.expcos_reference_case()
    sol = _solve(nls, fam, method, dtype)
    assert sol.retcode[0] == "Success"
    assert np.max(np.abs(sol.resid)) < (1e-12 if dtype is np.float64 else R.ABSTOL_F32)
    ref = fam.run(method, dtype)
    _assert_counts(sol, ref, fam, dtype)
    _assert_u(sol, ref, fam, method, dtype)
    assert np.allclose(sol.u[0], R.EXPCOS_THETA, rtol=1e-9 if dtype is np.float64 else 1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_expcos_family(nls, method, dtype):
    """2000 problems, θ_true scaled by ±20 %, starts perturbed by up to ±0.4, default abstol of the dtype: all Success"""
    fam = R.expcos_family()
    sol = _solve(nls, fam, method, dtype)
    assert (sol.retcode == "Success").all(), np.unique(sol.retcode, return_counts=True)
    ref = fam.run(method, dtype)
    assert (ref[2] == R.SUCCESS).all()
    _assert_counts(sol, ref, fam, dtype)
    _assert_u(sol, ref, fam, method, dtype)


ALGEBRAIC = {"michaelis_menten_8": lambda: R.michaelis_menten_family(8), "michaelis_menten_16": lambda: R.michaelis_menten_family(16),
             "michaelis_menten_64": lambda: R.michaelis_menten_family(64, nb=200), "rational": R.rational_family,
             "poly_squared": R.poly_squared_family, "squares_and_products_4": lambda: R.squares_and_products_family(4),
             "squares_and_products_12": lambda: R.squares_and_products_family(12)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(ALGEBRAIC))
def test_algebraic_families_follow_the_restatement(nls, name, method, dtype):
    """+ − × ÷ only (Michaelis–Menten with m = 8, 16, 64 — the last reads p in place and runs from scratch —, a rational
    with n = 3, a squared polynomial with nk_jac, n = 12 > 8 unknowns): the kernel and the restatement perform the same
    operations, so retcodes and iteration counts are equal on every problem"""
    fam = ALGEBRAIC[name]()
    sol = _solve(nls, fam, method, dtype)
    ref = fam.run(method, dtype)
    assert (sol.retcode == "Success").all()
    _assert_counts(sol, ref, fam, dtype)
    _assert_u(sol, ref, fam, method, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_analytic_and_dual_jacobians_agree(nls, method, dtype):
    fam = R.poly_squared_family()
    a = _solve(nls, fam, method, dtype, jac=True)
    d = _solve(nls, fam, method, dtype, jac=False)
    assert (a.retcode_raw == d.retcode_raw).all() and (a.iters == d.iters).all()
    _assert_u(d, fam.run(method, dtype, use_jac=False), fam, method, dtype, " (dual numbers)")
    bound = R.BOUNDS[(fam.name, np.dtype(dtype).name, method)]
    assert float(R.rel_dev(a.u, d.u).max()) <= bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_noisy_fit_ends_in_maxiters_at_the_least_squares_solution(nls, method, dtype):
    """a non-zero residual at the optimum never passes ‖f‖₂ ≤ abstol: MaxIters after maxiters = 20, retcodes, iteration
    counts and u as the restatement; Gauss–Newton has converged by then, so the gradient Jᵀf is at rounding level against
    ‖J‖‖f‖ (Float64 arithmetic on the returned u: 1e-8 in Float64, 1e-3 in Float32)"""
    fam = R.michaelis_menten_family(16, noise=0.02, maxiters=20)
    sol = _solve(nls, fam, method, dtype)
    ref = fam.run(method, dtype)
    assert (sol.retcode == "MaxIters").all() and (sol.iters == 20).all()
    _assert_counts(sol, ref, fam, dtype)
    _assert_u(sol, ref, fam, method, dtype)
    if method == "SimpleGaussNewton":
        u, p = np.asarray(sol.u, dtype=float), np.asarray(fam.p, dtype=dtype).astype(float)
        f = R._eval(fam.f, u, p, fam.m, np.float64)
        J = R._dual_jac(fam.f, u, p, fam.m, np.float64)
        g = np.einsum("bmn,bm->bn", J, f)
        rel = np.abs(g).max(axis=1) / (np.linalg.norm(J, axis=(1, 2)) * np.linalg.norm(f, axis=1))
        print(f"noisy {np.dtype(dtype).name}: max |J'f|inf/(|J||f|) = {rel.max():.3e}")
        assert rel.max() <= (1e-8 if dtype is np.float64 else 1e-3)
        assert (np.linalg.norm(f, axis=1) > 1e-3).all()
        assert np.allclose(np.asarray(sol.resid, dtype=float), f, atol=1e-12 if dtype is np.float64 else 1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_rank_deficient_jacobian(nls, method, dtype):
    """two identical Jacobian columns and noisy data: finite output, no hang, never Success"""
    fam = R.rank_deficient_family()
    sol = _solve(nls, fam, method, dtype)
    assert np.isfinite(sol.u).all() and np.isfinite(sol.resid).all()
    assert (sol.retcode != "Success").all() and (sol.iters <= 50).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(nls, dtype):
    sq = R.squares_and_products_family(4, nb=3)
    ut = np.array([[1.0, 2.0, 0.5, 1.5]] * 3)
    p = R._plain(R.squares_and_products_f, ut, np.zeros((3, 8)))
    p[1, 0] = np.nan
    u0 = ut.copy()
    u0[2] += 0.1
    fam = R.Family("edge", sq.source, sq.f, 4, 8, u0, p, maxiters=30)
    # iszero(f(u0)): Gauss–Newton returns at once, the trust region's check before the loop does the same; a NaN residual
    # never terminates
    for method in METHODS:
        sol = _solve(nls, fam, method, dtype)
        ref = fam.run(method, dtype)
        assert sol.retcode[0] == "Success" and sol.iters[0] == 0 and (np.asarray(sol.u[0]) == ut[0].astype(dtype)).all()
        assert sol.retcode[1] != "Success" and sol.retcode[2] == "Success"
        assert (sol.retcode_raw == ref[2]).all() and (sol.iters == ref[3]).all(), (sol.iters, ref[3])
    assert _solve(nls, fam, "SimpleGaussNewton", dtype).iters[1] == 30
    # m == n: a least-squares problem that happens to be square runs the same QR kernel with the 2-norm check
    quad = R.Family("square", R.N_OUTPUTS_ONLY, lambda u, p: [u[i] * u[i] - p[:, i] for i in range(3)], 3, 3,
                    np.ones((2, 3)), np.array([[2.0, 3.0, 4.0], [1.5, 2.5, 9.0]]), abstol32=1e-5)
    for method in METHODS:
        sol = _solve(nls, quad, method, dtype)
        ref = quad.run(method, dtype)
        assert (sol.retcode == "Success").all() and (sol.retcode_raw == ref[2]).all() and (sol.iters == ref[3]).all()
        assert np.allclose(np.asarray(sol.u) ** 2, quad.p, rtol=1e-12 if dtype is np.float64 else 1e-5)
    # a source that writes n outputs, built with m > n: the other residuals are zero
    more = R.Family("padded", R.N_OUTPUTS_ONLY, lambda u, p: [u[i] * u[i] - p[:, i] for i in range(3)] + [0 * u[0], 0 * u[0]],
                    3, 5, np.ones((2, 3)), quad.p, abstol32=1e-5)
    sol = _solve(nls, more, "SimpleGaussNewton", dtype)
    assert (sol.retcode == "Success").all() and (np.asarray(sol.resid)[:, 3:] == 0).all()
    assert np.allclose(np.asarray(sol.u) ** 2, quad.p, rtol=1e-12 if dtype is np.float64 else 1e-5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_host_device_and_u0_layouts_agree_bitwise(nls, dev, method, dtype):
    import torch
    fam = R.michaelis_menten_family(8, nb=300)
    u0 = np.array([2.0, 1.0], dtype=dtype)
    P = fam.p.astype(dtype)
    host = _solve(nls, fam, method, dtype, u0=u0)
    prob = nls.ImmutableNonlinearLeastSquaresProblem(fam.source, torch.tensor(u0, device=dev), torch.tensor(P, device=dev),
                                                     fam.m, eltype=dtype)
    devs = nls.vectorized_solve(prob, _alg(nls, method))
    assert devs.u.is_cuda and devs.u.dtype == (torch.float32 if dtype is np.float32 else torch.float64)
    assert tuple(devs.resid.shape) == (300, 8)
    assert host.u.tobytes() == devs.u.cpu().numpy().tobytes() and host.resid.tobytes() == devs.resid.cpu().numpy().tobytes()
    assert (host.iters == devs.iters).all() and (host.retcode_raw == devs.retcode_raw).all()
    per = _solve(nls, fam, method, dtype, u0=np.tile(u0, (300, 1)))
    assert host.u.tobytes() == per.u.tobytes() and host.resid.tobytes() == per.resid.tobytes() and (host.iters == per.iters).all()


def _ptrs(*arrays):
    return [C.c_void_p(a.ctypes.data) for a in arrays]


def test_invalid_arguments(nls):
    from nonlinearsolve_jl_amd import _lib as L
    from nonlinearsolve_jl_amd.core import _BatchKernel
    lib = L.lib()
    ctx = nls.default_context()
    nb, n, m = 16, 2, 8
    fam = R.michaelis_menten_family(8, nb=nb)
    src = fam.source
    hn64 = _BatchKernel.get(ctx, src, n, 2 * m, 0, m)
    hn32 = _BatchKernel.get(ctx, src, n, 2 * m, L.BATCH_FLOAT32, m)
    hsq = _BatchKernel.get(ctx, R.N_OUTPUTS_ONLY, 2, 2, 0)
    P, u0 = fam.p.copy(), fam.u0.copy()
    u, r = np.empty((nb, n)), np.empty((nb, m))
    rc, it = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32)
    pu0, pP, pu, pr, prc, pit = _ptrs(u0, P, u, r, rc, it)
    tr = (-1.0, -1.0, -1.0, -1.0, -1.0, -1)
    assert lib.nk_batch_solve_gauss_newton(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == 0 and (rc == 1).all()
    assert lib.nk_batch_solve_trust_region_nlls(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, *tr, pu, pr, prc, pit) == 0
    assert (rc == 1).all()
    # a square entry point on a least-squares object, and the reverse
    assert lib.nk_batch_solve(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == -1
    assert b"least-squares" in lib.nk_last_error()
    assert lib.nk_batch_solve_trust_region(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, *tr, pu, pr, prc, pit) == -1
    assert lib.nk_batch_solve_broyden(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, -1.0, pu, pr, prc, pit) == -1
    assert lib.nk_batch_solve_klement(hn64, nb, pu0, 1, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == -1
    assert lib.nk_batch_solve_gauss_newton(hsq, nb, pu0, 1, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == -1
    assert b"square" in lib.nk_last_error()
    assert lib.nk_batch_solve_trust_region_nlls(hsq, nb, pu0, 1, pP, L.HOST, 0.0, 100, *tr, pu, pr, prc, pit) == -1
    # the other precision's entry points
    u0f, Pf, uf, rf = u0.astype(F32), P.astype(F32), u.astype(F32), r.astype(F32)
    pu0f, pPf, puf, prf = _ptrs(u0f, Pf, uf, rf)
    assert lib.nk_batch_solve_gauss_newton(hn32, nb, pu0, 1, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == -1
    assert b"Float32" in lib.nk_last_error()
    assert lib.nk_batch_solve_trust_region_nlls(hn32, nb, pu0, 1, pP, L.HOST, 0.0, 100, *tr, pu, pr, prc, pit) == -1
    assert lib.nk_batch_solve_gauss_newton_f32(hn64, nb, pu0f, 1, pPf, L.HOST, 0.0, 100, puf, prf, prc, pit) == -1
    assert b"Float64" in lib.nk_last_error()
    assert lib.nk_batch_solve_trust_region_nlls_f32(hn64, nb, pu0f, 1, pPf, L.HOST, 0.0, 100, *tr, puf, prf, prc, pit) == -1
    assert lib.nk_batch_solve_gauss_newton_f32(hn32, nb, pu0f, 1, pPf, L.HOST, 0.0, 100, puf, prf, prc, pit) == 0
    assert (rc == 1).all()
    # m < n
    h = C.c_void_p()
    assert lib.nk_batch_create_nlls(ctx._h, src.encode(), 3, 2, 4, 0, C.byref(h)) == -1
    assert b"n <= m <= 64" in lib.nk_last_error()
    with pytest.raises(ValueError):
        nls.ImmutableNonlinearLeastSquaresProblem(src, np.ones(3), np.ones((4, 4)), 2)


def test_jacobian_free_methods_are_refused(nls):
    fam = R.michaelis_menten_family(8, nb=4)
    prob = nls.ImmutableNonlinearLeastSquaresProblem(fam.source, fam.u0, fam.p, fam.m)
    for alg in (nls.SimpleBroyden(), nls.SimpleKlement(), nls.SimpleDFSane()):
        with pytest.raises(TypeError, match="least-squares"):
            nls.vectorized_solve(prob, alg)
    assert nls.SimpleGaussNewton is nls.SimpleNewtonRaphson
