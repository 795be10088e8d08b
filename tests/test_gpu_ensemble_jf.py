"""SimpleBroyden, SimpleKlement and SimpleDFSane on ensembles (nk_batch_solve_broyden / _klement / _dfsane and their _f32
twins): the reference's own GPU case, its known answers, and system-by-system parity with the NumPy restatement in
simple_jf_reference.py. Where the residual is built from + − × ÷ and sqrt alone, retcodes and iteration counts are equal on
every system and the iterates agree to 1e-12 relative in Float64 and to 2 ulp in Float32."""
import ctypes as C

import numpy as np
import pytest

import simple_jf_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32
METHODS = tuple(R.SOLVERS)
DTYPES = [pytest.param(np.float64, id="float64"), pytest.param(np.float32, id="float32")]


def _solve(nls, src, u0, P, name, dtype=np.float64, alg_kw=None, **kw):
    prob = nls.ImmutableNonlinearProblem(src, np.asarray(u0, dtype=dtype), np.asarray(P, dtype=dtype), eltype=dtype)
    return nls.vectorized_solve(prob, getattr(nls, name)(**(alg_kw or {})), **kw)


def _ref(f, name, u0, P, dtype, alg_kw=None, **kw):
    return R.SOLVERS[name](f, u0, P, dtype=dtype, **(alg_kw or {}), **kw)


def _assert_parity(sol, ref, dtype):
    x, _fx, rc, it, _ = ref
    assert (sol.retcode_raw == rc).all(), np.flatnonzero(sol.retcode_raw != rc)[:10]
    assert (sol.iters == it).all(), np.flatnonzero(sol.iters != it)[:10]
    u = np.asarray(sol.u)
    assert u.dtype == dtype
    assert (np.isnan(u) == np.isnan(x)).all()
    ok = np.isfinite(x)
    err = np.abs(u[ok].astype(float) - x[ok].astype(float))
    if dtype is np.float64:
        assert (err <= 1e-12 * np.abs(x[ok])).all(), err.max()
    else:
        assert (err <= 2 * np.spacing(np.abs(x[ok]).astype(F32)).astype(float)).all(), err.max()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_reference_gpu_case(nls, name, dtype):
    """test/gpu/cuda_tests__item1.jl: f(u) = u .* u .- 2 from [1, 1] with abstol = 1f-6: Success, max|resid| ≤ abstol"""
    sol = _solve(nls, R.QUADRATIC, [1.0, 1.0], [[2.0, 2.0]], name, dtype, abstol=1e-6)
    assert sol.retcode[0] == "Success" and np.max(np.abs(sol.resid)) <= F32(1e-6)
    assert np.allclose(sol.u, np.sqrt(2.0), rtol=1e-5)


@pytest.mark.parametrize("name", METHODS)
def test_known_answers_on_device(nls, name):
    """rootfind_tests__item3.jl: quadratic_f from [1, 1] and from 1.0, p = 2, abstol 1e-9, and (__item4.jl) DFSane on
    newton_fails as one 7-unknown system: Success with max|f| < 1e-9, the restatement's iterations"""
    for u0 in ([1.0, 1.0], [1.0]):
        P = np.full((1, len(u0)), 2.0)
        sol = _solve(nls, R.QUADRATIC, u0, P, name, abstol=1e-9)
        assert sol.retcode[0] == "Success" and np.max(np.abs(sol.u * sol.u - 2.0)) < 1e-9
        _assert_parity(sol, _ref(R.quadratic_f, name, u0, P, np.float64, abstol=1e-9), np.float64)
    if name == "SimpleDFSane":
        u0 = np.array([-10.0, -1.0, 1.0, 2.0, 3.0, 4.0, 10.0])
        sol = _solve(nls, R.NEWTON_FAILS, u0, np.zeros((1, 7)), name, abstol=1e-9)
        assert sol.retcode[0] == "Success" and np.max(np.abs(R.newton_fails_f(sol.u, np.zeros((1, 7))))) < 1e-9
        _assert_parity(sol, _ref(R.newton_fails_f, name, u0, np.zeros((1, 7)), np.float64, abstol=1e-9), np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_parity_quadratic_sweep(nls, name, dtype):
    """the tutorial's sweep p = 1:1000 from [1, 1] (Float32 at abstol 1f-4: |u*u - p| cannot go below ulp(p) = 6.1e-5)"""
    P = np.repeat(np.arange(1, 1001, dtype=float)[:, None], 2, axis=1)
    tol = 1e-4 if dtype is np.float32 else None
    sol = _solve(nls, R.QUADRATIC, [1.0, 1.0], P, name, dtype, abstol=tol)
    assert (sol.retcode == "Success").all()
    _assert_parity(sol, _ref(R.quadratic_f, name, [1.0, 1.0], P, dtype, abstol=tol), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_parity_p2(nls, name, dtype):
    """p2_f of the tutorial with 1024 random parameter sets from [1, 2, 3, 4], maxiters 200: its root is singular, so
    most systems run the full 200 iterations, and every one of them must follow the restatement's trajectory"""
    P = np.random.default_rng(7).random((1024, 4)) + 0.05
    sol = _solve(nls, R.P2, [1.0, 2.0, 3.0, 4.0], P, name, dtype, maxiters=200)
    _assert_parity(sol, _ref(R.p2_f, name, [1.0, 2.0, 3.0, 4.0], P, dtype, maxiters=200), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [16, 33, 64])
@pytest.mark.parametrize("name", METHODS)
def test_parity_dense_coupled_scratch_sizes(nls, name, n, dtype):
    """8 < n ≤ 64 (per thread, from scratch): 100 systems with one start each, all Success"""
    rng = np.random.default_rng(n)
    P = rng.uniform(1.0, 4.0, (100, n))
    u0 = rng.uniform(0.5, 2.0, (100, n))
    sol = _solve(nls, R.DENSE_COUPLED, u0, P, name, dtype, maxiters=200)
    assert (sol.retcode == "Success").all()
    _assert_parity(sol, _ref(R.dense_f, name, u0, P, dtype, maxiters=200), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_transcendental_roots_agree(nls, name, dtype):
    """exp / sin / tanh: the device's libm and NumPy's may differ in the last bit, so the trajectories may part, and from a
    few starts they end at different roots of this system (it has several). Every device Success is a root (f evaluated in
    Float64 at most 1e-10, or 1e-4 for Float32), and where both succeed the roots agree within 1e-9 (Float64) or 2e-4
    (Float32) relative on at least 95 % (90 %) of the systems."""
    rng = np.random.default_rng(3)
    utrue = rng.uniform(0.2, 1.2, (300, 3))
    P = np.array([[np.exp(u[0]) + u[1] * u[2], np.sin(u[1]) + u[0] ** 2, u[2] ** 3 + np.tanh(u[0])] for u in utrue])
    u0 = utrue + 0.05 * rng.standard_normal((300, 3))
    sol = _solve(nls, R.TRIG, u0, P, name, dtype, maxiters=500)
    x, _f, rc, _it, _ = _ref(R.trig_f, name, u0, P, dtype, maxiters=500)
    ok = sol.retcode_raw == R.SUCCESS
    both = ok & (rc == R.SUCCESS)
    assert ok.mean() >= 0.4 and abs(ok.mean() - (rc == R.SUCCESS).mean()) <= 0.1
    f64 = np.max(np.abs(R.trig_f(sol.u[ok].astype(float), P[ok].astype(dtype).astype(float))), axis=1)
    assert f64.max() <= (1e-10 if dtype is np.float64 else 1e-4), f64.max()
    tol = 1e-9 if dtype is np.float64 else 2e-4
    rel = np.max(np.abs(sol.u[both].astype(float) - x[both]) / np.maximum(1.0, np.abs(x[both])), axis=1)
    assert (rel <= tol).mean() >= 0.9, np.sort(rel)[-5:]


@pytest.mark.parametrize("dtype", DTYPES)
def test_dfsane_history_in_long_line_searches(nls, dtype):
    """where the line search keeps failing (an abstol out of reach), k advances by inner passes and the slot each merit
    value goes to, mod1(k, M), decides which values the non-monotone test compares against: newton_fails as seven scalar
    systems at abstol 1e-9, and the quadratic at abstol 1e-12, both with M = 10 and M = 3"""
    nf0 = np.array([-10.0, -1.0, 1.0, 2.0, 3.0, 4.0, 10.0])[:, None]
    Pq = np.repeat(np.linspace(1.0, 4.0, 500)[:, None], 2, axis=1)
    for M in (10, 3):
        sol = _solve(nls, R.NEWTON_FAILS, nf0, np.zeros((7, 1)), "SimpleDFSane", dtype, alg_kw=dict(M=M), abstol=1e-9,
                     maxiters=300)
        ref = _ref(R.newton_fails_f, "SimpleDFSane", nf0, np.zeros((7, 1)), dtype, alg_kw=dict(M=M), abstol=1e-9, maxiters=300)
        _assert_parity(sol, ref, dtype)
        sol = _solve(nls, R.QUADRATIC, [1.0, 1.0], Pq, "SimpleDFSane", dtype, alg_kw=dict(M=M), abstol=1e-12)
        ref = _ref(R.quadratic_f, "SimpleDFSane", [1.0, 1.0], Pq, dtype, alg_kw=dict(M=M), abstol=1e-12)
        _assert_parity(sol, ref, dtype)
        if dtype is np.float32:
            assert ref[4]["inner_passes"].mean() > 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_nondefault_parameters_reach_the_kernel(nls, dtype):
    """Broyden alpha, DFSane M = 1, n_exp = 1 and σ₁ = 0.25: each run differs from the default one and matches the restatement"""
    rng = np.random.default_rng(11)
    P = rng.uniform(1.0, 4.0, (256, 4))
    u0 = rng.uniform(0.5, 2.0, (256, 4)) + rng.standard_normal((256, 4))
    for name, kw in (("SimpleBroyden", dict(alpha=0.5)), ("SimpleDFSane", dict(M=1)), ("SimpleDFSane", dict(n_exp=1)),
                     ("SimpleDFSane", dict(sigma_1=0.25))):
        base = _solve(nls, R.DENSE_COUPLED, u0, P, name, dtype, maxiters=300)
        sol = _solve(nls, R.DENSE_COUPLED, u0, P, name, dtype, alg_kw=kw, maxiters=300)
        assert (sol.iters != base.iters).any() or not np.array_equal(sol.u, base.u), (name, kw)
        _assert_parity(sol, _ref(R.dense_f, name, u0, P, dtype, alg_kw=kw, maxiters=300), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_cases(nls, dtype):
    # Broyden's iszero shortcut: 0 iterations; Klement and DFSane take one step
    for name, iters in (("SimpleBroyden", 0), ("SimpleKlement", 1), ("SimpleDFSane", 1)):
        sol = _solve(nls, R.QUADRATIC, [2.0, 3.0], [[4.0, 9.0]], name, dtype)
        assert sol.retcode[0] == "Success" and sol.iters[0] == iters and (sol.u[0] == [2.0, 3.0]).all()
    # a NaN residual never terminates: MaxIters after exactly maxiters, no hang
    for name in METHODS:
        sol = _solve(nls, R.QUADRATIC, [1.0, 1.0], [[np.nan, 2.0], [2.0, 2.0]], name, dtype, maxiters=50)
        assert list(sol.retcode) == ["MaxIters", "Success"] and sol.iters[0] == 50
    # Klement's reset: the flat part leaves J at exactly 0, the next iteration resets it (2 and 3 times), then Success
    P = np.full((2, 1), 0.5)
    u0 = np.array([[-2.5], [-3.5]])
    ref = _ref(R.flat_then_quadratic_f, "SimpleKlement", u0, P, dtype)
    assert list(ref[4]["resets"]) == [2, 3]
    sol = _solve(nls, R.FLAT_THEN_QUADRATIC, u0, P, "SimpleKlement", dtype)
    assert (sol.retcode == "Success").all()
    _assert_parity(sol, ref, dtype)
    # DFSane running out of maxiters inside the line search: the last trial point is taken and checked
    for maxiters in (1, 2, 3):
        ref = _ref(R.quadratic_f, "SimpleDFSane", [1.0, 1.0], [[2.0, 2.0]], dtype, maxiters=maxiters)
        sol = _solve(nls, R.QUADRATIC, [1.0, 1.0], [[2.0, 2.0]], "SimpleDFSane", dtype, maxiters=maxiters)
        assert sol.retcode[0] == "MaxIters" and sol.iters[0] == maxiters
        _assert_parity(sol, ref, dtype)
        if maxiters == 1:
            assert ref[4]["exhausted"][0] == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", METHODS)
def test_host_device_and_u0_layouts_agree_bitwise(nls, dev, name, dtype):
    import torch
    rng = np.random.default_rng(5)
    P = rng.uniform(1.0, 4.0, (300, 4)).astype(dtype)
    u0 = np.array([1.0, 1.5, 0.5, 2.0], dtype=dtype)
    host = _solve(nls, R.DENSE_COUPLED, u0, P, name, dtype, maxiters=300)
    prob = nls.ImmutableNonlinearProblem(R.DENSE_COUPLED, torch.tensor(u0, device=dev), torch.tensor(P, device=dev), eltype=dtype)
    devs = nls.vectorized_solve(prob, getattr(nls, name)(), maxiters=300)
    assert devs.u.is_cuda and devs.u.dtype == (torch.float32 if dtype is np.float32 else torch.float64)
    assert host.u.tobytes() == devs.u.cpu().numpy().tobytes() and host.resid.tobytes() == devs.resid.cpu().numpy().tobytes()
    assert (host.iters == devs.iters).all() and (host.retcode_raw == devs.retcode_raw).all()
    per = _solve(nls, R.DENSE_COUPLED, np.tile(u0, (300, 1)), P, name, dtype, maxiters=300)
    assert host.u.tobytes() == per.u.tobytes() and (host.iters == per.iters).all()


def _ptrs(*arrays):
    return [C.c_void_p(a.ctypes.data) for a in arrays]


def test_invalid_arguments(nls):
    from nonlinearsolve_jl_amd import _lib as L
    from nonlinearsolve_jl_amd.core import _BatchKernel
    lib = L.lib()
    ctx = nls.default_context()
    nb, n = 16, 4
    h64 = _BatchKernel.get(ctx, R.QUADRATIC, n, n, 0)
    h32 = _BatchKernel.get(ctx, R.QUADRATIC, n, n, L.BATCH_FLOAT32)
    P, u0 = np.full((nb, n), 2.0), np.ones(n)
    u, r = np.empty((nb, n)), np.empty((nb, n))
    rc, it = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32)
    pu0, pP, pu, pr, prc, pit = _ptrs(u0, P, u, r, rc, it)
    dfs = lambda h, M, ne: lib.nk_batch_solve_dfsane(h, nb, pu0, 0, pP, L.HOST, 0.0, 100, -1.0, -1.0, -1.0, M, -1.0, -1.0,
                                                      -1.0, ne, pu, pr, prc, pit)
    for M, ne in ((-1, 0), (33, 0), (0, 3), (0, -1)):
        assert dfs(h64, M, ne) == -1, (M, ne)
    assert dfs(h64, 0, 0) == 0 and (rc == 1).all()
    assert dfs(h64, 32, 1) == 0 and (rc == 1).all()
    # the other precision's entry points
    assert lib.nk_batch_solve_broyden(h32, nb, pu0, 0, pP, L.HOST, 0.0, 100, -1.0, pu, pr, prc, pit) == -1
    assert b"Float32" in lib.nk_last_error()
    assert lib.nk_batch_solve_klement(h32, nb, pu0, 0, pP, L.HOST, 0.0, 100, pu, pr, prc, pit) == -1
    assert dfs(h32, 0, 0) == -1
    u0f, Pf, uf, rf = u0.astype(F32), P.astype(F32), u.astype(F32), r.astype(F32)
    pu0f, pPf, puf, prf = _ptrs(u0f, Pf, uf, rf)
    assert lib.nk_batch_solve_broyden_f32(h64, nb, pu0f, 0, pPf, L.HOST, 0.0, 100, -1.0, puf, prf, prc, pit) == -1
    assert b"Float64" in lib.nk_last_error()
    assert lib.nk_batch_solve_klement_f32(h64, nb, pu0f, 0, pPf, L.HOST, 0.0, 100, puf, prf, prc, pit) == -1
    assert lib.nk_batch_solve_dfsane_f32(h64, nb, pu0f, 0, pPf, L.HOST, 0.0, 100, -1.0, -1.0, -1.0, 0, -1.0, -1.0, -1.0, 0,
                                         puf, prf, prc, pit) == -1
    assert lib.nk_batch_solve_klement_f32(h32, nb, pu0f, 0, pPf, L.HOST, 0.0, 100, puf, prf, prc, pit) == 0
    assert (rc == 1).all()
    with pytest.raises(ValueError):
        _solve(nls, R.QUADRATIC, u0, P, "SimpleDFSane", alg_kw=dict(M=33))


def test_newton_and_trust_region_unchanged_after_the_jf_module_is_built(nls):
    """on one object: Newton and trust-region results before and after the Jacobian-free module is compiled and run are
    bitwise equal"""
    from nonlinearsolve_jl_amd import _lib as L
    lib = L.lib()
    ctx = nls.default_context()
    nb, n = 512, 4
    rng = np.random.default_rng(9)
    P = rng.uniform(1.0, 4.0, (nb, n))
    u0 = rng.uniform(0.5, 2.0, (nb, n))
    h = C.c_void_p()
    assert lib.nk_batch_create(ctx._h, R.DENSE_COUPLED.encode(), n, n, 0, C.byref(h)) == 0
    try:
        def run(kind):
            u, r = np.empty((nb, n)), np.empty((nb, n))
            rc, it = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32)
            a = _ptrs(u0, P, u, r, rc, it)
            if kind == "newton":
                st = lib.nk_batch_solve(h, nb, a[0], 1, a[1], L.HOST, 0.0, 100, *a[2:])
            elif kind == "tr":
                st = lib.nk_batch_solve_trust_region(h, nb, a[0], 1, a[1], L.HOST, 0.0, 100, -1.0, -1.0, -1.0, -1.0, -1.0, -1,
                                                     *a[2:])
            elif kind == "broyden":
                st = lib.nk_batch_solve_broyden(h, nb, a[0], 1, a[1], L.HOST, 0.0, 100, -1.0, *a[2:])
            elif kind == "klement":
                st = lib.nk_batch_solve_klement(h, nb, a[0], 1, a[1], L.HOST, 0.0, 100, *a[2:])
            else:
                st = lib.nk_batch_solve_dfsane(h, nb, a[0], 1, a[1], L.HOST, 0.0, 100, -1.0, -1.0, -1.0, 0, -1.0, -1.0, -1.0, 0,
                                               *a[2:])
            assert st == 0, lib.nk_last_error()
            return u.tobytes() + r.tobytes() + rc.tobytes() + it.tobytes()
        before = run("newton"), run("tr")
        for kind in ("broyden", "klement", "dfsane"):
            run(kind)
        assert (run("newton"), run("tr")) == before
    finally:
        lib.nk_batch_destroy(h)
