"""Float32 ensembles of small systems (ImmutableNonlinearProblem(..., eltype=float32), nk_batch_solve*_f32): the
tutorial's element type (docs/src/tutorials/nonlinear_solve_gpus.md:146-160), checked system by system against the float32
restatement of SimpleNewtonRaphson / SimpleTrustRegion in ensemble_f32.py, and against the Float64 device path."""
import ctypes as C

import numpy as np
import pytest

import ensemble_f32 as F

pytestmark = pytest.mark.gpu

F32 = np.float32
FP64_DEFAULT_ABSTOL = float(np.finfo(float).eps) ** 0.8   # 3.0e-13


def _solve(nls, src, u0, P, alg=None, **kw):
    return nls.vectorized_solve(nls.ImmutableNonlinearProblem(src, u0, P, eltype=np.float32), alg or nls.SimpleNewtonRaphson(), **kw)


def test_quadratic_sweep_float32(nls):
    """f(u,p) = u.*u .- p over p = 1:1000 (nonlinear_solve_gpus.md:47-62) in Float32 with the tutorial's abstol = 1f-4
    (|u*u - p| cannot go below ulp(p) = 6.1e-5 at p = 1000): u ≈ sqrt.(p), every system Success, Newton steps as the
    float32 restatement takes them."""
    nb, n = 1000, 3
    P = np.repeat(np.arange(1, nb + 1, dtype=F32)[:, None], n, axis=1)
    sol = _solve(nls, F.QUADRATIC, np.ones(n, dtype=F32), P, abstol=1e-4)
    assert sol.u.dtype == np.float32 and sol.resid.dtype == np.float32
    assert (sol.retcode == "Success").all()
    assert np.max(np.abs(sol.u.astype(float) - np.sqrt(P.astype(float))) / np.sqrt(P.astype(float))) <= 1e-6
    _x, _f, rco, ito = F.ensemble_f32(F.simple_newton_raphson_f32, F.quadratic_f, F.quadratic_jac, np.ones(n), P, abstol=1e-4)
    assert (rco == F.SUCCESS).all()
    assert (sol.iters == ito).mean() >= 0.99 and np.max(np.abs(sol.iters - ito)) <= 1


def test_tutorial_p2_float32_on_device(nls, dev):
    """p2_f exactly as the tutorial states it: rand(Float32, 4) parameters (+0.05, away from sqrt(0)), u0 = [1f0, 2f0, 3f0,
    4f0], 1024 systems, device-resident torch tensors in and float32 tensors out."""
    import torch
    rng = np.random.default_rng(7)
    P = rng.random((1024, 4), dtype=F32) + F32(0.05)
    u0 = np.array([1, 2, 3, 4], dtype=F32)
    prob = nls.ImmutableNonlinearProblem(F.P2, torch.tensor(u0, device=dev), torch.tensor(P, device=dev), eltype=torch.float32)
    sol = nls.vectorized_solve(prob, nls.SimpleNewtonRaphson(), maxiters=200)
    assert sol.u.dtype == torch.float32 and sol.resid.dtype == torch.float32 and sol.u.is_cuda and sol.resid.is_cuda
    _x, _f, rco, ito = F.ensemble_f32(F.simple_newton_raphson_f32, F.p2_f, F.p2_jac, u0, P, maxiters=200)
    rc = sol.retcode_raw
    assert (rc == rco).mean() >= 0.99
    assert ((rc == rco) & (sol.iters == ito)).mean() >= 0.95
    ok = rc == F.SUCCESS
    assert ok.mean() > 0.9
    assert float(sol.resid.abs().max(dim=1).values.cpu().numpy()[ok].max()) <= 2.8909994e-6


def test_default_abstol_is_float32s(nls, dev):
    """No abstol: the default is eps(Float32)^(4/5) = 2.89e-6 (common_defaults.jl:53), not Float64's 3.0e-13 — an ensemble
    that reaches Success does so with residuals the FP64 default would not accept."""
    import torch
    rng = np.random.default_rng(1)
    P = rng.uniform(1.0, 4.0, (500, 4)).astype(F32)
    q = _solve(nls, F.QUADRATIC, np.ones(4, dtype=F32), P)
    Pp = rng.random((512, 4), dtype=F32) + F32(0.05)
    p2 = nls.vectorized_solve(nls.ImmutableNonlinearProblem(F.P2, torch.tensor([1, 2, 3, 4], dtype=torch.float32, device=dev),
                                                            torch.tensor(Pp, device=dev), eltype="float32"))
    for sol, resid in ((q, q.resid), (p2, p2.resid.cpu().numpy())):
        ok = sol.retcode_raw == F.SUCCESS
        assert ok.all()
        rmax = np.max(np.abs(resid), axis=1)
        assert rmax.max() <= 2.8909994e-6
        assert (rmax > FP64_DEFAULT_ABSTOL).any()


def test_analytic_jacobian_per_system_u0_float32(nls):
    """flags 3 (Float32 + nk_jac) with one start per system on the transcendental system: retcodes as the float32
    restatement's, roots within 1e-4 (relative) of the Float64 device solution of the same systems."""
    rng = np.random.default_rng(3)
    nb = 300
    utrue = rng.uniform(0.2, 1.2, (nb, 3))
    P = np.array([[np.exp(u[0]) + u[1] * u[2], np.sin(u[1]) + u[0] ** 2, u[2] ** 3 + np.tanh(u[0])] for u in utrue]).astype(F32)
    u0 = (utrue + 0.05 * rng.standard_normal((nb, 3))).astype(F32)
    _x, _f, rco, ito = F.ensemble_f32(F.simple_newton_raphson_f32, F.trig_f, F.trig_jac, u0, P)
    sol = _solve(nls, F.TRIG_WITH_JAC, u0, P, nls.SimpleNewtonRaphson(jac=True))
    assert (sol.retcode_raw == rco).all()
    ref = nls.vectorized_solve(nls.ImmutableNonlinearProblem(F.TRIG_WITH_JAC, u0.astype(float), P.astype(float)),
                               nls.SimpleNewtonRaphson(jac=True))
    assert (ref.retcode == "Success").all() and ref.u.dtype == np.float64
    ok = sol.retcode_raw == F.SUCCESS
    assert ok.mean() > 0.95
    rel = np.max(np.abs(sol.u[ok] - ref.u[ok]) / np.maximum(1.0, np.abs(ref.u[ok])), axis=1)
    assert (rel <= 1e-4).mean() >= 0.97
    # where the two roots differ by more, the system is ill-conditioned: the gap stays within the first-order bound
    # 2‖J⁻¹‖∞‖f(u32)‖∞ (J at the Float64 root, f of the Float32 root evaluated in Float64)
    import ensemble_sources as E
    P64 = P.astype(float)
    for b in np.flatnonzero(ok):
        bound = 2 * np.linalg.norm(np.linalg.inv(E.trig_jac(ref.u[b], P64[b])), np.inf) * \
            np.max(np.abs(E.trig_f(sol.u[b].astype(float), P64[b])))
        assert np.max(np.abs(sol.u[b] - ref.u[b])) <= max(1e-4 * max(1.0, np.max(np.abs(ref.u[b]))), bound), b
    dual = _solve(nls, F.TRIG_WITH_JAC, u0, P)                    # the same systems with the dual-number Jacobian
    assert (dual.retcode_raw == rco).mean() >= 0.99


def test_shortcut_maxiters_and_nan_float32(nls):
    """iszero(f(u0)) ⇒ Success after 0 steps; a singular start runs NaN to maxiters (NaN never terminates); a regular
    one takes the restatement's steps — the Float64 semantics in Float32."""
    P = np.array([[9, 9], [2, 2], [2, 2]], dtype=F32)
    u0 = np.array([[3, 3], [0, 0], [1, 1]], dtype=F32)
    sol = _solve(nls, F.QUADRATIC, u0, P, maxiters=9)
    assert list(sol.retcode) == ["Success", "MaxIters", "Success"]
    assert list(sol.iters) == [0, 9, F.simple_newton_raphson_f32(F.quadratic_f, F.quadratic_jac, u0[2], P[2])[3]]
    assert np.isnan(sol.u[1]).all() and sol.u.dtype == np.float32
    tr = _solve(nls, F.QUADRATIC, u0, P, nls.SimpleTrustRegion(), maxiters=9)
    assert tr.retcode[0] == "Success" and tr.iters[0] == 0


@pytest.mark.parametrize("n", [9, 16, 33, 64])
def test_medium_systems_one_per_wavefront_float32(nls, n):
    """8 < n ≤ 64 on the wave kernel in Float32 (one 32-bit readlane per crossing, float wave max for the pivot): dense
    coupled residual, 130 systems (not a multiple of 4); retcodes as the float32 restatement's, ≥ 95 % equal step counts,
    solutions within 1e-4 (relative) of the Float64 path's."""
    rng = np.random.default_rng(n)
    nb = 130
    P = rng.uniform(1.0, 4.0, (nb, n)).astype(F32)
    u0 = rng.uniform(0.5, 2.0, (nb, n)).astype(F32)
    sol = _solve(nls, F.DENSE_COUPLED, u0, P, maxiters=100)
    _x, _f, rco, ito = F.ensemble_f32(F.simple_newton_raphson_f32, F.dense_f, F.dense_jac, u0, P, maxiters=100)
    assert (sol.retcode_raw == rco).all() and (sol.retcode == "Success").all()
    assert (sol.iters == ito).mean() >= 0.95
    ref = nls.vectorized_solve(nls.ImmutableNonlinearProblem(F.DENSE_COUPLED, u0.astype(float), P.astype(float)),
                               nls.SimpleNewtonRaphson(), maxiters=100)
    assert (ref.retcode == "Success").all()
    assert np.max(np.abs(sol.u - ref.u) / np.maximum(1.0, np.abs(ref.u))) <= 1e-4


def test_simple_trust_region_float32_vs_restatement(nls):
    """SimpleTrustRegion in Float32 (every threshold and factor taken as T(·)) on the dense coupled system from rough
    starts: retcodes and step counts as the float32 restatement's."""
    rng = np.random.default_rng(5)
    nb, n = 200, 4
    P = rng.uniform(1.0, 4.0, (nb, n)).astype(F32)
    u0 = (rng.uniform(0.5, 2.0, (nb, n)) + 1.5 * rng.standard_normal((nb, n))).astype(F32)
    sol = _solve(nls, F.DENSE_COUPLED, u0, P, nls.SimpleTrustRegion(), maxiters=300)
    _x, _f, rco, ito = F.ensemble_f32(F.simple_trust_region_f32, F.dense_f, F.dense_jac, u0, P, maxiters=300)
    assert (sol.retcode_raw == rco).mean() >= 0.99
    assert ((sol.retcode_raw == rco) & (sol.iters == ito)).mean() >= 0.95
    ok = sol.retcode_raw == F.SUCCESS
    assert ok.mean() > 0.8 and np.max(np.abs(sol.resid[ok])) <= 2.8909994e-6


NEWTON_FAILS_F32 = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  const T a = nk_real(0.21640425613334457) + nk_real(216.40425613334457) / (nk_real(1) + nk_real(0.0006250000000000001) * (u[0] * u[0]));
  const T b = nk_real(0.21640425613334457) + nk_real(216.40425613334457) / (nk_real(1) + a * a);
  f[0] = nk_real(0.010000000000000002) + nk_real(10.000000000000002) / (nk_real(1) + b * b) - nk_real(0.0011552453009332421) * u[0] - p[0];
}
"""


def test_simple_trust_region_newton_fails_float32(nls):
    """rootfind_tests__item10.jl's `newton_fails` as seven scalar systems in Float32: with the Float32 default abstol the
    trust region converges from every start; with the Float64 fixture's abstol = 1e-9, out of reach of a float32 residual,
    every start ends in ShrinkThresholdExceeded — the Float64 retcode semantics, in Float32."""
    u0 = np.array([-10.0, -1.0, 1.0, 2.0, 3.0, 4.0, 10.0], dtype=F32)[:, None]
    P = np.zeros((7, 1), dtype=F32)
    ok = _solve(nls, NEWTON_FAILS_F32, u0, P, nls.SimpleTrustRegion(), maxiters=1000)
    assert (ok.retcode == "Success").all() and np.max(np.abs(ok.resid)) <= 2.8909994e-6
    tight = _solve(nls, NEWTON_FAILS_F32, u0, P, nls.SimpleTrustRegion(), abstol=1e-9, maxiters=1000)
    assert (tight.retcode == "ShrinkThresholdExceeded").all()
    assert (tight.iters > ok.iters).all() and (tight.iters < 1000).all()


def test_precision_mismatch_is_an_error_and_float32_is_deterministic(nls):
    from nonlinearsolve_jl_amd import _lib as L
    from nonlinearsolve_jl_amd.core import _BatchKernel
    ctx = nls.default_context()
    nb, n = 64, 4
    P = np.random.default_rng(2).uniform(1.0, 4.0, (nb, n))
    u0 = np.ones(n)
    h32 = _BatchKernel.get(ctx, F.QUADRATIC, n, n, L.BATCH_FLOAT32)
    h64 = _BatchKernel.get(ctx, F.QUADRATIC, n, n, 0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    u, r = np.empty((nb, n)), np.empty((nb, n))
    rc, it = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.int32)
    # a Float32 object through the Float64 entry points, and the other way round: NK_E_INVALID with a message
    assert L.lib().nk_batch_solve(h32, nb, p(u0), 0, p(P), L.HOST, 0.0, 100, p(u), p(r), p(rc), p(it)) == -1
    assert b"Float32" in L.lib().nk_last_error()
    assert L.lib().nk_batch_solve_trust_region(h32, nb, p(u0), 0, p(P), L.HOST, 0.0, 100, -1.0, -1.0, -1.0, -1.0, -1.0, -1,
                                               p(u), p(r), p(rc), p(it)) == -1
    u0f, Pf = u0.astype(F32), P.astype(F32)
    uf, rf = np.empty((nb, n), dtype=F32), np.empty((nb, n), dtype=F32)
    assert L.lib().nk_batch_solve_f32(h64, nb, p(u0f), 0, p(Pf), L.HOST, 0.0, 100, p(uf), p(rf), p(rc), p(it)) == -1
    assert b"Float64" in L.lib().nk_last_error()
    assert L.lib().nk_batch_solve_trust_region_f32(h64, nb, p(u0f), 0, p(Pf), L.HOST, 0.0, 100, -1.0, -1.0, -1.0, -1.0, -1.0,
                                                   -1, p(uf), p(rf), p(rc), p(it)) == -1
    # the objects still work through their own entry points, and two identical Float32 calls give the same bits
    a = _solve(nls, F.QUADRATIC, u0f, Pf)
    b = _solve(nls, F.QUADRATIC, u0f, Pf)
    assert (a.retcode == "Success").all()
    assert a.u.tobytes() == b.u.tobytes() and a.resid.tobytes() == b.resid.tobytes() and (a.iters == b.iters).all()
    d = nls.vectorized_solve(nls.ImmutableNonlinearProblem(F.QUADRATIC, u0, P))
    assert d.u.dtype == np.float64 and (d.retcode == "Success").all()
