"""SimpleTrustRegion for medium systems, one system per wavefront (nk_batch_trust_region_wave, 8 < n ≤ 64): lane j owns
column j of the dual-number Jacobian, the dogleg's norms and dot products are wave butterflies, and δᵀJᵀJδ comes from a
dual-number JVP. Checked system by system against the oracle's restatement of trust_region.jl on the cases of
wave_tr_cases.py, against the per-thread kernel (`per_wavefront=False`), at the edges of the launch geometry, in Float32, and
for what `vectorized_solve` dispatches where."""
import numpy as np
import pytest

import wave_tr_cases as W
from oracle import reference_restatement as R

pytestmark = pytest.mark.gpu

WAVE, THREAD = "nk_batch_trust_region_wave", "nk_batch_trust_region"
_solved = {}


def _solve(nls, case, n, f32=False, **kw):
    """the case's ensemble on the device (kept: several tests compare against the same Float64 wavefront result)"""
    key = (case, n, f32, tuple(sorted(kw.items())))
    if key not in _solved:
        src, _, _, ckw, start = W.CASES[case]
        P, u0 = W.inputs(n, start=start)
        prob = nls.ImmutableNonlinearProblem(src, u0, P, eltype=np.float32 if f32 else None)
        _solved[key] = nls.vectorized_solve(prob, nls.SimpleTrustRegion(**ckw), maxiters=W.MAXITERS, **kw)
    return _solved[key]


def _check(sol, ref, **kw):
    share = W.check_against_oracle(np.asarray(sol.u), np.asarray(sol.resid), sol.retcode_raw, sol.iters, ref, **kw)
    print(f"share with the oracle's step count {share:.4f}")
    return share


@pytest.mark.parametrize("case", list(W.CASES))
@pytest.mark.parametrize("n", W.NS)
def test_cases_vs_oracle(nls, case, n):
    """retcodes equal the oracle's on every system; retcode and step count on at least 0.97 of them, and there the solutions
    agree to 1e-10; every Success within eps^0.8"""
    sol = _solve(nls, case, n)
    assert sol.kernel == WAVE
    _check(sol, W.oracle(case, n))
    assert sol.u.shape == (W.NB, n) and sol.resid.shape == (W.NB, n)


def test_per_thread_switch(nls):
    """per_wavefront=False runs the per-thread kernel on the same inputs: the same retcodes, the same solutions to 1e-10"""
    wave, thread = _solve(nls, "rough", 16), _solve(nls, "rough", 16, per_wavefront=False)
    assert (wave.kernel, thread.kernel) == (WAVE, THREAD)
    assert np.array_equal(wave.retcode_raw, thread.retcode_raw)
    err = float(np.max(np.abs(wave.u - thread.u)))
    print(f"|u_wave - u_thread|_inf = {err:.2e}; steps equal on {(wave.iters == thread.iters).mean():.4f}")
    assert err < 1e-10


@pytest.mark.parametrize("nb", [1, 3, 4, 5])
def test_batch_sizes_around_a_workgroup(nls, nb):
    """4 systems per workgroup: a lone wavefront, a partly filled workgroup, a full one, one system into the next"""
    P, u0 = W.inputs(9)
    sol = nls.vectorized_solve(nls.ImmutableNonlinearProblem(W.DENSE_COUPLED, u0[:nb], P[:nb]), nls.SimpleTrustRegion(),
                               maxiters=W.MAXITERS)
    assert sol.kernel == WAVE
    _check(sol, tuple(a[:nb] for a in W.oracle("rough", 9)))


def test_edges_at_n9(nls, dev):
    import torch
    P, u0 = W.inputs(9)
    tr = nls.SimpleTrustRegion()

    def run(u0_, P_, **kw):
        sol = nls.vectorized_solve(nls.ImmutableNonlinearProblem(W.DENSE_COUPLED, u0_, P_), tr, **kw)
        assert sol.kernel == WAVE
        return sol

    def ref(u0_, P_, **kw):
        return W.oracle_solve(W.dense_f, W.dense_jac, u0_, P_, **kw)

    # one start shared by every system
    shared = run(u0[0], P[:7], maxiters=W.MAXITERS)
    _check(shared, ref(u0[0], P[:7], maxiters=W.MAXITERS))
    # device tensors in, device tensors out
    sol = run(torch.tensor(u0, device=dev), torch.tensor(P, device=dev), maxiters=W.MAXITERS)
    assert sol.u.is_cuda and sol.resid.is_cuda and sol.u.dtype == torch.float64
    W.check_against_oracle(sol.u.cpu().numpy(), sol.resid.cpu().numpy(), sol.retcode_raw, sol.iters, W.oracle("rough", 9))
    # maxiters = 1: one trial point, MaxIters
    one = run(u0[:6], P[:6], maxiters=1)
    assert (one.retcode == "MaxIters").all() and (one.iters == 1).all()
    _check(one, ref(u0[:6], P[:6], maxiters=1), min_same=1.0)
    # a start at the root: Success before the first step, the start returned
    roots = W.oracle("rough", 9)[0][:6]
    at_root = run(roots, P[:6], maxiters=W.MAXITERS)
    assert (at_root.retcode == "Success").all() and (at_root.iters == 0).all() and np.array_equal(at_root.u, roots)
    # a NaN parameter in one system: it never terminates, and its neighbours do not notice
    Pn = P[:5].copy()
    Pn[2, 0] = np.nan
    nan = run(u0[:5], Pn, maxiters=7)
    assert nan.retcode[2] == "MaxIters" and nan.iters[2] == 7
    _check(nan, ref(u0[:5], Pn, maxiters=7), min_same=1.0)
    clean = ref(u0[:5], P[:5], maxiters=7)
    keep = [0, 1, 3, 4]
    assert np.array_equal(nan.retcode_raw[keep], clean[2][keep]) and np.array_equal(nan.iters[keep], clean[3][keep])


@pytest.mark.parametrize("n", W.F32_NS)
def test_float32(nls, n):
    """Float32 `rough`: the retcodes of ensemble_f32.simple_trust_region_f32 (all Success); u within 1e-4 relative of the Float64
    wavefront result; and the restatement's step count at least as often as the per-thread Float32 kernel has it, less 0.03
    (four systems of 130, for ties that split differently under column pivoting)"""
    rco, ito = W.f32_reference(n)
    wave, thread = _solve(nls, "rough", n, f32=True), _solve(nls, "rough", n, f32=True, per_wavefront=False)
    assert (wave.kernel, thread.kernel) == (WAVE, THREAD) and wave.u.dtype == np.float32
    u64 = _solve(nls, "rough", n).u
    rel = np.max(np.abs(wave.u.astype(float) - u64), axis=1) / np.max(np.abs(u64), axis=1)
    share_wave, share_thread = float((wave.iters == ito).mean()), float((thread.iters == ito).mean())
    print(f"n = {n}: max relative |u32 - u64| = {rel.max():.2e}; step-count share wave {share_wave:.4f}, "
          f"per thread {share_thread:.4f}; retcodes differing: wave {(wave.retcode_raw != rco).sum()}, "
          f"per thread {(thread.retcode_raw != rco).sum()}")
    assert np.array_equal(wave.retcode_raw, rco) and (rco == R.SUCCESS).all()
    assert rel.max() < 1e-4
    assert share_wave >= share_thread - 0.03
    assert float(np.max(np.abs(wave.resid))) <= 2.8909994e-6     # eps(Float32)^(4/5)


def test_dispatch(nls):
    tr, nr = nls.SimpleTrustRegion(), nls.SimpleNewtonRaphson()

    def prob(n, nb=8):
        P, u0 = W.inputs(n, nb=nb)
        return nls.ImmutableNonlinearProblem(W.DENSE_COUPLED, np.abs(u0) + 0.5, P)

    assert nls.vectorized_solve(prob(4), tr).kernel == THREAD
    with pytest.raises(ValueError):
        nls.vectorized_solve(prob(8), tr, per_wavefront=True)
    assert nls.vectorized_solve(prob(16), tr, per_wavefront=True).kernel == WAVE
    assert nls.vectorized_solve(prob(16), nr).kernel == "nk_batch_newton_wave"
    assert nls.vectorized_solve(prob(16), nr, per_wavefront=False).kernel == "nk_batch_newton"
    assert nls.vectorized_solve(prob(16), nls.SimpleKlement(), maxiters=5).kernel == "nk_batch_klement"
