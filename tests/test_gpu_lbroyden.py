"""LimitedMemoryBroyden on the device (csrc/nk_qn.hip, nk_solver.hip: lb_step) against the sequential restatement
tests/lbroyden_reference.py: u and fu after EVERY step, the step at which a reset happens, the retcodes, the reset count.
The per-step bounds come from the restatement's own float64 ↔ long-double distance (lbroyden_reference.bounds), never from
the device's output."""
import numpy as np
import pytest

import lbroyden_reference as R

pytestmark = pytest.mark.gpu


def _problem(nls, name, dev):
    """the device twin of a restatement case: (NonlinearProblem, keyword arguments of the algorithm, maxiters)"""
    import torch
    _f, u0, kw, _upto = R.CASES[name]
    kw = dict(kw)
    maxiters = kw.pop("maxiters", 1000)
    u0t = torch.tensor(u0, dtype=torch.float64, device=dev)
    if name.startswith("quadratic"):
        prob = nls.NonlinearProblem(nls.Quadratic(len(u0), 2.0), u0t)
    elif name.startswith("bratu"):
        prob = nls.NonlinearProblem(nls.Bratu2D(int(round(len(u0) ** 0.5)), 6.0), u0t)
    else:   # the stall: a device callback that supplies f and nothing else
        def f(du, u, p):
            torch.mul(u, u, out=du)
            du.sub_(2.0)
            du[-1] = 1.0
            du[-2] = 0.0
        prob = nls.NonlinearProblem(nls.NonlinearFunction(f), u0t)
    return prob, kw, maxiters


def _run(nls, name, dev, steps=None, u0=None, cache=None):
    """steps the cache until it stops; returns (cache, [u after each step that moved], [fu], [nresets after each step])"""
    prob, kw, maxiters = _problem(nls, name, dev)
    if cache is None:
        cache = nls.init(prob, nls.LimitedMemoryBroyden(**kw), abstol=R.ABSTOL, maxiters=maxiters)
    us, fus, resets = [], [], []
    while not cache.force_stop and cache.nsteps < maxiters and (steps is None or cache.nsteps < steps):
        nls.step_(cache)
        resets.append(cache.lbroyden_state["nresets"])
        if cache.retcode != "ConvergenceFailure":
            us.append(cache.u.cpu().numpy())
            fus.append(cache.fu.cpu().numpy())
    return cache, us, fus, resets


def _assert_parity(name, us, fus):
    ref, bnd = R.run(name), R.bounds(name)
    assert len(us) == len(ref.us), (len(us), len(ref.us))
    for k, (u, fu, ur, fr, (bu, bf)) in enumerate(zip(us, fus, ref.us, ref.fus, bnd), start=1):
        eu, ef = float(np.max(np.abs(u - ur))), float(np.max(np.abs(fu - fr)))
        print(f"{name} step {k}: |du| {eu:.3e} (bound {bu:.3e})  |dfu| {ef:.3e} (bound {bf:.3e})")
        assert eu <= bu and ef <= bf, (name, k, eu, bu, ef, bf)


def _reset_steps(resets):
    return [k for k, (a, b) in enumerate(zip([0] + resets[:-1], resets), start=1) if b > a]


@pytest.mark.parametrize("name", ["quadratic64_t10", "quadratic64_t3"])
def test_quadratic_parity_every_step(nls, dev, name):
    cache, us, fus, resets = _run(nls, name, dev)
    ref = R.run(name)
    assert (cache.retcode if cache.force_stop else None, cache.nsteps) == (ref.retcode, ref.nsteps)
    assert resets[-1] == ref.nresets == 0
    _assert_parity(name, us, fus)
    st = cache.lbroyden_state
    assert st["idx"] == len(ref.cols) and st["threshold"] == R.CASES[name][2]["threshold"]
    cache.close()


def _assert_spread_start(nls, dev, name):
    cache, us, fus, resets = _run(nls, name, dev)
    ref = R.run(name)
    assert ref.reset_steps == [14] and ref.nsteps == 15
    assert (cache.retcode, cache.nsteps) == (ref.retcode, ref.nsteps)
    assert _reset_steps(resets) == ref.reset_steps
    _assert_parity(name, us, fus)
    cache.close()


def test_spread_start_resets_where_the_restatement_does(nls, dev):
    _assert_spread_start(nls, dev, "quadratic1000_spread")   # n = 1000: no multiple of the wave or the workgroup


def test_spread_start_at_five_workgroups(nls, dev):
    _assert_spread_start(nls, dev, "quadratic4099_spread")   # five workgroups in every kernel, an odd tail, the reset step included


@pytest.mark.parametrize("name", ["quadratic65539", "quadratic262145"])
def test_large_sizes_and_bitwise_repeatability(nls, dev, name):
    import torch
    ref = R.run(name)
    outs = []
    for _ in range(2):
        prob, kw, maxiters = _problem(nls, name, dev)
        sol = nls.solve(prob, nls.LimitedMemoryBroyden(**kw), abstol=R.ABSTOL, maxiters=maxiters)
        assert (sol.retcode, sol.stats.nsteps) == (ref.retcode, ref.nsteps)
        outs.append((sol.u, sol.resid))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    bu, bf = R.bounds(name)[-1]
    eu = float(np.max(np.abs(outs[0][0].cpu().numpy() - ref.u)))
    ef = float(np.max(np.abs(outs[0][1].cpu().numpy() - ref.fu)))
    print(f"{name}: final |du| {eu:.3e} (bound {bu:.3e}) |dfu| {ef:.3e} (bound {bf:.3e})")
    assert eu <= bu and ef <= bf


def test_bratu_first_six_steps(nls, dev):
    """the non-diagonal check: J⁻ᵀ is not J⁻¹ here, and U and V are not interchangeable"""
    name = "bratu16_t10"
    cache, us, fus, _r = _run(nls, name, dev, steps=6)
    assert cache.nsteps == 6 and not cache.force_stop
    _assert_parity(name, us, fus)
    cache.close()


def test_convergence_failure_through_a_residual_only_callback(nls, dev):
    name = "stall64"
    ref = R.run(name)
    assert (ref.retcode, ref.nsteps, ref.reset_steps) == (R.CONVERGENCE_FAILURE, 10, [4, 7, 10])
    cache, us, fus, resets = _run(nls, name, dev)
    assert (cache.retcode, cache.nsteps, cache.force_stop) == ("ConvergenceFailure", 10, True)
    assert _reset_steps(resets) == ref.reset_steps and cache.lbroyden_state["nresets"] == 3
    _assert_parity(name, us, fus)
    st = cache.stats
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (9, 0, 0, 0, 0, 0)
    cache.close()
    prob, kw, maxiters = _problem(nls, name, dev)
    sol = nls.solve(prob, nls.LimitedMemoryBroyden(**kw), abstol=R.ABSTOL)
    assert sol.retcode == "ConvergenceFailure" and not sol.successful_retcode


@pytest.mark.parametrize("name", ["quadratic64_alpha_t1", "quadratic64_clamped"])
def test_alpha_given_threshold_one_and_clamped(nls, dev, name):
    cache, us, fus, _r = _run(nls, name, dev)
    ref = R.run(name)
    _assert_parity(name, us, fus)
    st = cache.lbroyden_state
    assert st["a"] == 1.0 / 2.5
    if name == "quadratic64_clamped":   # threshold 32 > maxiters 4: clamped (initialization.jl:180)
        assert st["threshold"] == 4 and cache.nsteps == 4 and not cache.force_stop
        assert nls.solve_(cache).retcode == "MaxIters"
    else:
        assert st["threshold"] == 1 and (cache.retcode, cache.nsteps) == (ref.retcode, ref.nsteps)
    cache.close()


def test_reinit_repeats_the_trajectory(nls, dev):
    import torch
    name = "quadratic1000_spread"
    cache, us, fus, resets = _run(nls, name, dev)
    assert cache.lbroyden_state["nresets"] == 1
    other = torch.full((1000,), 1.5, dtype=torch.float64, device=dev)
    nls.reinit_(cache, other)
    st = cache.lbroyden_state
    assert (st["nresets"], st["idx"], st["since_du"], st["since_dfu"]) == (0, 0, 0, 0) and cache.nsteps == 0
    nls.step_(cache)
    a_other = cache.lbroyden_state["a"]
    fu0 = 1.5 * 1.5 - 2.0   # a = max(‖u0‖, 1)/(2‖fu0‖) from the NEW start, not the first run's
    assert abs(a_other - (1.5 * 1000 ** 0.5) / (2.0 * abs(fu0) * 1000 ** 0.5)) <= 4 * R.EPS * a_other
    nls.solve_(cache)
    u0 = torch.tensor(R.spread_start(1000), dtype=torch.float64, device=dev)
    nls.reinit_(cache, u0)
    _c, us2, fus2, resets2 = _run(nls, name, dev, cache=cache)
    assert resets2 == resets and len(us2) == len(us)
    for a, b, c, d in zip(us, us2, fus, fus2):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    cache.close()


def test_nothing_but_the_residual_ran(nls, dev):
    prob, kw, maxiters = _problem(nls, "quadratic64_t10", dev)
    cache = nls.init(prob, nls.LimitedMemoryBroyden(**kw), abstol=R.ABSTOL, store_trace=True)
    sol = nls.solve_(cache)
    st = sol.stats
    assert sol.retcode == "Success" and st.nsteps == 6
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (6, 0, 0, 0, 0, 0)
    assert [r["iter"] for r in sol.trace] == list(range(1, 7)) and sol.trace[-1]["fnorm_inf"] <= R.ABSTOL
    assert not nls.supports_deferred_residual(cache)
    cache.close()


def test_arguments_outside_the_supported_range(nls, dev):
    prob, _kw, _m = _problem(nls, "quadratic64_t10", dev)
    with pytest.raises(nls.NKError, match="threshold"):
        nls.init(prob, nls.LimitedMemoryBroyden(threshold=33))
    cache = nls.init(prob, nls.LimitedMemoryBroyden())
    nls.step_(cache)
    with pytest.raises(nls.NKError, match="recompute_jacobian"):
        nls.step_(cache, recompute_jacobian=False)
    cache.close()
