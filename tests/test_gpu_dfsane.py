"""DFSane on the device (csrc/nk_qn.hip, nk_solver.hip: sane_step) against the sequential restatement
tests/dfsane_reference.py: u and fu after EVERY step, and through the getter the trials of each line search, the signed α, σ
and the merit history. The per-step bounds come from the restatement's own float64 ↔ long-double distance
(dfsane_reference.bounds / scalar_bounds), never from the device's output."""
import numpy as np
import pytest

import dfsane_reference as R

pytestmark = pytest.mark.gpu


def _problem(nls, name, dev):
    """the device twin of a restatement case: (NonlinearProblem, keyword arguments of the algorithm, steps compared)"""
    import torch
    _f, u0, kw, upto = R.CASES[name]
    u0t = torch.tensor(u0, dtype=torch.float64, device=dev)
    if name.startswith("quadratic"):
        prob = nls.NonlinearProblem(nls.Quadratic(len(u0), 2.0), u0t)
    elif name.startswith("bratu"):
        prob = nls.NonlinearProblem(nls.Bratu2D(int(round(len(u0) ** 0.5)), 6.0), u0t)
    else:   # root_domain: a device callback that supplies f and nothing else, and returns NaN outside u ≥ 0
        def f(du, u, p):
            torch.sqrt(u, out=du)
            du[0::2] += 1.0
            du[1::2] -= 3.0
        prob = nls.NonlinearProblem(nls.NonlinearFunction(f), u0t)
    return prob, dict(kw), upto


def _run(nls, name, dev, cache=None):
    """steps the cache until it stops (or the case's step count); returns (cache, [u], [fu], [getter state] after each step)"""
    prob, kw, upto = _problem(nls, name, dev)
    if cache is None:
        cache = nls.init(prob, nls.DFSane(**kw), abstol=R.ABSTOL)
    us, fus, states = [], [], []
    while not cache.force_stop and (upto is None or cache.nsteps < upto):
        nls.step_(cache)
        states.append(cache.dfsane_state)
        if cache.retcode != "InternalLineSearchFailed":
            us.append(cache.u.cpu().numpy())
            fus.append(cache.fu.cpu().numpy())
    return cache, us, fus, states


def _assert_parity(name, us, fus, states):
    ref, bnd, sbnd = R.run(name), R.bounds(name), R.scalar_bounds(name)
    assert len(us) == len(ref.us), (len(us), len(ref.us))
    assert [s["trials"] for s in states] == ref.trials
    total = 0
    for k, (u, fu, st, ur, fr, (bu, bf), (bs, ba, bh)) in enumerate(zip(us, fus, states, ref.us, ref.fus, bnd, sbnd), start=1):
        eu, ef = float(np.max(np.abs(u - ur))), float(np.max(np.abs(fu - fr)))
        es, ea = abs(st["sigma"] - float(ref.sigmas[k - 1])), abs(st["alpha"] - float(ref.alphas[k - 1]))
        eh = np.abs(np.array(st["history"]) - np.asarray(ref.histories[k - 1], np.float64))
        print(f"{name} step {k}: |du| {eu:.3e} (bound {bu:.3e})  |dfu| {ef:.3e} (bound {bf:.3e})  |dsigma| {es:.3e} (bound {bs:.3e})  "
              f"|dalpha| {ea:.3e} (bound {ba:.3e})  max |dhist|/bound {float(np.max(eh / bh)):.3e}")
        assert eu <= bu and ef <= bf, (name, k, eu, bu, ef, bf)
        assert es <= bs and ea <= ba and np.all(eh <= bh), (name, k, es, bs, ea, ba, eh, bh)
        total += ref.trials[k - 1]
        assert st["total_trials"] == total and st["M"] == len(ref.histories[k - 1])


SMALL = ["quadratic1", "quadratic2", "quadratic63", "quadratic257", "quadratic1000_spread", "quadratic4099_spread"]
OPTIONS = ["quadratic64", "quadratic64_M3", "quadratic64_nexp1", "quadratic64_sigma1", "quadratic64_smin", "bratu16_g2"]


@pytest.mark.parametrize("name", SMALL + OPTIONS)
def test_parity_every_step(nls, dev, name):
    cache, us, fus, states = _run(nls, name, dev)
    ref = R.run(name)
    assert (cache.retcode if cache.force_stop else None, cache.nsteps) == (ref.retcode, ref.nsteps)
    _assert_parity(name, us, fus, states)
    st = cache.stats
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (ref.nf, 0, 0, 0, 0, 0)
    cache.close()


@pytest.mark.parametrize("name", ["quadratic65539", "quadratic262145"])
def test_large_sizes_and_bitwise_repeatability(nls, dev, name):
    import torch
    ref = R.run(name)
    cache, us, fus, states = _run(nls, name, dev)
    assert (cache.retcode, cache.nsteps) == (ref.retcode, ref.nsteps)
    _assert_parity(name, us, fus, states)
    outs = [(cache.u.clone(), cache.fu.clone())]
    cache.close()
    for _ in range(2):
        prob, kw, _upto = _problem(nls, name, dev)
        sol = nls.solve(prob, nls.DFSane(**kw), abstol=R.ABSTOL)
        assert (sol.retcode, sol.stats.nsteps, sol.stats.nf) == (ref.retcode, ref.nsteps, ref.nf)
        outs.append((sol.u, sol.resid))
    for u, fu in outs[1:]:
        assert torch.equal(outs[0][0], u) and torch.equal(outs[0][1], fu)


def test_nan_trials_end_in_internal_line_search_failed(nls, dev):
    name = "root_domain_nan"
    ref = R.run(name)
    assert (ref.retcode, ref.nf) == (R.LINESEARCH_FAILED, 7)
    cache, us, fus, states = _run(nls, name, dev)
    assert (cache.retcode, cache.nsteps, cache.force_stop, us) == ("InternalLineSearchFailed", 1, True, [])
    assert states[0]["trials"] == 7 and np.isnan(states[0]["alpha"]) and states[0]["sigma"] == 1.0
    st = cache.stats
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (ref.nf, 0, 0, 0, 0, 0)
    assert np.array_equal(cache.u.cpu().numpy(), ref.u)      # nothing moved; fu is f(u0) (sqrt: the device's, a rounding apart at most)
    assert np.allclose(cache.fu.cpu().numpy(), ref.fu, rtol=4 * R.EPS, atol=0)
    cache.close()
    prob, kw, _upto = _problem(nls, name, dev)
    sol = nls.solve(prob, nls.DFSane(**kw), abstol=R.ABSTOL)
    assert sol.retcode == "InternalLineSearchFailed" and not sol.successful_retcode and sol.stats.nf == 7


def test_reinit_repeats_the_trajectory(nls, dev):
    import torch
    name = "quadratic1000_spread"
    cache, us, fus, states = _run(nls, name, dev)
    other = torch.full((1000,), 1.5, dtype=torch.float64, device=dev)
    nls.reinit_(cache, other)
    st = cache.dfsane_state
    # σ = ⟨u,u⟩/⟨u,f⟩ = 1.5/0.25 and the history M × ‖f‖₂² = 1000·0.25², from the NEW start
    assert abs(st["sigma"] - 6.0) <= 64 * R.EPS * 6.0 and (st["alpha"], st["trials"], st["total_trials"]) == (0.0, 0, 0)
    assert np.allclose(st["history"], [62.5] * 10, rtol=64 * R.EPS, atol=0) and cache.nsteps == 0
    nls.step_(cache)
    nls.step_(cache)
    u0 = torch.tensor(R.spread_start(1000), dtype=torch.float64, device=dev)
    nls.reinit_(cache, u0)
    _c, us2, fus2, states2 = _run(nls, name, dev, cache=cache)
    assert states2 == states and len(us2) == len(us)
    for a, b, c, d in zip(us, us2, fus, fus2):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    cache.close()


def test_trace_and_ignored_recompute_jacobian(nls, dev):
    prob, kw, _upto = _problem(nls, "quadratic64", dev)
    cache = nls.init(prob, nls.DFSane(**kw), abstol=R.ABSTOL, store_trace=True)
    nls.step_(cache, recompute_jacobian=False)       # ignored: the method has no Jacobian (the reference only warns)
    assert cache.nsteps == 1 and cache.dfsane_state["trials"] == 3
    sol = nls.solve_(cache)
    assert sol.retcode == "Success" and sol.stats.nsteps == 8
    assert [r["iter"] for r in sol.trace] == list(range(1, 9)) and sol.trace[-1]["fnorm_inf"] <= R.ABSTOL
    assert not nls.supports_deferred_residual(cache)
    cache.close()


def test_arguments_outside_the_supported_range(nls, dev):
    prob, _kw, _upto = _problem(nls, "quadratic64", dev)
    with pytest.raises(nls.NKError, match="M = 33"):
        nls.init(prob, nls.DFSane(M=33))
    with pytest.raises(nls.NKError, match="n_exp"):
        nls.init(prob, nls.DFSane(n_exp=3))
    alg = nls.DFSane()
    alg.linesearch = nls.BackTracking()              # what a caller of the C ABI would set in nk_options.linesearch
    with pytest.raises(nls.NKError, match="line search"):
        nls.init(prob, alg)
    alg = nls.DFSane()
    alg.forcing = nls.EisenstatWalkerForcing2()
    with pytest.raises(nls.NKError, match="forcing"):
        nls.init(prob, alg)
    cache = nls.init(prob, nls.LimitedMemoryBroyden())
    with pytest.raises(nls.NKError, match="DFSane"):
        cache.dfsane_state
    cache.close()
