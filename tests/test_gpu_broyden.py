"""Broyden on the device (csrc/nk_qn.hip: the dense inverse Jacobian's two passes, nk_solver.hip: qn_step) against the sequential
restatement tests/broyden_reference.py: u and fu after EVERY step within the restatement's own float64 ↔ long-double bounds,
retcode, step count, reset steps and reset count wherever a solve ends, and J⁻¹ itself entry by entry."""
import numpy as np
import pytest

import broyden_reference as R
import qn_device_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["broyden64_good", "broyden64_bad", "broyden64_diagonal", "broyden65_good", "broyden1000_good",
                                  "broyden1000_bad", "broyden1000_diagonal", "broyden4099_diagonal", "broyden64_alpha", "broyden64_small_fu"])
def test_parity_every_step(nls, dev, name):
    """n = 64: two row tiles; 65: the odd column tail and the padded ld; 1000: no multiple of wave, workgroup or tile;
    4099: five workgroups in the vector and reduce kernels"""
    cache, us, fus, resets = D.run(nls, name, dev)
    D.assert_control_flow(name, cache, resets)
    D.assert_parity(name, us, fus)
    ref = R.run(name)
    if name == "broyden64_alpha":
        assert cache.qn_state["a"] == 1.0 / 2.5
    if name == "broyden64_small_fu":   # ‖fu‖₂ < 1e-5: α = 1
        assert cache.qn_state["a"] == 1.0 == float(ref.alphas[0][1])
    st = cache.stats
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (ref.nsteps, 0, 0, 0, 0, 0)
    cache.close()


def test_several_row_tiles_and_bitwise_repeatability(nls, dev):
    import torch
    name = "broyden2049_good"   # 65 row tiles, the last one ragged (1 row), an odd n
    ref = R.run(name)
    outs = []
    for _ in range(2):
        prob, alg, maxiters = D.problem(nls, name, dev)
        sol = nls.solve(prob, alg, abstol=R.ABSTOL, maxiters=maxiters)
        assert (sol.retcode, sol.stats.nsteps) == (ref.retcode, ref.nsteps)
        outs.append((sol.u, sol.resid))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    cache, us, fus, resets = D.run(nls, name, dev)
    D.assert_control_flow(name, cache, resets)
    D.assert_parity(name, us, fus)
    assert torch.equal(cache.u, outs[0][0])
    cache.close()


def test_inverse_jacobian_entry_by_entry(nls, dev):
    """one-sided coupling: J⁻¹ is not symmetric, so J⁻¹ taken for J⁻ᵀ, or rows for columns, cannot pass"""
    name = "broyden130_nonsym"
    cache, us, fus, _r = D.run(nls, name, dev)
    assert cache.nsteps == 4 and not cache.force_stop
    D.assert_parity(name, us, fus)
    J, Jr, bound = cache.broyden_inverse().cpu().numpy(), R.run(name).J, R.matrix_bound(name)
    assert J.shape == (130, 130)
    asym = float(np.max(np.abs(Jr - Jr.T)))
    err = np.abs(J - Jr)
    print(f"max|J - Jref| {err.max():.3e}, smallest bound {bound.min():.3e}, max|Jref - Jrefᵀ| {asym:.3e}")
    assert asym > 1e3 * float(bound.max())
    assert np.all(err <= bound), float((err - bound).max())
    cache.close()


def test_bratu_first_six_steps(nls, dev):
    name = "broyden_bratu16"
    cache, us, fus, _r = D.run(nls, name, dev)
    assert cache.nsteps == 6 and not cache.force_stop
    D.assert_parity(name, us, fus)
    cache.close()


def test_third_reset_ends_the_solve_and_is_not_applied(nls, dev):
    name = "broyden_stall64"
    ref = R.run(name)
    assert (ref.retcode, ref.nsteps, ref.reset_steps) == (R.CONVERGENCE_FAILURE, 10, [4, 7, 10])
    cache, us, fus, resets = D.run(nls, name, dev)
    assert (cache.retcode, cache.nsteps, cache.force_stop) == ("ConvergenceFailure", 10, True)
    D.assert_control_flow(name, cache, resets)
    D.assert_parity(name, us, fus)
    st = cache.qn_state
    # the third reset recomputed nothing: a is the second reset's, within the restatement's own gap for that number
    a64, a80 = float(ref.alphas[-1][1]), float(R.run(name, np.longdouble).alphas[-1][1])
    assert st["nresets"] == 3 and len(ref.alphas) == 3 and abs(st["a"] - a64) <= R.MARGIN * abs(a64 - a80) + R.FLOOR_ULPS * R.EPS * a64
    assert cache.stats.nf == 9
    cache.close()


def test_reinit_repeats_the_trajectory_and_the_diagonal_is_readable(nls, dev):
    import torch
    name = "broyden64_diagonal"
    cache, us, fus, resets = D.run(nls, name, dev)
    d = cache.broyden_inverse()
    assert d.shape == (64,) and bool(torch.isfinite(d).all())
    nls.reinit_(cache, torch.tensor(R.CASES[name][1], dtype=torch.float64, device=dev))
    st = cache.qn_state
    assert (st["nresets"], st["since_du"], st["since_dfu"], st["steps_since_reset"]) == (0, 0, 0, 0) and cache.nsteps == 0
    _c, us2, fus2, resets2 = D.run(nls, name, dev, cache=cache)
    assert resets2 == resets and len(us2) == len(us)
    for a, b, c, e in zip(us, us2, fus, fus2):
        assert np.array_equal(a, b) and np.array_equal(c, e)
    cache.close()


def test_what_is_not_built_is_refused(nls, dev):
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    prob, _alg, _m = D.problem(nls, "broyden64_good", dev)
    with pytest.raises(nls.NKError, match=r"status -5: .*true_jacobian"):
        nls.init(prob, nls.Broyden(init_jacobian="true_jacobian"))
    with pytest.raises(nls.NKError, match=r"status -1: .*line-search"):
        nls.init(prob, nls.Broyden(linesearch=nls.BackTracking()))
    n = L.BROYDEN_MAX_N + 1
    big = nls.NonlinearProblem(nls.Quadratic(n, 2.0), torch.ones(n, dtype=torch.float64, device=dev))
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(nls.NKError, match=r"status -5: .*NK_BROYDEN_MAX_N"):
        nls.init(big, nls.Broyden())
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 28)   # nothing of the 8 GiB matrix was allocated
    c = nls.init(big, nls.Broyden(update_rule="diagonal"))    # the diagonal structure has no such cap
    c.close()
    cache = nls.init(prob, nls.Broyden())
    with pytest.raises(nls.NKError, match="first step"):
        cache.broyden_inverse()
    nls.step_(cache)
    with pytest.raises(nls.NKError, match="recompute_jacobian"):
        nls.step_(cache, recompute_jacobian=False)
    cache.close()
