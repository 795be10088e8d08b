"""Klement on the device (csrc/nk_qn.hip: k_kl_step, one fused launch per step besides the residual) against the sequential
restatement tests/broyden_reference.py: u and fu after every step, retcode, step count, reset steps, reset count."""
import numpy as np
import pytest

import broyden_reference as R
import qn_device_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["klement64", "klement65", "klement1000", "klement4099", "klement64_alpha"])
def test_parity_every_step(nls, dev, name):
    cache, us, fus, resets = D.run(nls, name, dev)
    D.assert_control_flow(name, cache, resets)
    D.assert_parity(name, us, fus)
    ref = R.run(name)
    a = cache.qn_state["a"]   # Klement's J is not inverted: the scaling is α itself
    assert abs(a - float(ref.alphas[-1][1])) <= 4 * R.EPS * a
    if name == "klement64_alpha":
        assert a == 2.8
    st = cache.stats
    assert (st.nf, st.njacs, st.nfactors, st.nsolve, st.gmres_iters, st.op_applies) == (ref.nsteps, 0, 0, 0, 0, 0)
    J = cache.broyden_inverse().cpu().numpy()
    assert J.shape == (len(ref.u),) and np.all(np.isfinite(J))
    cache.close()


def test_a_zero_in_j_asks_for_a_reset_every_step(nls, dev):
    """alpha = 1 and a component with constant residual 1: its J is 1 + ((0 − 1·(−1))/1)·(−1)·1 = 0 after every update"""
    name = "klement_reset64"
    ref = R.run(name)
    assert (ref.retcode, ref.nsteps, ref.reset_steps, ref.nresets) == (R.CONVERGENCE_FAILURE, 4, [2, 3, 4], 3)
    cache, us, fus, resets = D.run(nls, name, dev)
    assert (cache.retcode, cache.nsteps, cache.force_stop) == ("ConvergenceFailure", 4, True)
    D.assert_control_flow(name, cache, resets)
    D.assert_parity(name, us, fus)
    assert cache.broyden_inverse().cpu().numpy()[-1] == 0.0 and cache.stats.nf == 3
    cache.close()


def test_reinit_repeats_the_trajectory(nls, dev):
    import torch
    name = "klement1000"
    cache, us, fus, resets = D.run(nls, name, dev)
    nls.reinit_(cache, torch.tensor(R.CASES[name][1], dtype=torch.float64, device=dev))
    assert cache.nsteps == 0 and cache.qn_state["nresets"] == 0
    _c, us2, fus2, resets2 = D.run(nls, name, dev, cache=cache)
    assert resets2 == resets and len(us2) == len(us)
    for a, b, c, e in zip(us, us2, fus, fus2):
        assert np.array_equal(a, b) and np.array_equal(c, e)
    cache.close()


def test_what_is_not_built_is_refused(nls, dev):
    prob, _alg, _m = D.problem(nls, "klement64", dev)
    for ij in ("true_jacobian", "true_jacobian_diagonal"):
        with pytest.raises(nls.NKError, match=r"status -5: .*true_jacobian"):
            nls.init(prob, nls.Klement(init_jacobian=ij))
    with pytest.raises(nls.NKError, match=r"status -1: .*line-search"):
        nls.init(prob, nls.Klement(linesearch=nls.BackTracking()))
