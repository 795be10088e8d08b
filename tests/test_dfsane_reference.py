"""Pins tests/dfsane_reference.py, the sequential restatement of DFSane the GPU tests compare with: the case list and what each
case exercises, the two conditions on it (float64 and long double take the same decisions; every decision has a relative margin
of at least 2⁻²⁰), agreement with the SimpleDFSane restatement, and the float64 ↔ long-double distance per step that the GPU
bounds are made from. No GPU needed."""
import numpy as np
import pytest

import dfsane_reference as R
import simple_jf_reference as SJ


def test_the_python_class_and_the_enum_exist():
    import nonlinearsolve_jl_amd as nls
    from nonlinearsolve_jl_amd import _lib as L
    alg = nls.DFSane()
    assert (alg.sigma_min, alg.sigma_max, alg.sigma_1, alg.M, alg.gamma, alg.tau_min, alg.tau_max, alg.n_exp,
            alg.max_inner_iterations) == (1e-10, 1e10, None, 10, 1e-4, 0.1, 0.5, 2, 100)
    assert L.ALG_DFSANE == 6 and L.RET_NAMES[9] == "InternalLineSearchFailed"
    with pytest.raises(NotImplementedError, match="eta_strategy"):
        nls.DFSane(eta_strategy=lambda f1, k, x, fx: f1 / k)
    hdr = open(L.CSRC + "/../../include/mi355x_nk.h").read()
    assert "NK_ALG_DFSANE = 6" in hdr and "nk_solver_get_dfsane_state" in hdr
    o = L.Options()
    L.check(L.lib().nk_options_default(o))
    assert (o.sane_sigma_min, o.sane_sigma_max, o.sane_sigma_1, o.sane_M, o.sane_gamma, o.sane_tau_min, o.sane_tau_max,
            o.sane_n_exp, o.sane_max_inner_iterations) == (1e-10, 1e10, 0.0, 10, 1e-4, 0.1, 0.5, 2, 100)


def test_case_list():
    assert sorted(R.CASES) == sorted([
        "quadratic64", "quadratic64_M3", "quadratic64_nexp1", "quadratic64_sigma1", "quadratic64_smin", "quadratic1000_spread",
        "quadratic4099_spread",
        "bratu16_g2", "quadratic1", "quadratic2", "quadratic63", "quadratic257", "quadratic65539", "quadratic262145",
        "root_domain_nan"])


def _kinds(r, step=None):
    return {(k, out) for s, k, out, _m in r.decisions if step is None or s == step}


def test_what_the_cases_exercise():
    # a step accepted at the first trial; a first step that needs three trials (α_t = 0.2 lies between the clamps)
    r = R.run("quadratic64")
    assert (r.retcode, r.nsteps, r.nf, r.trials) == (R.SUCCESS, 8, 10, [3, 1, 1, 1, 1, 1, 1, 1])
    assert float(r.sigma0) == -1.0 and [float(a) for a in r.alphas] == [0.2] + [1.0] * 7
    assert float(np.max(np.abs(r.u - np.sqrt(2.0)))) < 1e-12
    # accepted on the minus side (steps 3 and 4), a clamp at τ_min
    r = R.solve(*R.CASES["quadratic1000_spread"][:2])
    assert (r.retcode, r.nsteps, r.nf) == (R.SUCCESS, 34, 44)
    assert r.trials[:11] == [1, 3, 4, 2, 1, 1, 1, 1, 1, 3, 3]
    assert [float(a) for a in r.alphas[:4]] == [1.0, 0.1, -0.1, -1.0]
    assert ("accept-", True) in _kinds(r, 3) and ("accept-", True) in _kinds(r, 4) and ("clamp+<lo", True) in _kinds(r, 2)
    assert R.run("quadratic1000_spread").trials == r.trials[:6]
    # accepted at the third plus trial after a clamp at τ_min and one at τ_max: α = 1 → 0.3 → 0.15 (step 11); σ replaced at the
    # start, where ⟨u,u⟩/⟨u,f⟩ = 0/0
    r = R.run("bratu16_g2")
    assert r.nsteps == 12 and r.retcode is None and r.trials == [3, 5, 3, 7, 3, 5, 5, 3, 3, 7, 5, 3]
    assert r.sigma_replaced == [0] and float(r.sigma0) == float(R.jl_clamp(1.0 / np.sqrt(R.seq_dot(r0 := R.bratu(16)(np.zeros(256)), r0)), 1.0, 1e5))
    assert {("clamp+<lo", True), ("clamp+>hi", True), ("accept+", True)} <= _kinds(r, 11)
    assert abs(float(r.alphas[10]) - 0.3 * 0.5) < 1e-15
    # σ replaced by clamp(1/‖f‖₂, 1, 1e5) after a spectral update
    r = R.run("quadratic64_smin")
    assert r.retcode == R.SUCCESS and r.sigma_replaced == [3, 4]
    assert float(r.sigmas[3]) == 1.0 and float(r.sigmas[2]) == float(1.0 / np.sqrt(R.seq_dot(r.fus[2], r.fus[2])))
    # a wrapped history
    r = R.run("quadratic64_M3")
    assert r.nsteps == 8 and len(r.histories[0]) == 3
    for k in range(3, 8):
        assert [float(x) for x in sorted(r.histories[k])] == sorted(float(np.sqrt(R.seq_dot(f, f)) ** 2) for f in r.fus[k - 2:k + 1])
    # n_exp = 1; sigma_1 given
    r = R.run("quadratic64_nexp1")
    assert r.retcode == R.SUCCESS and float(r.histories[0][0]) == float(np.sqrt(R.seq_dot(r.fus[0], r.fus[0])))
    r = R.run("quadratic64_sigma1")
    assert (r.retcode, r.nsteps, r.trials, float(r.sigma0)) == (R.SUCCESS, 5, [1] * 5, 0.4)


def test_nan_trials_run_to_the_cap():
    r = R.run("root_domain_nan")
    assert (r.retcode, r.nsteps, r.nf, r.trials, len(r.us)) == (R.LINESEARCH_FAILED, 1, 7, [7], 0)
    assert np.isnan(float(r.alphas[0])) and all(m == float("inf") and not out for _s, _k, out, m in r.decisions)
    assert np.array_equal(r.u, np.full(64, 0.01))
    assert np.isnan(R.jl_clamp(np.float64(np.nan), 0.1, 0.5))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float64_and_long_double_take_the_same_decisions_with_a_margin(name):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here")
    f, u0, kw, _upto = R.CASES[name]
    upto = 12 if name.startswith("bratu") else None            # the whole solve, not only the steps the device is compared on
    a, b = R.solve(f, u0, np.float64, stop_after=upto, **kw), R.solve(f, u0, np.longdouble, stop_after=upto, **kw)
    assert [d[:3] for d in a.decisions] == [d[:3] for d in b.decisions]
    assert (a.retcode, a.nsteps, a.nf, a.trials) == (b.retcode, b.nsteps, b.nf, b.trials)
    worst = min(a.decisions + b.decisions, key=lambda d: d[3])
    print(name, "decisions", len(a.decisions), "smallest margin", worst)
    assert worst[3] >= 2.0 ** -20, worst


def test_agrees_with_the_simple_dfsane_restatement_bit_for_bit():
    """sigma_1 given, no bound violation, every step accepted at its first trial: the same arithmetic in the same order"""
    r = R.run("quadratic64_sigma1")
    assert r.trials == [1] * r.nsteps and r.sigma_replaced == []
    u0, p = R.CASES["quadratic64_sigma1"][1], np.full(64, 2.0)
    for j in range(1, r.nsteps + 1):
        x, fx, rc, iters, info = SJ.simple_dfsane(SJ.quadratic_f, u0, p, abstol=R.ABSTOL, maxiters=j, sigma_1=0.4)
        assert np.array_equal(x[0], r.us[j - 1]) and np.array_equal(fx[0], r.fus[j - 1]), j
        assert info["inner_passes"][0] == 0
    assert rc[0] == SJ.SUCCESS and iters[0] == r.nsteps


@pytest.mark.parametrize("name", sorted(n for n in R.CASES if n != "root_domain_nan"))
def test_float64_against_long_double_gap_per_step(name):
    """the gap is the algorithm's sensitivity to rounding on that case and step; the GPU bound is 16 × gap + a floor"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here")
    gaps, bnds, sb, ref = R.gaps(name), R.bounds(name), R.scalar_bounds(name), R.run(name)
    assert len(gaps) == len(ref.us) == len(bnds) == len(sb) > 0
    scale = max(1.0, max(float(np.max(np.abs(u))) for u in ref.us))
    for k, ((gu, gf), (bu, bf), (bs, ba, bh)) in enumerate(zip(gaps, bnds, sb), start=1):
        print(f"{name} step {k}: gap u {gu:.3e} fu {gf:.3e}   bound u {bu:.3e} fu {bf:.3e}  sigma {bs:.3e} alpha {ba:.3e}")
        assert bu >= 16.0 * gu and bf >= 16.0 * gf and bu > 0.0 and bf > 0.0 and bs > 0.0 and ba >= 0.0 and np.all(bh > 0.0)
        assert bu - 16.0 * gu <= 4.0 * R.EPS * scale * (1 + 1e-12)       # the floor is a few eps·‖u‖∞, no more
