"""Pins tests/lbroyden_reference.py, the sequential restatement of LimitedMemoryBroyden the GPU tests compare with: the step
counts and reset steps of the Quadratic cases, the α rule, the wrap of the column index, the ConvergenceFailure exit, and the
float64 ↔ long-double distance per step that the GPU bounds are made from. No GPU needed."""
import numpy as np
import pytest

import lbroyden_reference as R


def test_the_python_class_and_the_enum_exist():
    import nonlinearsolve_jl_amd as nls
    from nonlinearsolve_jl_amd import _lib as L
    alg = nls.LimitedMemoryBroyden()
    assert (alg.max_resets, alg.threshold, alg.reset_tolerance, alg.alpha) == (3, 10, None, None)
    assert L.ALG_LIMITED_MEMORY_BROYDEN == 5 and L.RET_NAMES[10] == "ConvergenceFailure"
    with pytest.raises(NotImplementedError, match="line search"):
        nls.LimitedMemoryBroyden(linesearch=nls.BackTracking())
    hdr = open(L.CSRC + "/../../include/mi355x_nk.h").read()
    assert "NK_ALG_LIMITED_MEMORY_BROYDEN = 5" in hdr and "NK_RET_CONVERGENCE_FAILURE = 10" in hdr


@pytest.mark.parametrize("name,steps,resets,cols", [
    ("quadratic64_t10", 6, [], [0, 1, 2, 3, 4]),
    ("quadratic64_t3", 11, [], [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]),          # the column index wraps
    ("quadratic1000_spread", 15, [14], list(range(10)) + [0, 1, 2, 0]),   # wraps, then restarts at column 0 after the reset
    ("quadratic4099_spread", 15, [14], list(range(10)) + [0, 1, 2, 0]),   # the same at five workgroups
])
def test_quadratic_step_counts_and_reset_steps(name, steps, resets, cols):
    r = R.run(name)
    assert (r.retcode, r.nsteps, r.reset_steps, r.cols) == (R.SUCCESS, steps, resets, cols)
    assert float(np.max(np.abs(r.fu))) <= R.ABSTOL and float(np.max(np.abs(r.u - np.sqrt(2.0)))) < 1e-12


def test_the_issue_s_start_linspace_1_3_resets_on_a_narrow_margin():
    """n = 1000, u0 = linspace(1, 3): 12 steps with ONE reset, at step 11 — decided by a min|δu_i| within a factor 2.1 of the
    tolerance, which is why the shared case starts from linspace(1, 2.375) instead."""
    r = R.solve(R.quadratic(2.0), np.linspace(1.0, 3.0, 1000))
    assert (r.retcode, r.nsteps, r.reset_steps) == (R.SUCCESS, 12, [11])
    assert min(m[1] for m in r.margins if m[0] <= 11) < 4.0


def test_no_reset_decision_of_a_shared_case_hangs_on_a_rounding():
    """The flag any(|x_i| ≤ tol) is min|x_i| ≤ tol: entries near the tolerance do not matter while a smaller one holds the flag
    (with 1000 spread components some entry is always near it), so a flag is `firm` when min|x_i| is a factor 4 away from the
    tolerance, or exactly 0. A case that resets: every flag of every reset test up to the last reset is firm. A case that
    does not: a reset needs three flagged tests in a row, and there are never three in a row that are flagged or not firm."""
    for name in R.CASES:
        r = R.run(name)
        if r.reset_steps:
            for step, mdu, mdfu, _fdu, _fdfu in r.margins:
                if step <= r.reset_steps[-1]:
                    assert mdu >= 4.0 and (mdfu is None or mdfu >= 4.0), (name, step, mdu, mdfu)
        else:
            streak = 0
            for step, mdu, mdfu, fdu, fdfu in r.margins:
                streak = streak + 1 if (fdu or mdu < 4.0 or fdfu or mdfu < 4.0) else 0
                assert streak < 3, (name, step)


def test_alpha_rule():
    u, fu = np.full(9, 2.0), np.full(9, 0.5)
    assert R.initial_alpha(None, u, fu) == (2.0 * 1.5) / 6.0            # 2‖fu‖₂ / max(‖u‖₂, 1)
    assert R.initial_alpha(None, np.full(4, 0.1), np.full(4, 0.5)) == 2.0 * 1.0 / 1.0     # ‖u‖₂ = 0.2 < 1
    assert R.initial_alpha(None, u, np.full(9, 1.0e-6)) == 1.0          # ‖fu‖₂ = 3e-6 < 1e-5
    assert R.initial_alpha(None, u, np.full(9, 1.0e-5)) != 1.0          # ‖fu‖₂ = 3e-5
    assert R.initial_alpha(2.5, u, fu) == 2.5
    r = R.run("quadratic64_t10")
    assert r.alphas == [(1, 8.0 / 16.0)]                                 # a = 1/α = max(‖u0‖, 1)/(2‖fu0‖) = 8/(2·8)
    r = R.run("quadratic1000_spread")
    assert [s for s, _a in r.alphas] == [1, 14]                          # recomputed by the reset, from the current (u, fu)
    assert r.alphas[1][1] == 1.0                                         # ‖fu‖₂ < 1e-5 there: α = 1
    assert R.run("quadratic64_alpha_t1").alphas == [(1, 1.0 / 2.5)]


def test_low_rank_operator_and_wrap():
    rng = np.random.default_rng(0)
    J = R.LowRank(7, 3, np.float64)
    J.a = 0.75
    dense = 0.75 * np.eye(7)
    pairs = []
    for k in range(5):
        ucol, vcol = rng.standard_normal(7), rng.standard_normal(7)
        col = J.rank1(ucol, vcol)
        assert col == k % 3 and J.idx == k + 1
        pairs.append((ucol, vcol))
        live = pairs[-3:]                          # after `threshold` updates the oldest pair is overwritten, nothing else
        dense = 0.75 * np.eye(7) + sum(np.outer(a, b) for a, b in live)
        x = rng.standard_normal(7)
        assert np.allclose(J.mul(x), dense @ x, rtol=1e-13, atol=1e-13)
        assert np.allclose(J.tmul(x), dense.T @ x, rtol=1e-13, atol=1e-13)
    assert J.ncols() == 3


def test_reset_condition_counters():
    tol = R.RESET_TOL
    big, small = np.array([1.0, 2.0]), np.array([1.0, tol / 2])
    c = R.NoChangeInStateReset(np.zeros(2), tol)
    # dfu alone never reaches a reset: a `du` flag that is false zeroes both counters at every call
    for k in range(6):
        assert not c(np.zeros(2), big) and (c.since_du, c.since_dfu) == (0, 1)
    # du flagged three times in a row (dfu flagged as well, or the dfu branch would zero the du counter)
    c = R.NoChangeInStateReset(np.zeros(2), tol)
    assert not c(np.zeros(2), small) and not c(np.zeros(2), small)
    ref_before = c.ref.copy()
    assert c(np.ones(2), small) and (c.since_du, c.since_dfu) == (0, 0)
    assert np.array_equal(c.ref, ref_before)          # the early return skipped the dfu bookkeeping of that call
    # du flagged, dfu not: the dfu branch's else zeroes the du counter again
    c = R.NoChangeInStateReset(np.zeros(2), tol)
    for k in range(5):
        assert not c(np.full(2, float(k + 1)), small) and (c.since_du, c.since_dfu) == (0, 0)


def test_convergence_failure_on_the_constructed_stall():
    r = R.run("stall64")
    assert (r.retcode, r.nsteps, r.nresets, r.reset_steps) == (R.CONVERGENCE_FAILURE, 10, 3, [4, 7, 10])
    assert len(r.us) == 9                              # the third reset is never applied: step 10 moves nothing
    assert [s for s, _a in r.alphas] == [1, 4, 7]
    # one constant non-zero component alone does not stall the solve into resets
    def one_constant(u):
        f = u * u - 2.0
        f[-1] = 1.0
        return f
    q = R.solve(one_constant, np.ones(64), maxiters=40)
    assert q.reset_steps == []
    assert R.solve(R.stall(2.0), np.ones(64), max_resets=2).nsteps == 7


def test_threshold_is_clamped_to_maxiters():
    r = R.run("quadratic64_clamped")
    assert (r.retcode, r.nsteps, r.cols) == (R.MAXITERS, 4, [0, 1, 2, 3])


def test_bratu_diverges_without_a_line_search():
    """what the method does NOT do (DESIGN): the project's Bratu problem from u0 = 0 ends Unstable, or in ConvergenceFailure"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = {(ns, th): R.solve(R.bratu(ns), np.zeros(ns * ns), threshold=th) for ns in (8, 16) for th in (3, 10, 30)}
    # (the trajectories are chaotic: the step counts — 5 to 100 here — move with the last bit of exp; the outcome does not)
    assert all(v.retcode in (R.UNSTABLE, R.CONVERGENCE_FAILURE) and v.nsteps <= 200 for v in got.values()), \
        {k: (v.retcode, v.nsteps) for k, v in got.items()}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float64_against_long_double_gap_per_step(name):
    """the gap is the algorithm's sensitivity to rounding on that case and step; the GPU bound is 16 × gap + a floor"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here")
    gaps, bnds, ref = R.gaps(name), R.bounds(name), R.run(name)
    assert len(gaps) == len(ref.us) == len(bnds) > 0
    scale = max(1.0, max(float(np.max(np.abs(u))) for u in ref.us))
    for k, ((gu, gf), (bu, bf)) in enumerate(zip(gaps, bnds), start=1):
        print(f"{name} step {k}: gap u {gu:.3e} fu {gf:.3e}   bound u {bu:.3e} fu {bf:.3e}")
        assert bu >= 16.0 * gu and bf >= 16.0 * gf and bu > 0.0 and bf > 0.0
        assert bu - 16.0 * gu <= 4.0 * R.EPS * scale * (1 + 1e-12)       # the floor is a few eps·‖u‖∞, no more
