"""The restatement tests/broyden_reference.py on its own (no GPU): the pinned control flow of every case in both arithmetics,
the α rule, the update rules against their textbook secant property, the Klement reset prediction, and the bound rule."""
import numpy as np
import pytest

import broyden_reference as R

PINNED = {
    "broyden64_good": (11, R.SUCCESS, []), "broyden64_bad": (12, R.SUCCESS, []),
    "broyden64_diagonal": (33, R.SUCCESS, [9, 12, 15, 18, 21, 24, 27, 30, 33]), "broyden65_good": (11, R.SUCCESS, []),
    "broyden1000_good": (13, R.SUCCESS, []), "broyden1000_bad": (13, R.SUCCESS, []), "broyden1000_diagonal": (9, R.SUCCESS, [9]),
    "broyden2049_good": (13, R.SUCCESS, []), "broyden4099_diagonal": (8, R.SUCCESS, []), "broyden64_alpha": (7, R.SUCCESS, []), "broyden64_small_fu": (2, R.SUCCESS, []),
    "broyden130_nonsym": (4, None, []), "broyden_bratu16": (6, None, []),
    "broyden_stall64": (10, R.CONVERGENCE_FAILURE, [4, 7, 10]),
    "klement64": (7, R.SUCCESS, []), "klement65": (7, R.SUCCESS, []), "klement1000": (7, R.SUCCESS, []),
    "klement4099": (7, R.SUCCESS, []),
    "klement64_alpha": (6, R.SUCCESS, []), "klement_reset64": (4, R.CONVERGENCE_FAILURE, [2, 3, 4]),
}


def test_every_case_is_pinned():
    assert set(PINNED) == set(R.CASES)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("name", sorted(PINNED))
def test_control_flow_is_the_same_in_both_arithmetics(name):
    for dtype in (np.float64, np.longdouble):
        r = R.run(name, dtype)
        assert (r.nsteps, r.retcode, r.reset_steps) == PINNED[name], (name, dtype)
    closest = [m for row in R.run(name).margins for m in row[1:3] if m is not None and (name, row[0]) not in NARROW]
    assert not closest or min(closest) >= 2.0, min(closest)   # no reset test is decided within a factor 2 of its tolerance


# (case, step): a reset test whose dfu flag is decided within a factor 2 of the tolerance. Every other decision of every case
# keeps the factor 2 above.
NARROW = {("broyden4099_diagonal", 6)}


def test_the_narrow_decision_is_still_out_of_a_rounding_s_reach():
    """broyden4099_diagonal, step 6: min|dfu_i| = 1.0089 tol, flag false; a true flag would start a run of three and reset at
    step 8. The distance to the tolerance, 1.6e-14, is asked to exceed what the bound rule allows a device for the two
    residuals subtracted: MARGIN × the float64 ↔ long-double gap of min|dfu_i| (7.5e-17) plus FLOOR_ULPS eps at the size of
    the numbers rounded in each residual, u² and 2 — 8.3e-15 in all."""
    (name, step), = NARROW
    a, b = R.run(name), R.run(name, np.longdouble)
    ra, rb = ([row for row in r.margins if row[0] == step][0] for r in (a, b))
    assert ra[3:] == rb[3:] == (True, False) and ra[2] < 2.0
    m64, m80 = ra[2] * R.RESET_TOL, rb[2] * R.RESET_TOL
    su = max(1.0, float(np.max(np.abs(a.us[step - 2]))))
    reach = R.MARGIN * abs(m64 - m80) + 2.0 * R.FLOOR_ULPS * R.EPS * (su * su + 2.0)
    print(f"{name} step {step}: min|dfu| - tol = {m64 - R.RESET_TOL:.3e}, reach of a rounding {reach:.3e}")
    assert m64 - R.RESET_TOL >= reach


@pytest.mark.parametrize("name", sorted(PINNED))
def test_bounds_follow_the_rule(name):
    g, b, r = R.gaps(name), R.bounds(name), R.run(name)
    assert len(g) == len(b) == len(r.us)
    for (gu, gf), (bu, bf), u in zip(g, b, r.us):
        su = max(1.0, float(np.max(np.abs(u))))
        assert bu == R.MARGIN * gu + R.FLOOR_ULPS * R.EPS * su and bf >= R.MARGIN * gf + 7.0 * R.FLOOR_ULPS * R.EPS
        assert bu < 1e-9 and bf < 1e-8


def test_alpha_rule():
    u = np.linspace(1.0, 1.2, 64)
    r = R.run("broyden64_good")
    fu = u * u - 2.0
    assert float(r.alphas[0][1]) == 1.0 / ((2.0 * np.sqrt(fu @ fu)) / max(np.sqrt(u @ u), 1.0))
    assert float(R.run("broyden64_small_fu").alphas[0][1]) == 1.0 and float(R.run("broyden64_alpha").alphas[0][1]) == 1.0 / 2.5
    assert float(R.run("klement64_alpha").alphas[0][1]) == 2.8      # Klement's J is α·1, not inverted


@pytest.mark.parametrize("rule", ["good_broyden", "bad_broyden"])
def test_updated_inverse_satisfies_the_secant_equation(rule):
    """after an update J⁻¹_new·dfu = δu (both rules are rank-1 secant updates of the inverse)"""
    f, u0 = R.coupled(2.0, 0.1), np.linspace(1.0, 1.5, 40)
    a, b = R.solve(f, u0, update_rule=rule, stop_after=3), R.solve(f, u0, update_rule=rule, stop_after=2)
    du, dfu = a.us[2] - a.us[1], a.fus[2] - a.fus[1]
    assert np.max(np.abs(a.J @ dfu - du)) <= 1e-12 * np.max(np.abs(du))
    assert np.linalg.matrix_rank(a.J - b.J, tol=1e-10) == 1 and np.max(np.abs(a.J - a.J.T)) > 1e-4


def test_klement_zero_prediction():
    """alpha = 1, constant residual 1: J becomes 1 + ((0 − 1·(−1))/1)·(−1)·1 = 0 at every update, so steps 2, 3 and 4 ask for a
    reset and the third ends the solve without being applied (klement.jl:116-128, reset_conditions.jl:111-120, solve.jl:342-348)"""
    r = R.run("klement_reset64")
    assert r.J[-1] == 0.0 and r.nresets == 3 and len(r.us) == 3 and [float(a) for _s, a in r.alphas] == [1.0, 1.0, 1.0]


def test_matrix_bound_is_entrywise():
    b = R.matrix_bound("broyden130_nonsym")
    assert b.shape == (130, 130) and float(b.min()) > 0.0 and float(b.max()) < 1e-9
