"""tests/gmres_reference.py checked without a GPU: its assertions accept what is right — the oracle's float64 formulations of
GMRES over every case and every (m, k) tests/test_gpu_gmres.py uses, which is also where the committed tolerance table comes
from — and reject what is wrong: float64 copies of the reference with one planted defect each."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmres_reference as GR  # noqa: E402
from oracle import reference_restatement as R  # noqa: E402

pytestmark = pytest.mark.skipif(not GR.LONGDOUBLE_OK, reason="np.longdouble has fewer than 64 significand bits")


# ------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("n", [1, 2, 3, 31, 33, 63, 65, 99])
@pytest.mark.parametrize("pe", GR.PES)
def test_reference_solves_the_system(n, pe):
    """run to breakdown (m ≥ n) the reference returns the solution of the dense system; the CSR products and their transposes
    are those of the dense matrix"""
    case = GR.convdiff_n(n, pe)
    A = GR.to_scipy(case).toarray()
    op = GR.Operator(case)
    v = GR.rhs(n, "probe")
    assert np.allclose(np.asarray(op.A(np.asarray(v, GR.LD)), float), A @ v, rtol=1e-14, atol=0)
    assert np.allclose(np.asarray(op.AT(np.asarray(v, GR.LD)), float), A.T @ v, rtol=1e-14, atol=0)
    ref = GR.gmres(op, case.b, rtol=1e-15, restart=max(n, 1), itmax=10 * n)
    assert ref.converged and ref.iters <= n
    xs = np.linalg.solve(A, case.b)
    assert np.linalg.norm(np.asarray(ref.x, float) - xs) <= 1e-13 * np.linalg.norm(xs)
    assert ref.residuals[0] == ref.rnorm0 and len(ref.residuals) == ref.iters + 1
    assert all(b <= a * (1 + 1e-15) for a, b in zip(ref.residuals, ref.residuals[1:])), "GMRES residuals never grow"


def test_exact_families():
    """cyclic: the residual stays 4 for n − 1 steps and step n is an exact breakdown with P x = b bit for bit; with m = 3 and 12
    steps nothing moves. scaled_identity: an exact breakdown at step 1 with x = b/2. The oracle's column forms agree."""
    for n in (5, 33):
        case = GR.cyclic(n)
        e = np.zeros(n)
        e[n - 1] = 4.0
        for m in (n, n + 3):
            ref = GR.gmres(GR.Operator(case), case.b, restart=m)
            assert (ref.iters, ref.restarts, ref.converged, float(ref.rnorm)) == (n, 0, True, 0.0)
            assert [float(r) for r in ref.residuals] == [4.0] * n + [0.0]
            GR.check_exact(ref.x, e)
            GR.check_exact(GR.to_scipy(case) @ np.asarray(ref.x, float), case.b)
            for ortho in ("mgs", "cgs2", "dcgs2"):
                x, info = R.gmres(lambda z: GR.to_scipy(case) @ z, case.b, restart=m, ortho=ortho)
                GR.check_exact(x, e)
                GR.check_counts(GR.as_info(info), ref)
    case = GR.cyclic(5)
    ref = GR.gmres(GR.Operator(case), case.b, restart=3, itmax=12)
    assert (ref.iters, ref.restarts, ref.converged, ref.failed, float(ref.rnorm)) == (12, 3, False, False, 4.0)
    GR.check_exact(ref.x, np.zeros(5))
    assert not np.any(np.signbit(np.asarray(ref.x, float)))
    with pytest.raises(R.SStepBreakdown):
        R.gmres(lambda z: GR.to_scipy(GR.cyclic(33)) @ z, GR.cyclic(33).b, restart=33, ortho=("sstep", 4))
    for n in (7, 65):
        case = GR.scaled_identity(n)
        ref = GR.gmres(GR.Operator(case), case.b, restart=30)
        assert (ref.iters, ref.converged, float(ref.rnorm)) == (1, True, 0.0)
        GR.check_exact(ref.x, case.b / 2)


# ------------------------------------------------------------------------------------------------------------- accepts
def test_no_bound_exceeds_the_projects_limits():
    assert set(GR.TABLE) == {(n, pe, m) for n in GR.FIXED_N for pe in GR.PES for m in GR.RESTARTS}
    for key in GR.TABLE:
        tx, tr = GR.fixed_bounds(*key)
        assert GR.FLOOR <= tx <= GR.LIMIT_X and GR.FLOOR <= tr <= GR.LIMIT_R
    assert set(GR.GROUP_TABLE) == set(GR.all_specs(R))
    for name in GR.GROUP_TABLE:
        tx, tr = GR.group_bounds(name)
        assert GR.FLOOR <= tx <= GR.LIMIT_X and GR.FLOOR <= tr <= GR.LIMIT_R


@pytest.mark.parametrize("n", GR.FIXED_N)
@pytest.mark.parametrize("pe", GR.PES)
def test_oracle_formulations_pass_fixed_work_and_give_the_table(n, pe):
    """every float64 formulation of the oracle passes check_iterate at every (m, k) of the GPU file, and the spread they show —
    x, rnorm and rnorm0 — is the committed table's row (rounded up to a power of two)"""
    case = GR.convdiff_n(n, pe)
    op = GR.Operator(case)
    for m in GR.RESTARTS:
        tx, tr = GR.fixed_bounds(n, pe, m)
        sx = sr = 0.0
        names = set()
        counts = GR.fixed_counts(n, pe, m)
        assert counts[0] == 1 and counts[-1] <= GR.KMAX
        for k in counts:
            ref = GR.fixed_reference(n, pe, m, k)
            runs = GR.oracle_runs(R, case, m, k)
            assert len(runs) >= 4
            for name, x, info in runs:
                inf = GR.as_info(info)
                assert inf["iters"] == k, (name, m, k)
                GR.check_iterate(x, inf, ref, tx, tr, op=op, b=case.b)
                dx, dr = GR.deviation(x, inf, ref)
                sx, sr = max(sx, dx), max(sr, dr)
                names.add(name)
        assert names & set(GR.SSTEP_RUNS), f"no s-step formulation contributed to the row of m = {m}"
        assert (GR.pow2_up(sx), GR.pow2_up(sr)) == GR.TABLE[(n, pe, m)], (m, sx, sr)


def _accept(name, s, ref):
    """the oracle's column forms pass the solve's checks at its own bounds, and their spread is its committed row"""
    tx, tr = GR.group_bounds(name)
    sx = sr = 0.0
    for form, x, info in GR.oracle_on_spec(R, s, ref.iters):
        inf = GR.as_info(info)
        if form.startswith("sstep"):      # fixed work at the reference's count
            assert inf["iters"] == ref.iters
            inf.update(converged=ref.converged, restarts=ref.restarts)
        GR.check_counts(inf, ref)
        GR.check_spec(x, inf, s, ref, tx, tr)
        dx, dr = GR.deviation(x, inf, ref)
        sx, sr = max(sx, dx), max(sr, dr)
    assert (GR.pow2_up(sx), GR.pow2_up(sr)) == GR.GROUP_TABLE[name], (name, sx, sr)


@pytest.mark.parametrize("n", GR.STOP_N)
@pytest.mark.parametrize("pe", GR.PES)
def test_tolerance_stops_are_decided_and_the_oracle_passes(n, pe):
    """at every tolerance stop of the GPU file the reference's residual at the stopping step and at the step before are away
    from tol by more than 1e-6 relative, so the count is not a coin toss; the oracle's column forms stop at the same count
    with the same iterate, and their spread is the stop's row of GROUP_TABLE"""
    for m in GR.STOP_M:
        for i, stop in enumerate(GR.STOPS):
            ref, atol, rtol = GR.stop_reference(n, pe, m, stop)
            s = GR.stop_specs()[GR.stop_name(n, pe, m, i)]
            assert (s.atol, s.rtol, s.m) == (atol, rtol, m)
            assert ref.converged and ref.iters > 2
            assert GR.stop_is_decided(ref, atol + rtol * float(ref.rnorm0)), (m, stop)
            _accept(GR.stop_name(n, pe, m, i), s, ref)


OTHER_SPECS = dict(GR.group_specs(), **GR.brusselator_specs(R))


@pytest.mark.parametrize("name", sorted(OTHER_SPECS))
def test_oracle_formulations_pass_the_other_groups(name):
    """warm starts, preconditioner sides, shifts, the normal form, host-callback cases, Chebyshev: the oracle's float64 column
    forms pass check_iterate and check_counts against the reference at the solve's own bounds, and their spread is the solve's
    row of GROUP_TABLE"""
    s = OTHER_SPECS[name]
    ref = GR.solve_spec(s)
    if s.k == 0:
        assert GR.stop_is_decided(ref, s.atol + s.rtol * float(ref.rnorm0))
    _accept(name, s, ref)


# ------------------------------------------------------------------------------------------------------------- rejects
# defect -> the solve (by its name in GROUP_TABLE) that has to expose it
REJECTING_CASE = {
    "givens_not_applied_to_g": "plain-63",
    "update_k_minus_1": "plain-63",
    "restart_reuses_recurrence": "plain-63",
    "x0_ignored_in_r0": "warm-63-k17",
    "x0_not_added": "warm-63-k17",
    "tol_is_max": GR.stop_name(63, 0.5, 7, 3),
    "left_not_on_b": "prec-left-63-k17",
    "shift_without_weights": "shift0.75-w-63",
    "damping_d_squared": "normal-damped0.5-63",
    "normal_a_for_at": "normal-63",
    "dot_drops_last_entry": "plain-63",
    "subdiagonal_float32": "plain-63",
}


def _judge(name, s, x, info, ref):
    tx, tr = GR.group_bounds(name)
    GR.check_counts(info, ref)
    GR.check_spec(x, info, s, ref, tx, tr)


def test_every_defect_has_a_case():
    assert set(REJECTING_CASE) == set(GR.DEFECTS) and len(GR.DEFECTS) == 12


@pytest.mark.parametrize("defect", GR.DEFECTS)
def test_planted_defect_is_rejected(defect):
    """the float64 copy of the reference passes its case as it is, and fails it with the one line changed"""
    name = REJECTING_CASE[defect]
    s = GR.all_specs(R)[name]
    ref = GR.solve_spec(s)
    good = GR.solve_spec(s, dtype=np.float64)
    _judge(name, s, good.x, GR.as_info(good), ref)
    bad = GR.solve_spec(s, dtype=np.float64, defect=defect)
    with pytest.raises(AssertionError):
        _judge(name, s, bad.x, GR.as_info(bad), ref)


def test_check_exact_and_counts_reject():
    with pytest.raises(AssertionError):
        GR.check_exact(np.array([0.0, 4.0]), np.array([0.0, np.nextafter(4.0, 5.0)]))
    ref = GR.solve_spec(GR.stop_specs()[GR.stop_name(63, 0.5, 7, 0)])
    info = GR.as_info(ref)
    GR.check_counts(info, ref)
    later = dict(info, iters=info["iters"] + 3)
    later["restarts"] = (later["iters"] - 1) // 7
    GR.check_counts(later, ref, exact=False, block=4, m=7)
    with pytest.raises(AssertionError):
        GR.check_counts(dict(later, restarts=later["restarts"] + 1), ref, exact=False, block=4, m=7)
    for wrong in (dict(info, iters=info["iters"] + 1), dict(info, restarts=info["restarts"] + 1),
                  dict(info, converged=False), dict(info, failed=True)):
        with pytest.raises(AssertionError):
            GR.check_counts(wrong, ref)
    with pytest.raises(AssertionError):
        GR.check_counts(dict(info, iters=info["iters"] + 4), ref, exact=False, block=4, m=7)
