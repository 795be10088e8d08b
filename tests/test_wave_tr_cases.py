"""The yardstick of the per-wavefront SimpleTrustRegion tests, checked on the CPU: the case list is what it is meant to be (the
oracle's retcodes, and a census of the oracle's branches); a restatement that rounds the way the wavefront kernel may passes
the shared assertion at the GPU test's thresholds; and each of three planted defects fails that same assertion on at least
one case."""
import numpy as np
import pytest

import wave_tr_cases as W
from oracle import reference_restatement as R

SEGMENTS_SCALED = {9: 220, 16: 214, 33: 238, 64: 263}   # segment-branch counts of `scaled`


def test_case_list_pinned():
    assert W.NS == (9, 16, 33, 64) and W.NB == 130 and W.NB % 4 and W.MAXITERS == 300
    assert list(W.CASES) == ["rough", "scaled", "shrink0", "capped"]
    assert W.CASES["shrink0"][3] == {"max_shrink_times": 0} and W.CASES["shrink0"][0] is W.CASES["rough"][0]
    assert W.CASES["capped"][0] is W.CASES["scaled"][0]
    assert (W.MIN_SAME, W.U_TOL) == (0.97, 1e-10)
    P, u0 = W.inputs(9)
    assert P.shape == u0.shape == (130, 9) and 1.0 <= P.min() and P.max() < 4.0 and u0.min() < 0.0
    rng = np.random.default_rng(9)
    assert np.array_equal(P, rng.uniform(1.0, 4.0, (130, 9)))
    assert np.array_equal(u0, rng.uniform(0.5, 2.0, (130, 9)) + 1.5 * rng.standard_normal((130, 9)))
    u = u0[0]
    assert np.array_equal(W.scaled_f(u, P[0]), 0.1 * W.dense_f(u, P[0]))
    fd = np.array([(W.dense_f(u + 1e-6 * e, P[0]) - W.dense_f(u - 1e-6 * e, P[0])) / 2e-6 for e in np.eye(9)]).T
    assert np.max(np.abs(fd - W.dense_jac(u, P[0]))) < 1e-8


@pytest.mark.parametrize("n", W.NS)
def test_oracle_retcodes(n):
    for case in ("rough", "scaled", "capped"):
        _, resid, rc, it = W.oracle(case, n)
        assert (rc == R.SUCCESS).all() and it.max() < W.MAXITERS, case
        assert np.max(np.abs(resid)) <= W.ABSTOL
    assert W.oracle("rough", n)[3].max() <= 36
    _, _, rc, it = W.oracle("shrink0", n)
    assert set(rc) == {R.SUCCESS, R.SHRINK_EXCEEDED} and (rc == R.SHRINK_EXCEEDED).sum() >= 1


def _census(case, n):
    cen = {}
    out = W.restatement_solve(case, n, census=cen)
    for a, b in zip(out, W.oracle(case, n)):            # the oracle's bits, so the oracle's branches
        assert np.array_equal(a, b, equal_nan=True)
    return cen, out


def test_branch_census_of_the_oracle():
    total = {}
    for n in W.NS:
        cen, _ = _census("scaled", n)
        for k in ("newton", "clipped", "segment", "expand"):
            assert cen.get(k, 0) > 150, (n, cen)
        assert cen["segment"] == SEGMENTS_SCALED[n]
        for k, v in cen.items():
            total[k] = total.get(k, 0) + v
        rough, _ = _census("rough", n)
        assert min(rough.get(k, 0) for k in ("newton", "clipped", "rejected", "shrink", "expand")) >= 100, (n, rough)
    assert total.get("rejected", 0) >= 1 and total.get("shrink", 0) >= 1, total


@pytest.mark.parametrize("n", W.NS)
def test_shrink0_ends_every_shrinking_system(n):
    cen, (_, _, rc, _) = _census("shrink0", n)
    assert (rc == R.SHRINK_EXCEEDED).sum() == cen["shrink"] >= 1
    # the systems that never shrink are those that `rough` solves without a shrink: Success, and the same answer
    ok = rc == R.SUCCESS
    assert ok.any() and np.array_equal(W.oracle("shrink0", n)[0][ok], W.oracle("rough", n)[0][ok])


@pytest.mark.parametrize("case", list(W.CASES))
@pytest.mark.parametrize("n", W.NS)
def test_rerounded_restatement_passes_the_shared_assertion(case, n):
    """column-permuted solve, reversed-order sums, ‖Jδ‖²: the differences the wavefront kernel is allowed"""
    out = W.restatement_solve(case, n, rerounded=True)
    assert not np.array_equal(out[0], W.oracle(case, n)[0])     # it does round differently
    share = W.check_against_oracle(*out, W.oracle(case, n))
    assert share == 1.0                                          # the room below 1.00 is not used by rounding alone


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_planted_defects_fail_the_shared_assertion(defect):
    caught = []
    for case in W.CASES:
        for n in W.NS:
            try:
                W.check_against_oracle(*W.restatement_solve(case, n, defect=defect), W.oracle(case, n))
            except AssertionError:
                caught.append((case, n))
    assert caught, f"{defect} passes every case"
    print(defect, "caught by", caught)


def test_the_assertion_helper_itself():
    ref = W.oracle("rough", 9)
    u, resid, rc, it = (a.copy() for a in ref)
    assert W.check_against_oracle(u, resid, rc, it, ref) == 1.0
    it2 = it.copy()
    it2[:3] += 1                                                 # 3 of 130 off by a step: 0.977, allowed
    assert W.check_against_oracle(u, resid, rc, it2, ref) == pytest.approx(127 / 130)
    it2[:4] = it[:4] + 1                                         # 4 of 130: 0.969, refused
    with pytest.raises(AssertionError):
        W.check_against_oracle(u, resid, rc, it2, ref)
    rc2 = rc.copy()
    rc2[7] = R.MAXITERS
    with pytest.raises(AssertionError):
        W.check_against_oracle(u, resid, rc2, it, ref)
    u2 = u.copy()
    u2[5, 2] += 2e-10
    with pytest.raises(AssertionError):
        W.check_against_oracle(u2, resid, rc, it, ref)
    u2[5, 2] = np.nan
    with pytest.raises(AssertionError):
        W.check_against_oracle(u2, resid, rc, it, ref)
    r2 = resid.copy()
    r2[0, 0] = 2 * W.ABSTOL
    with pytest.raises(AssertionError):
        W.check_against_oracle(u, r2, rc, it, ref)


@pytest.mark.parametrize("n", W.F32_NS)
def test_float32_record_matches_a_recomputed_sample(n):
    """tests/golden/wave_tr_f32_steps.json holds what ensemble_f32.simple_trust_region_f32 gives: all Success; recomputed here
    for every system of n = 16 and for ten of n = 64"""
    rc, it = W.f32_reference(n)
    assert rc.shape == it.shape == (W.NB,) and (rc == R.SUCCESS).all()
    systems = list(range(W.NB)) if n == 16 else list(range(0, W.NB, 13))
    rc2, it2 = W.f32_reference_compute(n, systems)
    assert np.array_equal(rc[systems], rc2) and np.array_equal(it[systems], it2)
