"""tests/amg_reference.py checked without a GPU: its assertions accept what is right — the oracle's float64 restatement of the
aggregation AMG on every case tests/test_gpu_amg_direct.py uses, which is also where the committed tolerance table comes from —
and reject what is wrong: float64 copies of the reference with one planted defect each. The two closed forms the GPU file relies
on (chain(4**k) and the stalled Gershgorin matrices) are proved against the restatement at sizes it can run."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_reference as AR  # noqa: E402
from oracle import reference_restatement as R  # noqa: E402

pytestmark = pytest.mark.skipif(not AR.LONGDOUBLE_OK, reason="np.longdouble has fewer than 64 significand bits")


@pytest.mark.parametrize("name", list(AR.CASES))
def test_restatement_passes_every_check_and_its_deviation_is_the_committed_row(name):
    n = AR.matrix(name).shape[0]
    for matching in AR.MATCHINGS:
        S = AR.structure(name, matching)
        for which in (0, 1):
            lv = AR.numbers(S, AR.values(name, which))
            ref = AR.reference_applies(name, matching, which)
            for solve in (False, True):
                O = AR.oracle_with_values(name, matching, which, solve)
                AR.check_structure(S, lv, AR.oracle_as_got(O), f"{matching}/{which}: ",
                                   lmax_ulps=max(int(np.diff(p[0]).max(initial=0)) for p in S.pats))
                for b, y in zip(AR.rhs_set(n, name), ref):
                    AR.check_apply(name, O(b), y)
            # the module's own float64 V-cycle is the restatement to rounding
            V = AR.VCycle(S, AR.values(name, which), np.float64)
            for b, y in zip(AR.rhs_set(n, name), ref):
                AR.check_apply(name, V(b), y)
    assert AR.measure_row(name) == AR.TABLE[name]
    assert max(AR.FACTOR * AR.TABLE[name], AR.FLOOR) <= AR.LIMIT


def test_table_and_case_lists():
    assert set(AR.TABLE) == set(AR.CASES) | {AR.CHAIN4.name}
    assert all(AR.bound(k) <= AR.LIMIT for k in AR.TABLE)
    for name in AR.SAME_AGGREGATES:
        a, g = AR.structure(name, "auto"), AR.structure(name, "greedy")
        assert a.sizes() == g.sizes() and all(np.array_equal(x, y) for x, y in zip(a.aggs, g.aggs)), name
    # what the families are there for
    for name, sizes in (("chain129", [129, 33]), ("chain130", [130, 33]), ("chain200", [200, 50]), ("chain257", [257, 65]),
                        ("chain4094p1", [4094, 2047, 1024, 512, 256, 128]), ("chain4096p1", [4096, 2048, 1024, 512, 256, 128])):
        for m in AR.MATCHINGS:
            assert AR.structure(name, m).sizes() == sizes, (name, m)
    for m in AR.MATCHINGS:
        S = AR.structure("stall600", m)
        assert S.sizes() == [600, 300] and not S.dense
        for cm in (1, 8, 64):
            for base in ("chain300", "bratu20"):
                S = AR.structure(f"{base}cm{cm}", m)
                assert S.dense and S.sizes()[-1] <= cm
        assert any(AR.structure(f"{base}cm{cm}", m).sizes()[-1] % 8 for cm in (1, 8, 64) for base in ("chain300", "bratu20"))
        assert len(AR.structure("bratu48-passes4", m).sizes()) >= 2
    Z = AR.matrix("zeros300")
    assert np.count_nonzero(Z.data == 0.0) == 20 and np.count_nonzero(np.diff(Z.indptr) == 1) == 4
    assert np.all(AR.matrix("negbratu48").diagonal() < 0)
    d = AR.matrix("altrows20").diagonal()
    assert np.all(d[::2] * d[1::2] < 0)


@pytest.mark.parametrize("k", [6, 7])
def test_chain4_closed_form(k):
    S = AR.closed_chain4(k)
    lv = AR.numbers(S, None)
    assert S.sizes() == [4 ** j for j in range(k, 2, -1)] and S.dense
    for matching in AR.MATCHINGS:
        O = R.AggregationAMG(AR.chain(4 ** k), matching=AR.oracle_matching(matching))
        AR.check_structure(S, lv, AR.oracle_as_got(O), matching + ": ")   # (sums of small dyadic numbers: exact in any order)
    for l, L in enumerate(lv):
        d = 2.0 + 0.5 * 4.0 ** l
        assert float(L["lmax"]) == (d + 2.0) / d


@pytest.mark.parametrize("p", [0, 255, 256, AR.GERSHGORIN_N - 1])
def test_gershgorin_cases_stall_at_level_0_with_the_largest_bound_where_it_was_planted(p):
    name = f"gershgorin{p}"
    A = AR.matrix(name)
    assert AR.structure(name, "auto").sizes() == [AR.GERSHGORIN_N]
    # under ANY matching: a row without an off-diagonal entry stays alone, so there are at least n − (rows with one) aggregates
    assert A.shape[0] - np.count_nonzero(np.diff(A.indptr) > 1) > 0.8 * A.shape[0]
    ratio = np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(A.diagonal())
    assert int(np.argmax(ratio)) == p and np.count_nonzero(ratio == ratio[p]) == 1
    lv = AR.numbers(AR.structure(name, "auto"), AR.values(name))
    assert float(lv[0]["lmax"]) == ratio[p] or abs(float(lv[0]["lmax"]) - ratio[p]) <= 4e-16 * ratio[p]


APPLY_CASE = {"restrict_drop_last": "chain200", "prolong_neighbour": "chain200", "nu_off_by_one": "chain200",
              "coarse_nu": "stall600", "omega_twice": "chain200", "omega_none": "chain200", "stale_residual": "chain200",
              "lmax_wrong_level": "chain200", "stale_dinv": "chain200", "coarse_transposed": "altrows20", "border_leak": "chain9"}


@pytest.mark.parametrize("defect", AR.APPLY_DEFECTS)
def test_planted_apply_defects_are_rejected(defect):
    name = APPLY_CASE[defect]
    n = AR.matrix(name).shape[0]
    for matching in AR.MATCHINGS:
        S = AR.structure(name, matching)
        ref = AR.reference_applies(name, matching, 1)
        for d in (None, defect):
            V = AR.VCycle(S, AR.values(name, 0), np.float64, defect=d).update(AR.values(name, 1))
            ys = [V(b) for b in AR.rhs_set(n, name)]
            if d is None:
                for y, r in zip(ys, ref):
                    AR.check_apply(name, y, r)
            else:
                with pytest.raises(AssertionError):
                    for y, r in zip(ys, ref):
                        AR.check_apply(name, y, r)


SETUP_CASE = {"lmax_all_but_last": f"gershgorin{AR.GERSHGORIN_N - 1}", "galerkin_miss": "bratu48-nu1",
              "galerkin_descending": "bratu48-nu1", "aggregates_by_largest_row": "random3000sym-nu1"}


def _got(S, lv):
    return dict(sizes=S.sizes(), aggs=list(S.aggs), lmax=[L["lmax"] for L in lv],
                levels=[dict(nnz=len(L["ci"]), vals=L["v"], rp=L["rp"], ci=L["ci"]) for L in lv])


@pytest.mark.parametrize("defect", AR.SETUP_DEFECTS)
def test_planted_setup_defects_are_rejected(defect):
    name = SETUP_CASE[defect]
    for matching in AR.MATCHINGS:
        S = AR.structure(name, matching)
        lv = AR.numbers(S, AR.values(name))
        AR.check_structure(S, lv, _got(S, lv))
        if defect == "aggregates_by_largest_row":
            got = _got(S, lv)
            a = S.aggs[0]
            last = np.zeros(a.max() + 1, dtype=np.int64)
            np.maximum.at(last, a, np.arange(len(a)))
            got["aggs"][0] = np.argsort(np.argsort(last))[a]
        else:
            got = _got(S, AR.numbers(S, AR.values(name), defect=defect))
        with pytest.raises(AssertionError):
            AR.check_structure(S, lv, got)


def test_pattern_check_by_product_rejects_a_moved_column_and_a_moved_row_boundary():
    S = AR.structure("bratu20cm8", "auto")
    lv = AR.numbers(S, AR.values("bratu20cm8"))
    L = lv[1]
    A = sp.csr_matrix((L["v"], L["ci"], L["rp"]), shape=(L["n"], L["n"]))
    AR.check_pattern_by_product(L["rp"], L["ci"], L["v"], A @ AR.probe(L["n"], 1), 1)
    ci = L["ci"].copy()
    k = len(ci) // 2
    ci[k] = ci[k] + 1 if ci[k] + 1 < L["n"] and ci[k] + 1 not in ci[L["rp"][L["rows"][k]]:L["rp"][L["rows"][k] + 1]] else ci[k] - 2
    rp = L["rp"].copy()
    rp[5] += 1
    for bad in (sp.csr_matrix((L["v"], ci, L["rp"]), shape=A.shape), sp.csr_matrix((L["v"], L["ci"], rp), shape=A.shape)):
        with pytest.raises(AssertionError):
            AR.check_pattern_by_product(L["rp"], L["ci"], L["v"], bad @ AR.probe(L["n"], 1), 1)


def test_ge_solve_pivots():
    A = np.array([[0.0, 2.0, 1.0], [1.0, 1.0, 0.0], [4.0, 0.0, 3.0]])
    b = np.array([1.0, 2.0, 3.0])
    assert np.allclose(np.asarray(AR.ge_solve(A, b, AR.LD), float), np.linalg.solve(A, b), rtol=1e-15)
    with pytest.raises(ArithmeticError):
        AR.ge_solve(np.array([[1.0, 2.0], [1.0, 2.0]]), np.ones(2), np.float64)
