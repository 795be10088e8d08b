"""tests/precond_reference.py kept honest without a GPU: the float64 sweep is the oracle's ILU(0) bit for bit, the long-double
sweep has the defining property of ILU(0), the substitutions solve L U z = x, every case selects the schedule it is listed for,
and the hand-worked ILU(τ) cases are what the oracle's Crout restatement gives.

Schedules and float64-versus-long-double gaps of the cases (levels of L / U, widest level of L / U, the kernel that walks L / U —
`chain` is the persistent workgroup, `launch` one kernel per level — and max |float64 − long double| / max |long double| in units
of 2⁻⁵² for the factors and for one application to the case's random vector), as this file measures them:

  case                ordering    n      levels     widest       L / U             factors  apply
  tridiag16x300       natural     4800   16 / 16    300 / 300    launch / launch   0.40     0.78
  tridiag17x300       natural     5100   17 / 17    300 / 300    chain / chain     0.41     0.59
  tridiag17x4096      natural     69632  17 / 17    4096 / 4096  chain / chain     0.41     0.66
  tridiag17x4097      natural     69649  17 / 17    4097 / 4097  launch / launch   0.40     0.69
  mixed_schedule      natural     1545   46 / 46    1500 / 1426  chain / chain     0.95     0.90
  mixed_schedule      multicolor  1545   3 / 3      1510 / 1484  launch / launch   1.43     1.09
  lower_bidiagonal    natural     500    500 / 1    1 / 500      chain / launch    0.10     0.53
  upper_bidiagonal    natural     500    1 / 500    500 / 1      launch / chain    0.00     0.58
  random_unsymmetric  natural     2000   10 / 13    481 / 485    launch / launch   0.36     1.47
  random_unsymmetric  multicolor  2000   7 / 7      659 / 497    launch / launch   0.36     0.93
  random_banded       natural     2000   196 / 185  97 / 120     chain / chain     0.65     1.01
  random_banded       multicolor  2000   8 / 8      545 / 325    launch / launch   0.72     1.60
  dense40             natural     40     40 / 40    1 / 1        chain / chain     3.39     3.12
  diagonal300         natural     300    1 / 1      300 / 300    launch / launch   0.00     0.30
  one                 natural     1      1 / 1      1 / 1        launch / launch   0.00     0.31

The chain kernels meet a level wider than their 1024 threads in tridiag17x4096 (four strided passes per level) and in
mixed_schedule (two)."""
import numpy as np
import pytest
import scipy.sparse as sp

import precond_reference as PR
from oracle import reference_restatement as R

U = 2.0 ** -53


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} entries differ, first at {bad[0]}: {a[bad[0]]!r} != {b[bad[0]]!r}"


def _same_csr(A, B, what=""):
    A, B = sp.csr_matrix(A).copy(), sp.csr_matrix(B).copy()
    A.sort_indices(); B.sort_indices()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices), f"{what}: pattern"
    _same(A.data, B.data, what)


def test_the_restated_rule_at_its_edges():
    assert not PR.chain_pays([300] * 16) and PR.chain_pays([300] * 17)
    assert PR.chain_pays([4096] * 17) and not PR.chain_pays([4097] * 17)
    assert PR.chain_pays([1] * 17) and not PR.chain_pays([])
    assert PR.chain_pays([1] * 16 + [68 * 1024]) and not PR.chain_pays([1] * 16 + [68 * 1024 + 1])      # 16 + 68 < 85 ≤ 16 + 69


def test_level_widths_by_brute_force():
    """levels from the definition on a dense boolean copy of a small random pattern"""
    A = PR.random_unsymmetric(60, 0.05, seed=3)
    D = A.toarray() != 0
    n = D.shape[0]
    lev = np.zeros(n, dtype=int)
    for i in range(n):
        lev[i] = max([lev[k] + 1 for k in range(i) if D[i, k]], default=0)
    levu = np.zeros(n, dtype=int)
    for i in range(n - 1, -1, -1):
        levu[i] = max([levu[k] + 1 for k in range(i + 1, n) if D[i, k]], default=0)
    wl, wu = PR.level_widths(A)
    assert np.array_equal(wl, np.bincount(lev)) and np.array_equal(wu, np.bincount(levu))
    assert wl.sum() == wu.sum() == n


@pytest.mark.parametrize("name,ordering", PR.CASE_IDS)
def test_every_case_selects_the_schedule_it_is_listed_for(name, ordering):
    assert PR.schedule(name, ordering) == PR.EXPECTED[(name, ordering)]
    A = PR.matrix(name)
    d = np.abs(A.diagonal())
    if name != "dense40":
        assert np.all(np.asarray(abs(A).sum(axis=1)).ravel() - d < d)          # strictly diagonally dominant by rows


def test_the_case_list_covers_what_it_is_for():
    E = PR.EXPECTED
    assert set(E) == set(PR.CASE_IDS)
    wide_chain = [k for k, (nl, nu, wl, wu, cl, cu) in E.items() if (cl and wl > 1024) or (cu and wu > 1024)]
    assert ("mixed_schedule", "natural") in wide_chain and ("tridiag17x4096", "natural") in wide_chain
    assert {(cl, cu) for (_, _, _, _, cl, cu) in E.values()} == {(False, False), (True, True), (True, False), (False, True)}
    assert PR.matrix("mixed_schedule").shape[0] == 1545 and PR.matrix("tridiag17x4097").shape[0] == 69649
    P = (PR.matrix("random_unsymmetric") != 0).astype(int)
    assert (P != P.T).nnz > 0                                                    # an unsymmetric pattern


@pytest.mark.parametrize("name,ordering", PR.CASE_IDS)
def test_float64_sweep_is_the_oracles_ilu0_bit_for_bit(name, ordering):
    perm = PR.permutation(name, ordering)
    rp, ci, dg, lu = PR.factors(name, ordering)
    Lo, Uo = R.ilu0(PR.matrix(name), perm)
    L, Uf = PR.split_lu(rp, ci, lu)
    _same_csr(L, Lo, f"{name} {ordering} L")
    _same_csr(Uf, Uo, f"{name} {ordering} U")
    rp2, ci2, dg2, lu2 = PR.pack_lu(L, Uf)
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci) and np.array_equal(dg2, dg)
    _same(lu2, lu, "pack_lu(split_lu)")


@pytest.mark.parametrize("name,ordering", PR.CASE_IDS)
def test_long_double_sweep_has_the_defining_property_and_the_gaps_are_small(name, ordering):
    """(L U)_ij = A_ij on the pattern, for the long-double factors rounded to float64 and multiplied in float64: a dot product of
    k + 1 terms and the rounding of its factors stay within γ_{k+3} (|L||U|)_ij, k the longest row. The gap of the float64 sweep
    to it (the yardstick should a device comparison ever need one) is printed and stays under 4 · 2⁻⁵²."""
    perm = PR.permutation(name, ordering)
    rp, ci, dg, lul = PR.factors(name, ordering, PR.LD)
    Ap = PR.permuted(PR.matrix(name), perm)
    L, Uf = PR.split_lu(rp, ci, lul.astype(np.float64))
    k = int(np.diff(rp).max()) + 3
    g = k * U / (1.0 - k * U)
    pat = Ap.copy(); pat.data[:] = 1.0
    res = abs(L @ Uf - Ap).multiply(pat).tocsr()
    bound = (abs(L) @ abs(Uf)).multiply(pat).tocsr()
    assert (res - g * bound).max() <= 0.0
    if name == "dense40":
        assert Ap.nnz == 40 * 40 and pat.nnz == 1600                             # the full pattern: L U = A entirely
    gf, ga = PR.gaps(name, ordering)
    print(f"{name} {ordering}: gap of the float64 sweep to long double: factors {gf:.2f}, apply {ga:.2f} (units of 2^-52)")
    assert gf <= 4.0 and ga <= 4.0


def _solves(rp, ci, dg, lu, perm, what):
    """tri_apply in long double solves Pᵀ L U P z = x: the residual, formed in float64 from z rounded to float64, within
    2 γ_{k+3} |L| (|U| |z|) componentwise"""
    n = rp.size - 1
    x = np.random.default_rng(9).standard_normal(n)
    z = PR.tri_apply(rp, ci, dg, lu, perm, x, PR.LD).astype(np.float64)
    L, Uf = PR.split_lu(rp, ci, np.asarray(lu, dtype=np.float64))
    zp, xp = (z, x) if perm is None else (z[perm], x[perm])
    k = int(np.diff(rp).max()) + 3
    g = 2.0 * k * U / (1.0 - k * U)
    assert np.all(np.abs(L @ (Uf @ zp) - xp) <= g * (abs(L) @ (abs(Uf) @ np.abs(zp)))), what


@pytest.mark.parametrize("name,ordering", [("dense40", "natural"), ("random_banded", "multicolor"), ("mixed_schedule", "natural")])
def test_tri_apply_solves_with_the_ilu0_factors(name, ordering):
    rp, ci, dg, lu = PR.factors(name, ordering)
    _solves(rp, ci, dg, lu, PR.permutation(name, ordering), name)
    if name == "dense40":                        # ILU(0) of a full pattern is the LU: M⁻¹ A x = x to the conditioning of A
        A = PR.matrix(name)
        x = np.random.default_rng(9).standard_normal(40)
        z = PR.tri_apply(rp, ci, dg, lu, None, A @ x)
        assert np.max(np.abs(z - x)) <= 1e-12 * np.max(np.abs(x))


@pytest.mark.parametrize("name", ["unsymmetric400_tau0", "tridiagonal3000_tau0"])
def test_tri_apply_solves_with_the_complete_lu_of_ilut_at_tau_zero(name):
    A, tau, (rp, ci, dg, lu) = PR.ilut_case(name)
    assert tau == 0.0
    _solves(rp, ci, dg, lu, None, name)
    L, Uf = PR.split_lu(rp, ci, lu)
    assert abs(L @ Uf - A).max() <= 1e-13 * abs(A).max()                          # τ = 0: the complete LU
    x = np.random.default_rng(9).standard_normal(A.shape[0])
    z = PR.tri_apply(rp, ci, dg, lu, None, A @ x)
    assert np.max(np.abs(z - x)) <= 1e-11 * np.max(np.abs(x))


@pytest.mark.parametrize("name", list(PR.ILUT_HAND))
def test_ilut_hand_cases(name):
    """the drop rule at |z| == τ and one ulp above it, and a pivot created by fill where no diagonal entry is stored"""
    A, tau, Lh, Uh = PR.ILUT_HAND[name]
    L, Uf = R.ilut(A, tau)
    n = A.shape[0]
    _same_csr(L, sp.csr_matrix(np.array(Lh, dtype=np.float64)) + sp.identity(n), name + " L")
    _same_csr(Uf, sp.csr_matrix(np.array(Uh, dtype=np.float64)), name + " U")
    if name == "missing_diagonal":
        assert A[1, 1] == 0.0 and A.nnz == 6
        with pytest.raises(ArithmeticError, match="diagonal"):
            R.ilu0(A)                                                            # ILU(0) needs the stored diagonal
        assert np.array_equal((L @ Uf).toarray(), A.toarray())


def test_ilut_still_raises_on_a_zero_pivot():
    with pytest.raises(ArithmeticError, match="pivot"):
        R.ilut(sp.csr_matrix(np.ones((2, 2))), 0.0)
    with pytest.raises(ArithmeticError, match="pivot"):
        R.ilut(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), 0.0)           # a missing diagonal that no fill creates
    with pytest.raises(ArithmeticError, match="pivot"):
        R.ilu0(sp.csr_matrix(np.ones((2, 2))))


def test_ilut_cases_change_their_pattern_with_tau():
    """what the GPU cases rely on: the three drop tolerances of the unsymmetric family keep different numbers of entries, and
    τ = 0 keeps fill"""
    nnz = [PR.ilut_case(f"unsymmetric400_tau{t}")[2][3].size for t in ("0", "0.05", "0.5")]
    assert nnz[0] > nnz[1] > nnz[2] >= 400
    assert nnz[0] > PR.ilut_case("unsymmetric400_tau0")[0].nnz
    A = PR.matrix("random_banded")
    rp, ci, order = PR.shuffled(A)
    B = sp.csr_matrix((A.data[order], ci, rp), shape=A.shape)
    assert not B.has_sorted_indices and (B != A).nnz == 0
