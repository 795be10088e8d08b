"""Pins of tests/bcr_reference.py — the float64 restatement of block cyclic reduction that calibrates the bounds of
tests/test_gpu_bcr.py — and of the bounds themselves: on every committed run the restatement's own error against the
long-double solve is at most a quarter of the bound that run is tested with on the device, and every bound is 8 × the
restatement's maximum over its family and inversion kernel, rounded up to a power of two. Nothing here needs a GPU."""
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sla

import band_lu_reference as BR
import bcr_reference as B


# ----------------------------------------------------------------------------------------------------- block inverses
@pytest.mark.parametrize("n", [1, 7, 32, 100, 128])
def test_leaf_inverses_agree_where_no_pivoting_is_needed(n):
    """On a diagonally dominant block partial pivoting picks the diagonal, so both Gauss–Jordan variants do the same
    arithmetic: bitwise equal, and equal to LAPACK's inverse to rounding."""
    M = BR.dominant_band(n, n - 1, n - 1, 5 + n).toarray()
    a, p = B.inv_gauss_jordan(M), B.inv_gauss_jordan_pivoted(M)
    assert np.array_equal(a, p)
    assert np.max(np.abs(a - np.linalg.inv(M))) <= 64 * BR.U64 * np.max(np.abs(a))


@pytest.mark.parametrize("n", [2, 33, 128])
def test_pivoted_leaf_inverts_what_the_diagonal_cannot(n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    M[0, 0] = 0.0
    with pytest.raises(B.Breakdown):
        B.inv_gauss_jordan(M)
    X = B.inv_gauss_jordan_pivoted(M)
    kappa = np.linalg.cond(M, np.inf)
    assert np.max(np.abs(X - np.linalg.inv(M))) <= 64 * kappa * BR.U64 * np.max(np.abs(X))
    assert np.max(np.abs(X @ M - np.eye(n))) <= 64 * kappa * n * BR.U64


@pytest.mark.parametrize("mode", ["never", "always"])
@pytest.mark.parametrize("n", [128, 160, 256, 288, 416, 512])
def test_schur_recursion_inverts(n, mode):
    """Every branch of the split: direct, 128 + n2, 256 (128 + 128) + n2 with n2 ≤ 128, and n2 > 128 (a second recursion)."""
    M = BR.dominant_band(n, n // 2, n - 1, n).toarray()
    X = B.invert(M, B.LEAVES[mode])
    assert np.max(np.abs(X - np.linalg.inv(M))) <= 256 * BR.U64 * np.max(np.abs(X))


# ------------------------------------------------------------------------------------------------------------ the solve
@pytest.mark.parametrize("mode", ["never", "always"])
@pytest.mark.parametrize("n,kl,ku", [(128, 20, 31), (97, 32, 5), (300, 40, 64), (1000, 37, 20), (700, 150, 133)])
def test_restatement_matches_scipy_and_the_long_double_solve(n, kl, ku, mode):
    J = BR.dominant_band(n, kl, ku, n + kl)
    x_true = np.random.default_rng(n).standard_normal(n)
    b = BR.manufactured(J, x_true)
    F = B.Factorisation(J, mode)
    m = -(-n // B.block_order(kl, ku))
    assert F.b == B.block_order(kl, ku) and F.levels == math.ceil(math.log2(m)) + 1
    x = F.solve(b)
    kappa = BR.cond_inf(J)
    xs = sla.solve(J.toarray(), b)
    assert np.max(np.abs(x - xs)) <= 64 * kappa * BR.U64 * np.max(np.abs(xs))
    be, fe = B.errors(J, x, b, BR.reference_solve(J, b), kappa)
    assert be <= 16 and fe <= 16, (be, fe)


def test_restatement_of_the_exchanged_family_needs_the_pivoted_leaf():
    J, M, perm = B.exchanged(300, 20, 30, 3)
    assert np.all(J.diagonal()[0::2] == 0.0)
    b = BR.manufactured(J, np.ones(300))
    with pytest.raises(B.Breakdown):
        B.Factorisation(J, "never")
    x = B.solve(J, b, "always")
    x_ref = BR.reference_solve(M, b[np.argsort(perm)])
    be, fe = B.errors(J, x, b, x_ref, BR.cond_inf(J))
    assert be <= 16 and fe <= 16, (be, fe)


@pytest.mark.parametrize("e", [-1000, -200, 200, 1000])
def test_restatement_is_invariant_under_powers_of_two(e):
    """What the device's exponent-range test asks of the kernel holds for the algorithm: scaling A by 2^e scales x by 2^−e
    (exactly here: no intermediate leaves the normal range far enough to matter)."""
    J, b, _x, _k, _blk, _lev = B.problem("order64")
    x = B.solve(J, b)
    xs = B.solve((J * np.ldexp(1.0, e)).tocsr(), b)
    assert np.max(np.abs(np.ldexp(xs, e) - x)) <= 8 * BR.U64 * np.max(np.abs(x))


@pytest.mark.parametrize("mode", ["never", "always"])
@pytest.mark.parametrize("kind", list(B.BREAKDOWN_LEVEL))
def test_breakdown_cases_break_down_at_the_stated_level(kind, mode):
    Jp, vals, M = B.breakdown(kind)
    assert BR.bandwidths(vals) == BR.bandwidths(Jp) == (20, 30) and np.array_equal(vals.toarray(), M, equal_nan=True)
    with pytest.raises(B.Breakdown) as e:
        B.Factorisation(vals, mode)
    assert e.value.level == B.BREAKDOWN_LEVEL[kind]
    B.Factorisation(Jp, mode)   # the pattern matrix itself is fine


# ------------------------------------------------------------------------------------------------------- the case list
def test_case_list_covers_orders_kernels_triangles_and_level_shapes():
    orders, tri = set(), set()
    for b in B.ORDERS:
        c = B.CASES[f"order{b}"]
        n, kl, ku, _seed = c["args"]
        assert B.block_order(kl, ku) == b and kl != ku and -(-n // b) == c["m"] >= 4
        orders.add(b)
        tri.add("kl>ku" if kl > ku else "ku>kl")
        tri.add("kl=b" if kl == b else "ku=b" if ku == b else "")
    assert orders == set(range(32, 513, 32)) and {"kl>ku", "ku>kl", "kl=b", "ku=b"} <= tri
    assert {b for b in B.ORDERS if "always" in B.CASES[f"order{b}"]["modes"]} == B.BOTH == {32, 128, 160, 256, 288, 512}
    # block-row counts of both parities at each of the first five levels, an even row without a right neighbour (odd m)
    # and cP ≠ cQ (even m)
    chains = []
    for m in B.LEVEL_M:
        ch = [m]
        while ch[-1] > 1:
            ch.append((ch[-1] + 1) // 2)
        assert len(ch) == math.ceil(math.log2(m)) + 1 == B.levels_of(m)
        chains.append(ch)
    for lvl in range(5):
        ms = {ch[lvl] for ch in chains if len(ch) > lvl and ch[lvl] >= 2}
        assert {x % 2 for x in ms} == {0, 1}, (lvl, ms)
    for m in B.LEVEL_M:
        assert {B.CASES[f"levels{m}_{n}"]["args"][0] for n in (32 * m, 32 * m - 31, 32 * m - 1)} == {32 * m, 32 * m - 31, 32 * m - 1}


def test_brusselator_needs_the_renumbering_to_reach_cyclic_reduction():
    """In the problem's own numbering the half bandwidth is N²: two block rows at N = 16, beyond block order 512 at N = 24."""
    from oracle import reference_restatement as R
    for N, blk in ((16, 64), (24, 96)):
        P = R.Brusselator2D(N)
        assert BR.bandwidths(P.jac(np.ones(P.n))) == (N * N, N * N)
        J = B.brusselator(N, 600 + N)
        assert max(BR.bandwidths(J)) == 4 * N and B.block_order(*BR.bandwidths(J)) == blk
        # a symmetric permutation: the same multiset of entries and the same diagonal sum
        J0 = P.jac(1.0 + 0.1 * np.random.default_rng(600 + N).standard_normal(P.n))
        assert np.array_equal(np.sort(J.data), np.sort(J0.data)) and np.isclose(J.diagonal().sum(), J0.diagonal().sum())


# ---------------------------------------------------------------------------------------------------------- the bounds
@functools.lru_cache(maxsize=None)
def _restatement_errors(name, mode, rhs):
    J, b, x_ref, kappa, blk, lev = B.problem(name, rhs)
    F = B.Factorisation(J, mode)
    assert (F.b, F.levels) == (blk, lev)
    return B.errors(J, F.solve(b), b, x_ref, kappa)


@pytest.mark.parametrize("name,mode,rhs", B.RUNS, ids=[f"{n}-{m}-{r}" for n, m, r in B.RUNS])
def test_restatement_stays_within_a_quarter_of_the_bound(name, mode, rhs):
    be, fe = _restatement_errors(name, mode, rhs)
    bb, fb = B.BOUNDS[(B.CASES[name]["family"], mode)]
    print(f"{name} {mode} rhs {rhs}: backward {be:.2f} u (bound {bb}), forward {fe:.4f} κu (bound {fb})")
    assert be <= bb / 4 and fe <= fb / 4, (be, fe, bb, fb)


def test_the_bounds_are_eight_times_the_restatement_rounded_up():
    """The rule the constants were set by: 8 × the restatement's maximum per family and kernel, rounded up to a power of two,
    so bound / (8 × maximum) lies in [1, 2) where they were measured. Another BLAS or thread count moves the maxima a little:
    the assertion allows a factor of two below and four above (the quarter-of-the-bound test above holds throughout)."""
    worst = {}
    for name, mode, rhs in B.RUNS:
        k = (B.CASES[name]["family"], mode)
        be, fe = _restatement_errors(name, mode, rhs)
        o = worst.get(k, (0.0, 0.0))
        worst[k] = (max(o[0], be), max(o[1], fe))
    assert set(worst) == set(B.BOUNDS)
    for k, (be, fe) in sorted(worst.items()):
        bb, fb = B.BOUNDS[k]
        assert math.log2(bb) % 1 == 0 and math.log2(fb) % 1 == 0
        print(f"{k}: restatement maximum {be:.2f} u, {fe:.4f} κu; bounds {bb:g} u, {fb:g} κu")
        assert 0.5 <= bb / (B.MARGIN * be) <= 8 and 0.5 <= fb / (B.MARGIN * fe) <= 8, (k, be, fe)
