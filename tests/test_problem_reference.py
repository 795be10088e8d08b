"""tests/problem_reference.py without a GPU: over every case the float64 reference in the kernel's order lies within the stated
bound of the long-double reference of the mathematics (to the bit on the integer data), and the assertions the GPU tests use
reject a list of wrong results, each one a defect a kernel of csrc/nk_problems.hip could have."""
import numpy as np
import pytest

import problem_reference as PR

KINDS = ("spread", "exact")


def rejected(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def _res(c, tweak=None):
    res = PR.stencil64(c.ns, c.nl, c.c_lap, c.d, c.v, c.lo, c.hi)
    if tweak is not None:
        res = res.reshape(c.nl, c.ns).copy()
        tweak(res, c.v.reshape(c.nl, c.ns))
        res = res.ravel()
    return res


# ------------------------------------------------------------------------------------------ the two references agree
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PR.BRATU_SHAPES, ids=PR.shape_id)
def test_bratu_stencil_references_agree(shape, kind):
    PR.need_longdouble()
    c = PR.jvp_case(shape, kind)
    exact, M = PR.stencil_exact(c.ns, c.nl, c.c_lap, c.d, c.v, c.lo, c.hi)
    for tiled in (True, False):
        got = PR.stencil64(c.ns, c.nl, c.c_lap, c.d, c.v, c.lo, c.hi, tiled=tiled)
        if kind == "exact":
            PR.same(got, exact.astype(np.float64), "integer data")
        PR.within(got, exact, PR.K_STENCIL * PR.U * M, "stencil")
    for mode in PR.MODES:                   # the reference accepts itself, every output included
        for scaled in (False, True):
            PR.check_jvp(c, mode, scaled, PR.jvp64(c, mode, scaled), "self")


@pytest.mark.parametrize("scale", [0.0, 1.0])
@pytest.mark.parametrize("shape", PR.BRATU_SHAPES, ids=PR.shape_id)
def test_bratu_residual_references_agree(shape, scale):
    PR.need_longdouble()
    c = PR.residual_case(shape, scale)
    f = PR.residual64(c)
    PR.check_residual(c, f, "residual")
    PR.check_diag(c, c.c_exp * np.exp(c.u), "diagonal")
    g = PR.red_grid(f.size)
    PR.check_partials(f, g, PR.partials64(f, g), "partials")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PR.BRUS_SHAPES, ids=PR.brus_id)
def test_brusselator_references_agree(shape, kind):
    PR.need_longdouble()
    c = PR.brus_case(shape, kind)
    for op in (0, 1, 2):
        for scaled in ((False,) if op == 0 else (False, True)):
            got = PR.brus_residual64(c) if op == 0 else PR.brus_jvp64(c, op == 2, scaled)
            exact, M = PR.brus_exact(c, op, scaled)
            if kind == "exact":
                PR.same(got, exact.astype(np.float64), f"integer data, op {op}")
            PR.within(got, exact, PR.K_BRUS * PR.U * M, f"op {op}")


def test_forcing_disc_rim():
    """N = 11: x = 0.3 is a grid coordinate. (0.3, 0.5) and (0.3, 0.7) lie on the rim and count as inside in float64, (0.2, 0.6) too,
    (0.4, 0.6) does not: 0.4 − 0.3 rounds up."""
    bf = PR.brus_forcing(11, np.arange(11))
    inside = {(i, j) for j, i in zip(*np.nonzero(bf))}
    assert inside == {(3, 5), (3, 6), (3, 7), (2, 6)}, inside
    assert np.count_nonzero(PR.brus_forcing(5, np.arange(5))) == 0 and np.count_nonzero(PR.brus_forcing(16, np.arange(16))) > 0


# ------------------------------------------------------------------------------------------------- wrong stencils
def _edge_mutants(c):
    """(name, tweak of the stencil result) — each adds or removes c_lap·(one neighbour) along one edge"""
    ns, nl, cl = c.ns, c.nl, c.c_lap
    flat = lambda v: v.ravel()
    out = []
    if ns >= 2:
        out += [("east dropped at i = 0", lambda r, v: r.__setitem__((slice(None), 0), r[:, 0] + cl * v[:, 1])),
                ("east doubled at i = 0", lambda r, v: r.__setitem__((slice(None), 0), r[:, 0] - cl * v[:, 1])),
                ("west dropped at i = ns − 1", lambda r, v: r.__setitem__((slice(None), -1), r[:, -1] + cl * v[:, -2])),
                ("the neighbour in memory counted at i = ns − 1",
                 lambda r, v: r.__setitem__((slice(None), -1), r[:, -1] - cl * np.roll(flat(v), -1).reshape(v.shape)[:, -1]))]
    if nl >= 2:
        out += [("north dropped at jl = 0", lambda r, v: r.__setitem__(0, r[0] + cl * v[1])),
                ("north doubled at jl = 0", lambda r, v: r.__setitem__(0, r[0] - cl * v[1])),
                ("south dropped at jl = nl − 1", lambda r, v: r.__setitem__(-1, r[-1] + cl * v[-2])),
                ("south doubled at jl = nl − 1", lambda r, v: r.__setitem__(-1, r[-1] - cl * v[-2]))]
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in PR.BRATU_SHAPES if s[0] <= 7 or s[0] == 257 and s[1] <= 4], ids=PR.shape_id)
def test_wrong_stencils_are_rejected(shape, kind):
    c = PR.jvp_case(shape, kind)
    for name, tweak in _edge_mutants(c):
        for mode in PR.MODES:
            rejected(PR.check_jvp, c, mode, False, PR.epilogue64(c, _res(c, tweak), mode, False), name)
    ns, nl, lo, hi = shape
    swapped = PR.jvp_case(shape, kind)
    swapped.lo, swapped.hi = c.hi, c.lo
    if (lo or hi) and nl >= 2:             # (on a one-line slab both ghost lines meet the same point: swapping them is no error)
        rejected(PR.check_jvp, c, 0, False, PR.jvp64(swapped, 0, False), "lo and hi swapped")
    if nl == 1 and (lo or hi):
        blind = PR.jvp_case(shape, kind)
        blind.lo = blind.hi = None
        rejected(PR.check_jvp, c, 0, False, PR.jvp64(blind, 0, False), "the ghost lines ignored on a one-line slab")
        for only in ("lo", "hi"):
            if lo and hi:
                half = PR.jvp_case(shape, kind)
                setattr(half, only, None)
                rejected(PR.check_jvp, c, 0, False, PR.jvp64(half, 0, False), f"{only} ignored on a one-line slab")


@pytest.mark.parametrize("shape", [(5, 5, False, False), (6, 6, False, False), (7, 7, False, False), (5, 3, True, True), (257, 2, False, True)],
                         ids=PR.shape_id)
def test_ragged_tile_mutants_are_rejected(shape):
    """nl mod 4 ≠ 0: the last tile's rows past nl must not be written, its rows below nl must be"""
    c = PR.jvp_case(shape, "spread")
    for mode in PR.MODES:
        good = PR.jvp64(c, mode, False)
        for k in (("r", "dnew", "yacc") if mode == 1 else ("jv",)):       # what the mode writes
            bad = {**good, k: good[k].copy()}
            bad[k][-c.ns:] = PR.canary(c.ns) if k in ("jv", "dnew") else getattr(c, k)[-c.ns:]
            rejected(PR.check_jvp, c, mode, False, bad, f"mode {mode}: last row of {k} left unwritten")
    # A row beyond nl written: line nl of an output lies in the guard behind it, which the hook inspects and reports. What the
    # assertion has to catch is the stray write that stays inside the array: the last line's values one line too low.
    good = PR.jvp64(c, 0, False)
    shifted = {**good, "jv": np.concatenate([good["jv"][:-2 * c.ns], good["jv"][-c.ns:], good["jv"][-c.ns:]])}
    rejected(PR.check_jvp, c, 0, False, shifted, "the last row also written one line too low")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(3, 3, False, False), (5, 2, True, True), (257, 1, True, False)], ids=PR.shape_id)
def test_wrong_epilogues_are_rejected(shape, kind):
    c = PR.jvp_case(shape, kind)
    res, os, n = _res(c), c.out_scale, c.v.size
    for mode in (1, 2):                                    # out_scale applied where the kernel has none
        good = PR.jvp64(c, mode, True)
        if mode == 2:
            bad = {**good, "jv": os * (c.r - res)}
        else:
            r = c.r - os * res
            d = c.c1 * c.v + c.c2 * r
            bad = {**good, "r": r, "dnew": d, "yacc": c.yacc + d}
        rejected(PR.check_jvp, c, mode, True, bad, f"out_scale applied in mode {mode}")
    good = PR.jvp64(c, 3, True)
    rejected(PR.check_jvp, c, 3, True, {**good, "jv": os * (res + c.theta * c.v)}, "the sign of theta")
    good = PR.jvp64(c, 1, False)
    d = c.c2 * c.v + c.c1 * good["r"]
    rejected(PR.check_jvp, c, 1, False, {**good, "dnew": d, "yacc": c.yacc + d}, "c1 and c2 swapped")
    rejected(PR.check_jvp, c, 1, False, {**good, "yacc": good["dnew"].copy()}, "yacc overwritten, not accumulated")
    rejected(PR.check_jvp, c, 1, False, {**good, "r": c.r.copy()}, "r not updated in mode 1")
    rejected(PR.check_jvp, c, 1, False, {**good, "jv": good["r"].copy()}, "jv written in mode 1")
    for mode in PR.MODES:                                  # skip = 1: nothing may change
        ran = PR.jvp64(c, mode, False)
        kept = dict(jv=PR.canary(n), r=c.r, dnew=PR.canary(n), yacc=c.yacc)
        PR.check_jvp(c, mode, False, kept, "skip", skip=True)
        for k in ("jv", "r", "dnew", "yacc"):
            if not np.array_equal(PR.bits(ran[k]), PR.bits(kept[k])):
                rejected(PR.check_jvp, c, mode, False, {**kept, k: ran[k]}, f"mode {mode}: {k} touched with skip = 1", skip=True)
        one = PR.jvp64(c, mode, False)                     # one entry one ulp off
        k = "jv" if mode != 1 else "dnew"
        one[k] = one[k].copy()
        one[k][n // 2] = np.nextafter(one[k][n // 2], np.inf)
        rejected(PR.check_jvp, c, mode, False, one, f"mode {mode}: one ulp")


# ------------------------------------------------------------------------------------------------ wrong residuals
@pytest.mark.parametrize("shape", [(7, 7, False, False), (33, 33, False, False), (257, 5, True, True), (257, 257, False, False)], ids=PR.shape_id)
def test_wrong_partials_are_rejected(shape):
    PR.need_longdouble()
    c = PR.residual_case(shape, 0.0)
    f = PR.residual64(c)
    g = PR.red_grid(f.size)
    good = PR.partials64(f, g)
    PR.check_partials(f, g, good, "good")
    other = PR.partials64(f, g, final=lambda s: ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3])
    if not np.array_equal(PR.bits(other), PR.bits(good)):   # (four wavefronts with entries: the two orders differ)
        rejected(PR.check_partials, f, g, other, "another order")
        PR.check_partials(f, g, other, "another order, bound only", bitwise=False)
    twice = PR.partials64(f, g, extra_last=True)
    rejected(PR.check_partials, f, g, twice, "a past-the-end point counted", bitwise=False)
    one = good.copy()
    one[g] = np.nextafter(one[g], np.inf)
    rejected(PR.check_partials, f, g, one, "one ulp")
    low = good.copy()
    low[:g] = 0.5 * low[:g]
    rejected(PR.check_partials, f, g, low, "a max partial too small", bitwise=False)


def test_another_order_differs_somewhere():
    """the bit check has something to reject: on the 257 × 257 case the two orders of the final combination give different bits"""
    c = PR.residual_case((257, 257, False, False), 0.0)
    f = PR.residual64(c)
    g = PR.red_grid(f.size)
    a, b = PR.partials64(f, g), PR.partials64(f, g, final=lambda s: ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3])
    assert not np.array_equal(PR.bits(a), PR.bits(b))


def test_wrong_residual_entries_are_rejected():
    PR.need_longdouble()
    c = PR.residual_case((7, 7, False, False), 0.0)
    f = PR.residual64(c)
    k = int(np.argmin(np.abs(f)))            # the smallest entry: a norm-relative 1e-13 would not see ten of its ulps
    bad = f.copy()
    bad[k] = f[k] * (1.0 + 64 * PR.U) + 64 * PR.U * 20.0 * c.c_lap
    rejected(PR.check_residual, c, bad, "a small entry moved")
    assert abs(bad[k] - f[k]) <= 1e-13 * np.max(np.abs(f))
    slab = PR.residual_case((5, 1, True, True), 1.0)
    blind = PR.residual_case((5, 1, True, True), 1.0)
    blind.lo = None
    rejected(PR.check_residual, slab, PR.residual64(blind), "the lower ghost line ignored on a one-line slab")


def test_wrong_gershgorin_is_rejected():
    for ns in (1, 2, 3, 33):
        c = PR.residual_case((ns, ns, False, False), 1.0)
        dexp = c.c_exp * np.exp(c.u)
        good = PR.gershgorin64(ns, c.c_lap, dexp)
        d = 4.0 * c.c_lap - dexp
        rad, full = PR.radius64(ns, c.c_lap), ((np.full(ns * ns, c.c_lap) + c.c_lap) + c.c_lap) + c.c_lap   # full: four neighbours everywhere
        with pytest.raises(AssertionError):                # row by row: every edge row has a disc too wide
            PR.same(np.stack([-(d - full), d + full]), np.stack([-(d - rad), d + rad]), "a radius that counts a neighbour outside the grid")
        if ns <= 2:                                        # no interior row: the reduced pair is wrong as well
            with pytest.raises(AssertionError):
                PR.same((float(np.max(-(d - full))), float(np.max(d + full))), good, "the same, reduced")
    assert PR.radius64(1, 5.0).tolist() == [0.0] and sorted(PR.radius64(3, 1.0).tolist()) == [2.0] * 4 + [3.0] * 4 + [4.0]


# ------------------------------------------------------------------------------------------------ wrong Brusselators
def test_forcing_with_the_local_line_is_rejected():
    for shape in [s for s in PR.BRUS_SLABS if s[0] == 16 and s[2] in (8, 9, 10)]:
        c = PR.brus_case(shape)
        local = PR.brus_case(shape)
        local.j0 = 0
        with pytest.raises(AssertionError):
            PR.same(PR.brus_residual64(local), PR.brus_residual64(c), f"{PR.brus_id(shape)}: forcing from the local line")


@pytest.mark.parametrize("N", PR.BRUS_COLORED)
def test_merged_colours_are_rejected(N):
    PR.need_longdouble()
    rowptr, col, _, _ = PR.brus_pattern(N)
    n = 2 * N * N
    color = PR.greedy_coloring(n, rowptr, col)
    PR.check_coloring(n, rowptr, col, color, "greedy")
    c = PR.brus_case((N, N, 0, False))
    closed, M = PR.brus_fill64(c)
    PR.check_colored_fill(PR.compress_fill(n, rowptr, col, closed, color), closed, M, 6.0, "a proper colouring")
    merged = color.copy()
    a, b = col[rowptr[0]], col[rowptr[0] + 1]              # two columns that share row 0
    merged[merged == merged[b]] = merged[a]
    rejected(PR.check_coloring, n, rowptr, col, merged, "merged")
    rejected(PR.check_colored_fill, PR.compress_fill(n, rowptr, col, closed, merged), closed, M, 6.0, "two colours merged")


def test_small_periodic_grids_need_many_colours():
    """3 × 3 and 4 × 4: almost every pair of columns shares a row; the greedy count is what the GPU test expects of the library"""
    for N in (3, 4):
        rowptr, col, _, _ = PR.brus_pattern(N)
        color = PR.greedy_coloring(2 * N * N, rowptr, col)
        assert color.max() + 1 >= 6


def test_quadratic_reference():
    for n in PR.QUAD_N:
        c = PR.quad_case(n)
        q = PR.quad64(c)
        assert q["f"].size == n and np.all(q["jac"] == 2.0 * c.u) and np.all(q["jv"] == q["jac"] * c.v)
        assert np.log10(np.max(np.abs(c.u)) / np.min(np.abs(c.u))) >= 6.0 or n == 1
