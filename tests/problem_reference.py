"""Cases, data, references and assertions for the kernels of the built-in problems (csrc/nk_problems.hip), in plain NumPy.
tests/test_gpu_problem_kernels.py hands the device's results to the check_* functions below; tests/test_problem_reference.py
hands them the float64 references and deliberately wrong results, without a GPU.

Two references per operation.

ordered   float64, vectorised, in the kernel's own order of operations. The library is built with -ffp-contract=off and, apart
          from exp, everything is + − × ÷ (and one correctly rounded sqrt) in a fixed order, so the device has to return these
          bits: same().
exact     np.longdouble, the mathematics written as dense index arithmetic over (i, j) with explicit boundary tests — no clamped
          reads, no 0/1 weights, no knowledge of the kernels' order. Together with M_k, the sum of the magnitudes of an entry's
          terms, it carries the entrywise bounds: within().

Roundings (K). A product with 4, 2, 0 or 1 is exact and is not counted.
    Bratu stencil   c_lap·((((4c − w) − e) − s) − n) − d·c       4 subtractions, c_lap·, d·c, the last subtraction      K = 7
    Bratu residual  c_lap·((((4c − w) − e) − s) − n) − c_exp·eᵘ   the same with c_exp·eᵘ in place of d·c                 K = 7
    Bratu diagonal  d = c_exp·eᵘ                                                                                       K = 1
    Bratu fill      4c_lap − c_exp·eᵘ                                                                                  K = 2
    Brusselator F   α·lap + B + u·u·v − (A+1)·u + bf   lap 4, α·, u·u, ·v, A+1, ·u, three additions and a subtraction  K = 13
    Brusselator Jv  os·(α·lap + d11·a + d12·b)   lap 4, α·, d11 2, d12 1, two products, two additions, os·            K = 13
No term passes through more than K − 1 of these roundings, so (1+u)^(K−1) − 1 < K·u covers the second-order terms and the bound
is K·u·M_k with nothing added. The device's exp is not derivable from the source: its error E, in units of u·eᵘ, was measured
(EXP_ULP below) and enters as E·u·c_exp·eᵘ:

    |got − exact| ≤ u·(K·M_k + E·c_exp·exp(u_k))                 residual, diagonal, fill
    |Σ − exact Σ| ≤ n·u·Σ f²                                     a sum of n rounded squares added in any order

Masked neighbours. The kernels read a clamped address for a neighbour outside the grid and multiply by a weight 0.0: the value
read is the point's own (the tiled JVP's missing upper line reads 0.0 instead). The library promises the value for finite data
— there the term is ±0 and these references, which form the same product, agree bit for bit. It does not promise what a point
whose own value is NaN or ±Inf returns beyond "not finite": 0·NaN is NaN either way, 0·Inf is NaN in the one-point kernels and
absent in the tiled one. What it does promise is containment: a non-finite entry reaches its own point and its neighbours inside
the grid, nothing else (check in test_gpu_problem_kernels.py::test_bratu_residual_nan_stays_in_its_workgroups).

Data. "spread": magnitudes 10^x, x uniform, with the two ends of the range planted, so one vector spans at least six decades and
an entrywise check differs from a norm-relative one. "exact": nonzero integers, every operation exact, so the ordered and the
exact reference agree to the bit (test_problem_reference.py asserts it). Ghost lines come from ranges of their own; d, r, dnew
(canary on entry) and yacc are all distinct."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
GUARD = 8
CANARY = np.float64(-6.02214076e23)
NK_BLOCK, TY, MAX_RED_BLOCKS = 256, 4, 1024
# The error of the device's exp in units of u·eᵘ, against long-double expl over every argument the tests pass to the residual,
# the diagonal and the fill (exp_arguments()): measured maximum 1.2392 on the MI355X, at u = 4.4531, over 1 601 297 arguments in
# [−5.01, 5.01] (NumPy's exp on the same arguments: 1.1758). ceil(1.2392) + 1 = 3:
# the extra unit is for arguments the measurement did not visit.
EXP_ULP = 3
K_STENCIL, K_RESIDUAL, K_DIAG, K_FILL, K_BRUS = 7, 7, 1, 2, 13


def need_longdouble():
    if not LONGDOUBLE_OK:
        import pytest
        pytest.skip("np.longdouble has fewer than 64 significand bits on this machine")


def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def canary(n):
    return np.full(n, CANARY)


# ------------------------------------------------------------------------------------------------------------- assertions
def same(got, want, what):
    """equal bits"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)).ravel(), np.atleast_1d(np.asarray(want, dtype=np.float64)).ravel()
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} entries differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def within(got, exact, bound, what):
    """entrywise |got − exact| ≤ bound, in long double; prints the worst ratio"""
    err = np.abs(_ld(np.ravel(got)) - np.ravel(exact))
    bound = np.ravel(_ld(bound))
    ok = err <= bound                        # (a NaN fails)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))) if err.size else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}")
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{what}: {bad.size} of {err.size} entries outside the bound, first at {bad[0]}: error {float(err[bad[0]]):.3e}"
                           f" > {float(bound[bad[0]]):.3e}")


def untouched(got, what):
    same(got, canary(np.size(got)), what + " must keep its canary")


# ------------------------------------------------------------------------------------------------------------------- data
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def spread(rng, n, lo=-3.0, hi=3.0):
    """magnitudes 10^[lo, hi] with random signs; the smallest planted first, the largest last (n ≥ 2)"""
    x = rng.choice(np.array([-1.0, 1.0]), size=n) * 10.0 ** rng.uniform(lo, hi, size=n)
    if n >= 2:
        x[0], x[-1] = math.copysign(10.0 ** lo, x[0]), math.copysign(10.0 ** hi, x[-1])
    return x


def ints(rng, n, a=1, b=8):
    return rng.choice(np.array([-1.0, 1.0]), size=n) * rng.integers(a, b + 1, size=n).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ Bratu: cases
WHOLE_NS = [1, 2, 3, 4, 5, 6, 7, 255, 256, 257, 513]
SLAB_SHAPES = [(ns, nl) for ns in (5, 257) for nl in (1, 2, 3, 4, 5, 7)]   # (a slab's shape is free: 5 × 7 is one, with ghost lines)
SLABS = [(ns, nl, lo, hi) for ns, nl in SLAB_SHAPES for lo in (False, True) for hi in (False, True)]
BRATU_SHAPES = [(ns, ns, False, False) for ns in WHOLE_NS] + SLABS
MODES = (0, 1, 2, 3)


def shape_id(s):
    ns, nl, lo, hi = s
    return f"{ns}x{nl}" + ("+lo" if lo else "") + ("+hi" if hi else "")


def bratu_coefficients(ns, lam, scale):
    """nk_problems.hip: bratu_coefficients, float64, the same operations"""
    h = 1.0 / float(ns + 1)
    s = h * h if scale == 0.0 else scale
    return s / (h * h), s * lam


def jvp_case(shape, kind):
    """operands of one Bratu JVP launch on a slab; `kind` "spread" or "exact" """
    ns, nl, lo, hi = shape
    rng, n = _rng("bratu_jvp", shape, kind), ns * nl
    c = SimpleNamespace(ns=ns, nl=nl, kind=kind)
    if kind == "exact":
        c.c_lap, c.c1, c.c2, c.theta, c.out_scale = 3.0, -2.0, 5.0, 3.0, 2.0
        c.d, c.v, c.r, c.yacc = ints(rng, n), ints(rng, n), ints(rng, n, 9, 16), ints(rng, n, 17, 24)
        c.lo, c.hi = (ints(rng, ns, 25, 32) if lo else None), (ints(rng, ns, 33, 40) if hi else None)
    else:
        c.c_lap, c.c1, c.c2, c.theta, c.out_scale = float((ns + 1) ** 2) / 7.0, 0.37, -1.9, 0.83, 1.7
        c.d, c.v, c.r, c.yacc = spread(rng, n, -2, 4), spread(rng, n), spread(rng, n, -1, 5), spread(rng, n, -4, 2)
        c.lo, c.hi = (spread(rng, ns, 0, 6) if lo else None), (spread(rng, ns, -6, 0) if hi else None)
    return c


def residual_case(shape, scale):
    """u with magnitudes 10^[−6, 0.7]: six decades and more, and eᵘ ≤ 151"""
    ns, nl, lo, hi = shape
    rng = _rng("bratu_residual", shape)
    c = SimpleNamespace(ns=ns, nl=nl, lam=6.0, scale=scale)
    c.u = spread(rng, ns * nl, -6.0, 0.7)
    c.lo, c.hi = (spread(rng, ns, -5.0, 0.6) if lo else None), (spread(rng, ns, -4.0, 0.5) if hi else None)
    c.c_lap, c.c_exp = bratu_coefficients(ns, c.lam, scale)
    return c


GERSH_NS = [1, 2, 3, 33, 257]
FILL_NS = [1, 2, 3, 16, 17, 257]
BIG_NS = 1025        # 1025² points: the residual's grid is capped at 1024 workgroups and a thread makes a second trip


def exp_arguments():
    """every u the GPU tests pass through the device's exp"""
    out = [residual_case(s, 0.0).u for s in BRATU_SHAPES]
    out += [residual_case((ns, ns, False, False), 0.0).u for ns in sorted(set(GERSH_NS + FILL_NS))]
    out.append(residual_case((BIG_NS, BIG_NS, False, False), 0.0).u)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------ Bratu: the ordered references
def _neighbours(x, lo, hi, tiled):
    """(w, e, s, n, mw, me, ms, mn) as the kernels read them: clamped addresses, 0/1 weights. x: (nl, ns)"""
    nl, ns = x.shape
    i = np.arange(ns)
    w, e = x[:, np.maximum(i - 1, 0)], x[:, np.minimum(i + 1, ns - 1)]
    s = np.vstack([(lo if lo is not None else x[0])[None, :], x[:-1]])
    top = hi if hi is not None else (np.zeros(ns) if tiled else x[-1])
    n = np.vstack([x[1:], top[None, :]])
    mw, me = (i > 0).astype(np.float64)[None, :], (i < ns - 1).astype(np.float64)[None, :]
    jl = np.arange(nl)[:, None]
    ms = ((jl > 0) | (lo is not None)).astype(np.float64) * np.ones((1, ns))
    mn = ((jl < nl - 1) | (hi is not None)).astype(np.float64) * np.ones((1, ns))
    return w, e, s, n, mw, me, ms, mn


def stencil64(ns, nl, c_lap, d, v, lo=None, hi=None, tiled=True):
    """c_lap·((((4c − mw·w) − me·e) − ms·s) − mn·n) − d·c, float64, this order"""
    x, d = np.asarray(v, dtype=np.float64).reshape(nl, ns), np.asarray(d, dtype=np.float64).reshape(nl, ns)
    w, e, s, n, mw, me, ms, mn = _neighbours(x, lo, hi, tiled)
    with np.errstate(all="ignore"):
        return (c_lap * ((((4.0 * x - mw * w) - me * e) - ms * s) - mn * n) - d * x).ravel()


def epilogue64(c, res, mode, scaled):
    """what the launch leaves in jv, r, dnew, yacc (the hook hands dnew and jv over as canary)"""
    os = c.out_scale if scaled else 1.0
    out = dict(jv=canary(res.size), r=c.r.copy(), dnew=canary(res.size), yacc=c.yacc.copy())
    if mode == 0:
        out["jv"] = os * res
    elif mode == 3:
        out["jv"] = os * (res - c.theta * c.v)
    elif mode == 2:
        out["jv"] = c.r - res                              # (no output scale in this mode)
    elif mode == 1:
        out["r"] = c.r - res
        out["dnew"] = c.c1 * c.v + c.c2 * out["r"]
        out["yacc"] = c.yacc + out["dnew"]
    else:
        raise ValueError(mode)
    return out


def jvp64(c, mode, scaled):
    return epilogue64(c, stencil64(c.ns, c.nl, c.c_lap, c.d, c.v, c.lo, c.hi), mode, scaled)


def check_jvp(c, mode, scaled, got, what, skip=False):
    """got: dict(jv, r, dnew, yacc) as the hook delivered them. With skip every output keeps what it held."""
    want = jvp64(c, mode, scaled)
    if skip:
        want = dict(jv=canary(c.v.size), r=c.r, dnew=canary(c.v.size), yacc=c.yacc)
    for k in ("jv", "r", "dnew", "yacc"):
        same(got[k], want[k], f"{what}: {k}")


def residual64(c, exp=np.exp):
    x = c.u.reshape(c.nl, c.ns)
    w, e, s, n, mw, me, ms, mn = _neighbours(x, c.lo, c.hi, tiled=False)
    with np.errstate(all="ignore"):
        return (c.c_lap * ((((4.0 * x - mw * w) - me * e) - ms * s) - mn * n) - c.c_exp * exp(x)).ravel()


def radius64(ns, c_lap):
    """the Gershgorin radius of every row of a whole grid: c_lap added once per neighbour in S, W, E, N order"""
    j, i = np.divmod(np.arange(ns * ns), ns)
    rad = np.zeros(ns * ns)
    for present in (j > 0, i > 0, i < ns - 1, j < ns - 1):
        rad = rad + np.where(present, c_lap, 0.0)
    return rad


def gershgorin64(ns, c_lap, dexp):
    """{max −(d − rad), max (d + rad)} with d = 4c_lap − dexp, dexp = the device's own c_exp·eᵘ"""
    d, rad = 4.0 * c_lap - np.asarray(dexp), radius64(ns, c_lap)
    return float(np.max(-(d - rad))), float(np.max(d + rad))


def interval64(c_lap, dexp):
    return float(np.max(dexp)), float(8.0 * c_lap + np.max(-np.asarray(dexp)))


def bratu_pattern(ns):
    """rowptr, col, and the position of every row's diagonal, in the library's order [S][W][C][E][N]"""
    j, i = np.divmod(np.arange(ns * ns), ns)
    k = np.arange(ns * ns)
    present = np.stack([j > 0, i > 0, np.ones_like(k, dtype=bool), i < ns - 1, j < ns - 1], axis=1)
    cols = np.stack([k - ns, k - 1, k, k + 1, k + ns], axis=1)
    rowptr = np.concatenate([[0], np.cumsum(present.sum(axis=1))])
    diagpos = rowptr[:-1] + present[:, :2].sum(axis=1)
    return rowptr, cols[present], diagpos


def check_bratu_fill(ns, c, vals, what, colored=False, closed=None):
    """off-diagonals −c_lap exactly (both fills); the closed-form diagonal within u·(K_FILL·M + E·c_exp·eᵘ) of 4c_lap − c_exp·eᵘ;
    the coloured fill within 4u·M_k of the closed-form one. No stored position keeps the canary."""
    rowptr, col, diagpos = bratu_pattern(ns)
    assert vals.size == col.size, f"{what}: {vals.size} values for {col.size} pattern positions"
    assert not np.any(bits(vals) == bits(CANARY)), f"{what}: a stored position was not written"
    off = np.ones(vals.size, dtype=bool)
    off[diagpos] = False
    same(vals[off], np.full(int(off.sum()), -c.c_lap), f"{what}: off-diagonals")
    eu = np.exp(_ld(c.u))
    M = 4.0 * c.c_lap + c.c_exp * eu
    if colored:
        within(vals[diagpos], _ld(closed[diagpos]), 4.0 * U * M, f"{what}: diagonal against the closed-form fill")
    else:
        within(vals[diagpos], 4.0 * _ld(c.c_lap) - _ld(c.c_exp) * eu, U * (K_FILL * M + EXP_ULP * c.c_exp * eu), f"{what}: diagonal")


# -------------------------------------------------------------------------------------------- Bratu: the exact references
def stencil_exact(ns, nl, c_lap, d, v, lo=None, hi=None):
    """(c_lap·L v − d.*v, M) in long double: L from index arithmetic over (i, jl), a neighbour counts when it lies inside the
    line (0 ≤ i' < ns) and inside the slab or on a ghost line that exists"""
    x, dd = _ld(v).reshape(nl, ns), _ld(d).reshape(nl, ns)
    jl, i = np.meshgrid(np.arange(nl), np.arange(ns), indexing="ij")
    acc, mag = 4 * x, 4 * np.abs(x)
    for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ii, jj = i + di, jl + dj
        val = np.zeros_like(x)
        inside = (ii >= 0) & (ii < ns) & (jj >= 0) & (jj < nl)
        val[inside] = x[jj[inside], ii[inside]]
        if lo is not None:
            below = jj < 0
            val[below] = _ld(lo)[ii[below]]
        if hi is not None:
            above = jj >= nl
            val[above] = _ld(hi)[ii[above]]
        acc, mag = acc - val, mag + np.abs(val)
    cl = np.longdouble(c_lap)
    return (cl * acc - dd * x).ravel(), (abs(cl) * mag + np.abs(dd * x)).ravel()


def residual_exact(c):
    """(F, M, c_exp·eᵘ) in long double"""
    lap, mag = stencil_exact(c.ns, c.nl, c.c_lap, np.zeros(c.u.size), c.u, c.lo, c.hi)
    ce = np.longdouble(c.c_exp) * np.exp(_ld(c.u))
    return lap - ce, mag + ce, ce


def check_residual(c, f, what):
    F, M, ce = residual_exact(c)
    within(f, F, U * (K_RESIDUAL * M + EXP_ULP * ce), what)


def check_diag(c, dexp, what):
    ce = np.longdouble(c.c_exp) * np.exp(_ld(c.u))
    within(dexp, ce, U * (K_DIAG + EXP_ULP) * ce, what)


# ------------------------------------------------------------------------------------------- the residual's fused partials
def red_grid(n):
    return max(1, min((n + 4 * NK_BLOCK - 1) // (4 * NK_BLOCK), MAX_RED_BLOCKS))


def block_of(k, grid):
    """the workgroup that visits entry k"""
    return (np.asarray(k) % (grid * NK_BLOCK)) // NK_BLOCK


def _nanmax(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, b))


def partials64(f, grid, final=lambda s: (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3]), extra_last=False):
    """k_absmax_sumsq's stage-1 results for f on `grid` workgroups, float64 in its order: a thread adds its entries g, g + stride, …
    in ascending order; 64 lanes combine in an xor butterfly (offsets 32 … 1); the four wavefronts as (w0 + w1) + (w2 + w3).
    `final` and `extra_last` exist for test_problem_reference.py's wrong results."""
    n, stride = f.size, grid * NK_BLOCK
    trips = (n + stride - 1) // stride
    pad = np.zeros(trips * stride)
    pad[:n] = f
    live = np.arange(trips * stride).reshape(trips, stride) < n
    m, s = np.zeros(stride), np.zeros(stride)
    with np.errstate(all="ignore"):
        for t in range(trips):
            v = pad[t * stride:(t + 1) * stride]
            m = np.where(live[t], _nanmax(m, np.abs(v)), m)
            s = np.where(live[t], s + v * v, s)
        if extra_last:                      # the thread that would visit entry n counts entry n − 1 once more
            s[n % stride] = s[n % stride] + f[-1] * f[-1]
        m, s = m.reshape(grid, 4, 64), s.reshape(grid, 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            m, s = _nanmax(m, m[:, :, lane ^ o]), s + s[:, :, lane ^ o]
        m, s = m[:, :, 0], s[:, :, 0]
        return np.concatenate([_nanmax(_nanmax(m[:, 0], m[:, 1]), _nanmax(m[:, 2], m[:, 3])), final(s)])


def check_partials(f, grid, partials, what, bitwise=True):
    """partials: 2·grid doubles. Equal bits with the ordered emulation; max of the first half = max |f|; Σ of the second half
    within n·u·Σf² of the long-double sum of f's squares."""
    assert grid == red_grid(f.size), f"{what}: {grid} workgroups, expected {red_grid(f.size)}"
    if bitwise:
        same(partials, partials64(f, grid), f"{what}: partials")
    same(np.max(partials[:grid]), np.max(np.abs(f)), f"{what}: max of the max partials")
    exact = np.sum(_ld(f) * _ld(f))
    within(np.sum(_ld(partials[grid:2 * grid])), exact, f.size * U * exact, f"{what}: sum of the sum partials")


# ------------------------------------------------------------------------------------------------------------- Brusselator
BRUS_WHOLE = [3, 4, 5, 8, 11, 257]       # 11: x = 0.3 is a grid coordinate, points lie exactly on the forcing disc's rim
BRUS_SLABS = ([(5, nl, j0, g) for nl in (1, 2, 3) for j0 in sorted({0, 2, 5 - nl}) for g in (False, True)]
              + [(16, nl, j0, g) for nl in (1, 2, 3) for j0 in sorted({0, 8, 9, 10, 16 - nl}) for g in (False, True)])
BRUS_SHAPES = [(N, N, 0, False) for N in BRUS_WHOLE] + BRUS_SLABS
BRUS_COLORED = [3, 4, 5, 8]


def brus_id(s):
    N, nl, j0, g = s
    return f"{N}x{nl}@{j0}" + ("+ghost" if g else "")


def brus_case(shape, kind="spread"):
    N, nl, j0, ghost = shape
    rng, nn = _rng("brus", shape, kind), N * nl
    c = SimpleNamespace(N=N, nl=nl, j0=j0, kind=kind, out_scale=1.7)
    if kind == "exact":
        c.A, c.B, c.alpha, c.dx, c.out_scale = 3.0, 2.0, 8.0, 0.5, 2.0
        c.U, c.V = ints(rng, 2 * nn, 1, 4), ints(rng, 2 * nn)
        c.lo, c.hi = (ints(rng, 2 * N, 9, 12), ints(rng, 2 * N, 13, 16)) if ghost else (None, None)
    else:
        c.A, c.B, c.alpha, c.dx = 3.4, 1.0, 10.0, 1.0 / (N - 1)
        c.U, c.V = spread(rng, 2 * nn, -3, 3), spread(rng, 2 * nn, -3, 3)
        if kind == "state":                  # a state a solve visits (whole grids): the initial guess, perturbed; V still spread
            c.U = brus_u0_64(N) + 0.1 * rng.uniform(-1.0, 1.0, size=2 * nn)
        c.lo, c.hi = (spread(rng, 2 * N, -2, 4), spread(rng, 2 * N, -4, 2)) if ghost else (None, None)
    return c


def brus_forcing(N, lines):
    """5 inside the disc of radius 0.1 about (0.3, 0.6), float64 in the kernel's order; `lines`: the GLOBAL grid lines"""
    x, y = (np.arange(N).astype(np.float64) / float(N - 1))[None, :], (np.asarray(lines).astype(np.float64) / float(N - 1))[:, None]
    return np.where(((x - 0.3) * (x - 0.3) + (y - 0.6) * (y - 0.6)) <= 0.1 * 0.1, 5.0, 0.0)


def _brus_lap64(w, lo, hi):
    """(w[im1] + w[ip1] − 4w[c]), then the upper neighbour, then the lower one; without ghost lines the slab wraps onto itself"""
    nl, N = w.shape
    i = np.arange(N)
    up = np.vstack([w[1:], (hi if hi is not None else w[0])[None, :]])
    down = np.vstack([(lo if lo is not None else w[-1])[None, :], w[:-1]])
    return ((w[:, (i - 1) % N] + w[:, (i + 1) % N] - 4.0 * w) + up) + down


def _halves(a, N):
    return (None, None) if a is None else (a[:N], a[N:])


def brus_residual64(c):
    N, nl, nn = c.N, c.nl, c.N * c.nl
    al = c.alpha / (c.dx * c.dx)
    u, v = c.U[:nn].reshape(nl, N), c.U[nn:].reshape(nl, N)
    (lo0, lo1), (hi0, hi1) = _halves(c.lo, N), _halves(c.hi, N)
    bf = brus_forcing(N, c.j0 + np.arange(nl))
    f0 = al * _brus_lap64(u, lo0, hi0) + c.B + u * u * v - (c.A + 1.0) * u + bf
    f1 = al * _brus_lap64(v, lo1, hi1) + c.A * u - u * u * v
    return np.concatenate([f0.ravel(), f1.ravel()])


def brus_jvp64(c, transpose, scaled):
    N, nl, nn = c.N, c.nl, c.N * c.nl
    al, os = c.alpha / (c.dx * c.dx), (c.out_scale if scaled else 1.0)
    u, v = c.U[:nn].reshape(nl, N), c.U[nn:].reshape(nl, N)
    a, b = c.V[:nn].reshape(nl, N), c.V[nn:].reshape(nl, N)
    (lo0, lo1), (hi0, hi1) = _halves(c.lo, N), _halves(c.hi, N)
    la, lb = al * _brus_lap64(a, lo0, hi0), al * _brus_lap64(b, lo1, hi1)
    d11, d12, d21, d22 = 2.0 * u * v - (c.A + 1.0), u * u, c.A - 2.0 * u * v, -(u * u)
    if not transpose:
        o0, o1 = os * (la + d11 * a + d12 * b), os * (lb + d21 * a + d22 * b)
    else:
        o0, o1 = os * (la + d11 * a + d21 * b), os * (lb + d12 * a + d22 * b)
    return np.concatenate([o0.ravel(), o1.ravel()])


def _brus_lap_exact(w, lo, hi):
    """(Σ of the four periodic neighbours − 4w, Σ magnitudes) by index arithmetic: the neighbour of line jl in direction ±1 is the
    ghost line when it leaves the slab and a ghost line exists, the slab's other end otherwise"""
    nl, N = w.shape
    jl, i = np.meshgrid(np.arange(nl), np.arange(N), indexing="ij")
    acc, mag = -4 * w, 4 * np.abs(w)
    for di, dj in ((-1, 0), (1, 0), (0, 1), (0, -1)):
        ii, jj = (i + di) % N, jl + dj
        ghost = hi if dj > 0 else lo
        out = (jj < 0) | (jj >= nl)
        val = w[jj % nl, ii]
        if dj != 0 and ghost is not None:
            val = np.where(out, _ld(ghost)[ii], val)
        acc, mag = acc + val, mag + np.abs(val)
    return acc, mag


def brus_exact(c, op, scaled=False):
    """(result, M) in long double. op 0: F(U); 1: J(U)·V; 2: J(U)ᵀ·V. The forcing is taken from brus_forcing(): which side of the
    rim a point lies on is a float64 decision by definition."""
    N, nl, nn = c.N, c.nl, c.N * c.nl
    A, B, al = np.longdouble(c.A), np.longdouble(c.B), np.longdouble(c.alpha) / (np.longdouble(c.dx) * np.longdouble(c.dx))
    u, v = _ld(c.U[:nn]).reshape(nl, N), _ld(c.U[nn:]).reshape(nl, N)
    (lo0, lo1), (hi0, hi1) = _halves(c.lo, N), _halves(c.hi, N)
    if op == 0:
        bf = _ld(brus_forcing(N, c.j0 + np.arange(nl)))
        l0, m0 = _brus_lap_exact(u, lo0, hi0)
        l1, m1 = _brus_lap_exact(v, lo1, hi1)
        r0, r1 = al * l0 + B + u * u * v - (A + 1) * u + bf, al * l1 + A * u - u * u * v
        M0 = al * m0 + abs(B) + np.abs(u * u * v) + (abs(A) + 1) * np.abs(u) + bf
        M1 = al * m1 + np.abs(A * u) + np.abs(u * u * v)
    else:
        os = np.longdouble(c.out_scale if scaled else 1.0)
        a, b = _ld(c.V[:nn]).reshape(nl, N), _ld(c.V[nn:]).reshape(nl, N)
        l0, m0 = _brus_lap_exact(a, lo0, hi0)
        l1, m1 = _brus_lap_exact(b, lo1, hi1)
        j11, j12, j21, j22 = 2 * u * v - (A + 1), u * u, A - 2 * u * v, -u * u
        m11, m21 = 2 * np.abs(u * v) + abs(A) + 1, abs(A) + 2 * np.abs(u * v)
        if op == 2:
            j12, j21 = j21, j12
            m12, m21 = m21, np.abs(u * u)
        else:
            m12 = np.abs(u * u)
        r0, r1 = os * (al * l0 + j11 * a + j12 * b), os * (al * l1 + j21 * a + j22 * b)
        M0 = abs(os) * (al * m0 + m11 * np.abs(a) + m12 * np.abs(b))
        M1 = abs(os) * (al * m1 + m21 * np.abs(a) + np.abs(u * u) * np.abs(b))
    return np.concatenate([r0.ravel(), r1.ravel()]), np.concatenate([M0.ravel(), M1.ravel()])


def brus_pattern(N):
    """(rowptr, col, role, node) of a whole grid on one rank: six entries per row, columns ascending. Roles: 0 α · 1 ∂F1/∂u ·
    2 ∂F1/∂v · 3 ∂F2/∂v · 4 ∂F2/∂u"""
    j, i = np.divmod(np.arange(N * N), N)
    cols, roles = [], []
    for s in (0, 1):
        idx = lambda ii, jj, ss: ii + N * jj + N * N * ss
        cc = np.stack([idx((i - 1) % N, j, s), idx((i + 1) % N, j, s), idx(i, (j + 1) % N, s), idx(i, (j - 1) % N, s),
                       idx(i, j, s), idx(i, j, 1 - s)], axis=1)
        rr = np.tile(np.array([0, 0, 0, 0, 1 if s == 0 else 3, 2 if s == 0 else 4]), (N * N, 1))
        order = np.argsort(cc, axis=1, kind="stable")
        cols.append(np.take_along_axis(cc, order, axis=1))
        roles.append(np.take_along_axis(rr, order, axis=1))
    col, role = np.vstack(cols).ravel(), np.vstack(roles).ravel()
    node = np.repeat(np.tile(np.arange(N * N), 2), 6)
    return np.arange(0, 6 * 2 * N * N + 1, 6), col, role, node


def brus_fill64(c):
    """(values, M) of the closed-form fill in the kernel's order, per stored position of brus_pattern"""
    N = c.N
    _, _, role, node = brus_pattern(N)
    al = c.alpha / (c.dx * c.dx)
    u, v = c.U[:N * N][node], c.U[N * N:][node]
    vals = np.select([role == 0, role == 1, role == 2, role == 3],
                     [np.full(u.size, al), -4.0 * al + 2.0 * u * v - (c.A + 1.0), u * u, -4.0 * al - u * u], c.A - 2.0 * u * v)
    uv, uu = np.abs(_ld(u) * _ld(v)), _ld(u) * _ld(u)
    M = np.select([role == 0, role == 1, role == 2, role == 3],
                  [np.full(u.size, _ld(al)), 4 * _ld(al) + 2 * uv + abs(c.A) + 1, uu, 4 * _ld(al) + uu], abs(c.A) + 2 * uv)
    return vals, M


def brus_u0_64(N):
    x, y = np.arange(N).astype(np.float64) / float(N - 1), (np.arange(N).astype(np.float64) / float(N - 1))[:, None]
    a, b = y * (1.0 - y) * np.ones((1, N)), (x * (1.0 - x))[None, :] * np.ones((N, 1))
    return np.concatenate([(22.0 * a * np.sqrt(a)).ravel(), (27.0 * b * np.sqrt(b)).ravel()])


def within_ulps(got, want, ulps, what):
    d = np.abs(bits(got) - bits(want))       # (same sign, finite: the bit patterns are ordered like the values)
    print(f"{what}: largest distance {int(d.max())} ulp, {int(np.count_nonzero(d))} of {d.size} entries differ")
    assert d.max() <= ulps, f"{what}: {int(d.max())} ulp apart"


# --------------------------------------------------------------------------------------------------------------- colouring
def greedy_coloring(n, rowptr, col):
    """greedy distance-2 column colouring in natural order (columns that share a row get different colours): the library's
    greedy_column_coloring, written with sets"""
    rows_of = [[] for _ in range(n)]
    for r in range(n):
        for p in range(rowptr[r], rowptr[r + 1]):
            rows_of[col[p]].append(r)
    color = np.full(n, -1)
    for c in range(n):
        taken = {color[col[p]] for r in rows_of[c] for p in range(rowptr[r], rowptr[r + 1])}
        k = 0
        while k in taken:
            k += 1
        color[c] = k
    return color


def check_coloring(n, rowptr, col, color, what):
    """no two columns of one colour share a row"""
    for r in range(n):
        cs = color[col[rowptr[r]:rowptr[r + 1]]]
        assert np.unique(cs).size == cs.size, f"{what}: row {r} stores two columns of one colour"


def compress_fill(n, rowptr, col, vals, color):
    """what colour-compressed assembly returns for a matrix with these values if `color` is used: B[:, c] = Σ of the columns of
    colour c, vals[p] = B[row(p), colour(col(p))]"""
    ncol = int(color.max()) + 1
    B = np.zeros((n, ncol), dtype=vals.dtype)
    rowof = np.repeat(np.arange(n), np.diff(rowptr))
    np.add.at(B, (rowof, color[col]), vals)
    return B[rowof, color[col]]


def check_colored_fill(vals, closed, M, factor, what):
    assert not np.any(bits(vals) == bits(CANARY)), f"{what}: a stored position was not written"
    within(vals, _ld(closed), factor * U * _ld(M), what)


# --------------------------------------------------------------------------------------------------------------- quadratic
QUAD_N = [1, 255, 256, 257]


def quad_case(n):
    rng = _rng("quad", n)
    return SimpleNamespace(n=n, p=2.0, u=spread(rng, n), v=spread(rng, n, -2, 4))


def quad64(c):
    return dict(f=c.u * c.u - c.p, jv=2.0 * c.u * c.v, jac=2.0 * c.u)
