"""The kernels of the built-in problems (csrc/nk_problems.hip) on their own, through the development hooks nk_bratu_jvp_test,
nk_bratu_residual_test, nk_bratu_linearisation_test and nk_brus_test and through the public entry points, against
tests/problem_reference.py. Every hook reaches its kernel through the launch function the production path uses; every device
buffer of a hook lies between guard words it inspects, and its outputs start as canary.

Every assertion is bit equality with a float64 evaluation in the kernel's order, or — where exp is involved — an entrywise bound
against a long-double evaluation of the mathematics (derivations in problem_reference.py). No norm-relative tolerance.

Out of scope here: the fold / begin arguments of k_bratu_jac (the s-step cycle: test_gpu_round2.py, test_gpu_sstep.py), the peer
halo exchange itself (the slab hooks take the ghost lines as arguments), the finite-difference JVP (test_gpu_solvers.py), the
compiled problem kinds."""
import ctypes as C
import functools

import numpy as np
import pytest

import problem_reference as PR

pytestmark = pytest.mark.gpu

KINDS = ("spread", "exact")


@functools.lru_cache(maxsize=None)
def _hooks():
    """development hooks: exported, not in the public header, so not in _lib.SIGNATURES"""
    from nonlinearsolve_jl_amd import _lib as L
    lib = L.lib()
    D, P, I, I64 = C.c_double, C.c_void_p, C.c_int, C.c_int64
    lib.nk_bratu_jvp_test.restype = I
    lib.nk_bratu_jvp_test.argtypes = [P, I64, I64, D, P, P, P, P, I, P, P, P, D, D, D, P, I, P]
    lib.nk_bratu_residual_test.restype = I
    lib.nk_bratu_residual_test.argtypes = [P, I64, I64, D, D, P, P, P, I, P, P, P, P, P, P, C.POINTER(I)]
    lib.nk_bratu_linearisation_test.restype = I
    lib.nk_bratu_linearisation_test.argtypes = [P, P, P, P]
    lib.nk_brus_test.restype = I
    lib.nk_brus_test.argtypes = [P, I64, I64, I64, D, D, D, D, P, P, P, P, I, P, I, P]
    lib.nk_csr_gershgorin_test.restype = I
    lib.nk_csr_gershgorin_test.argtypes = [P, P]
    return lib, L.check


def _p(a):
    return None if a is None else a.ctypes.data


def _ctx(nls):
    return nls.default_context()._h


def _jvp(nls, c, mode, scaled, skip=0):
    """one nk_bratu_jvp_test call: dict(jv, r, dnew, yacc) as the launch left them"""
    lib, check = _hooks()
    n = c.v.size
    out = dict(jv=PR.canary(n), r=c.r.copy(), dnew=PR.canary(n), yacc=c.yacc.copy())
    os = np.array([c.out_scale]) if scaled else None
    check(lib.nk_bratu_jvp_test(_ctx(nls), c.ns, c.nl, c.c_lap, _p(c.d), _p(c.v), _p(c.lo), _p(c.hi), mode, _p(out["r"]), _p(out["dnew"]),
                                _p(out["yacc"]), c.c1, c.c2, c.theta, _p(os), skip, _p(out["jv"])))
    return out


def _residual(nls, c, fused):
    """one nk_bratu_residual_test call: f, or a namespace with everything the fused launch leaves"""
    lib, check = _hooks()
    n, nb = c.u.size, PR.MAX_RED_BLOCKS
    f = PR.canary(n)
    if not fused:
        check(lib.nk_bratu_residual_test(_ctx(nls), c.ns, c.nl, c.lam, c.scale, _p(c.u), _p(c.lo), _p(c.hi), 0, _p(f), None, None, None,
                                         None, None, None))
        return f
    from types import SimpleNamespace
    o = SimpleNamespace(f=f, f_copy=PR.canary(n), partials=PR.canary(2 * nb), ss_copy=PR.canary(nb), gpart=PR.canary(2 * nb),
                        partials_ref=PR.canary(2 * nb))
    grid = C.c_int(-1)
    check(lib.nk_bratu_residual_test(_ctx(nls), c.ns, c.nl, c.lam, c.scale, _p(c.u), _p(c.lo), _p(c.hi), 1, _p(o.f), _p(o.f_copy),
                                     _p(o.partials), _p(o.ss_copy), _p(o.gpart), _p(o.partials_ref), C.byref(grid)))
    o.grid = grid.value
    return o


def _linearisation(P, u):
    lib, check = _hooks()
    diag, interval = PR.canary(u.size), PR.canary(2)
    check(lib.nk_bratu_linearisation_test(P._h, _p(u), _p(diag), _p(interval)))
    return diag, interval


def _gersh(A):
    lib, check = _hooks()
    out = np.zeros(2)
    check(lib.nk_csr_gershgorin_test(A._h, _p(out)))
    return out


def _brus(nls, c, op, scaled=False, skip=0):
    lib, check = _hooks()
    out = PR.canary(c.U.size)
    os = np.array([c.out_scale]) if scaled else None
    check(lib.nk_brus_test(_ctx(nls), c.N, c.nl, c.j0, c.A, c.B, c.alpha, c.dx, _p(c.U), _p(c.V), _p(c.lo), _p(c.hi), op, _p(os), skip,
                           _p(out)))
    return out


# ------------------------------------------------------------------------------------------------------------- Bratu JVP
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PR.BRATU_SHAPES, ids=PR.shape_id)
def test_bratu_jvp(nls, shape, kind):
    """k_bratu_jvp_tile<4>, modes 0 … 3, with and without out_scale, and with the skip flag set: equal bits, the untouched outputs
    their canary. Whole grids: every residue of nl mod 4, the degenerate stencils, the NK_BLOCK column edge, three column blocks.
    Slabs: every combination of ghost lines, nl = 1 included."""
    c = PR.jvp_case(shape, kind)
    for mode in PR.MODES:
        for scaled in (False, True):
            PR.check_jvp(c, mode, scaled, _jvp(nls, c, mode, scaled), f"{PR.shape_id(shape)} {kind} mode {mode} scaled {scaled}")
        PR.check_jvp(c, mode, False, _jvp(nls, c, mode, False, skip=1), f"{PR.shape_id(shape)} {kind} mode {mode} skip", skip=True)


@pytest.mark.parametrize("mode", [4, -1, 5])
def test_bratu_jvp_refuses_an_unknown_epilogue(nls, mode):
    """NK_EPI_RESIDUAL_UPDATE is the CSR kernel's alone: an error, and nothing launched — every output keeps what it held"""
    from nonlinearsolve_jl_amd import _lib as L
    lib, check = _hooks()
    c = PR.jvp_case((5, 5, False, False), "spread")
    n = c.v.size
    out = dict(jv=PR.canary(n), r=c.r.copy(), dnew=PR.canary(n), yacc=c.yacc.copy())
    with pytest.raises(L.NKError, match="row epilogue"):
        check(lib.nk_bratu_jvp_test(_ctx(nls), c.ns, c.nl, c.c_lap, _p(c.d), _p(c.v), None, None, mode, _p(out["r"]), _p(out["dnew"]),
                                    _p(out["yacc"]), c.c1, c.c2, c.theta, None, 0, _p(out["jv"])))
    PR.check_jvp(c, 0, False, out, f"mode {mode}", skip=True)


@pytest.mark.parametrize("ns", PR.WHOLE_NS)
def test_bratu_public_jvp_equals_the_hook(nls, ns):
    """nk_jvp / nk_vjp on a whole grid = the hook's mode 0 with d from the diagonal hook = the ordered reference on that d"""
    shape = (ns, ns, False, False)
    c, r = PR.jvp_case(shape, "spread"), PR.residual_case(shape, 0.0)
    P = nls.Bratu2D(ns, r.lam, r.scale)
    diag, _ = _linearisation(P, r.u)
    PR.check_diag(r, diag, f"{ns}: diagonal")
    c.d, c.c_lap = diag, r.c_lap
    hook = _jvp(nls, c, 0, False)["jv"]
    PR.same(hook, PR.stencil64(ns, ns, c.c_lap, diag, c.v), f"{ns}: hook against the ordered reference")
    PR.same(P.jvp(c.v, r.u), hook, f"{ns}: nk_jvp against the hook")
    PR.same(P.vjp(c.v, r.u), hook, f"{ns}: nk_vjp against the hook")
    P.close()


def test_bratu_create_refuses_a_bad_side(nls):
    from nonlinearsolve_jl_amd import _lib as L
    for ns in (0, -4, 2 ** 30, float("nan")):
        with pytest.raises(L.NKError, match="n_side"):
            nls.Bratu2D(ns, 6.0)
    nls.Bratu2D(1, 6.0).close()


# -------------------------------------------------------------------------------------------------------- Bratu residual
def _check_fused(c, o, plain, what, exact=True):
    g = o.grid
    PR.same(o.f, plain, f"{what}: fused f against the plain kernel's")
    PR.same(o.f_copy, o.f, f"{what}: f_copy")
    PR.same(o.ss_copy[:g], o.partials[g:2 * g], f"{what}: ss_copy")
    PR.untouched(o.ss_copy[g:], f"{what}: ss_copy behind its {g} entries")
    PR.untouched(o.partials[2 * g:], f"{what}: partials behind their 2·{g} entries")
    if exact:
        PR.same(o.partials[:2 * g], o.partials_ref[:2 * g], f"{what}: fused partials against k_absmax_sumsq's")
    else:                                                  # (with NaNs about: the same values, a NaN where the other has one)
        assert np.array_equal(o.partials[:2 * g], o.partials_ref[:2 * g], equal_nan=True), f"{what}: fused partials against k_absmax_sumsq's"
    if exact:
        PR.check_partials(o.f, g, o.partials[:2 * g], what)
    whole = c.nl == c.ns and c.lo is None and c.hi is None
    if whole:
        assert not np.any(PR.bits(o.gpart[:2 * g]) == PR.bits(PR.CANARY)), f"{what}: a Gershgorin partial was not written"
        PR.untouched(o.gpart[2 * g:], f"{what}: gpart behind its 2·{g} entries")
    else:
        PR.untouched(o.gpart, f"{what}: gpart of a slab that is not the whole grid")


@pytest.mark.parametrize("scale", [0.0, 1.0])
@pytest.mark.parametrize("shape", PR.BRATU_SHAPES, ids=PR.shape_id)
def test_bratu_residual(nls, shape, scale):
    """k_bratu_residual within u·(7·M_k + E·c_exp·eᵘ) of the long-double residual, entry by entry; k_bratu_residual_norms returns
    the same bits, the copies, and k_absmax_sumsq's partial results"""
    PR.need_longdouble()
    c = PR.residual_case(shape, scale)
    what = f"{PR.shape_id(shape)} scale {scale}"
    f = _residual(nls, c, fused=False)
    PR.check_residual(c, f, what)
    _check_fused(c, _residual(nls, c, fused=True), f, what)
    if c.nl == c.ns and c.lo is None and c.hi is None:
        P = nls.Bratu2D(c.ns, c.lam, scale)
        PR.same(P.residual(c.u), f, f"{what}: nk_residual against the hook")
        P.close()


def test_bratu_residual_capped_grid(nls):
    """1025²: 1024 workgroups, and the threads below 2049 make a second trip of four points, part of it past the end"""
    PR.need_longdouble()
    c = PR.residual_case((PR.BIG_NS,) * 2 + (False, False), 0.0)
    assert PR.red_grid(c.u.size) == PR.MAX_RED_BLOCKS and c.u.size > 4 * PR.MAX_RED_BLOCKS * PR.NK_BLOCK
    f = _residual(nls, c, fused=False)
    PR.check_residual(c, f, "1025²")
    _check_fused(c, _residual(nls, c, fused=True), f, "1025²")


def test_bratu_residual_nan_stays_in_its_workgroups(nls):
    """a NaN in one u: NaN in f at that point and its four neighbours, NaN partials in the workgroups that visit those five points and
    in no other; everything else keeps the bits of the run without it"""
    c = PR.residual_case((65, 65, False, False), 0.0)
    clean = _residual(nls, c, fused=True)
    assert clean.grid == 5
    k = 40 * 65 + 17
    c.u[k] = np.nan
    o = _residual(nls, c, fused=True)
    hit = np.zeros(c.u.size, dtype=bool)
    hit[[k, k - 1, k + 1, k - 65, k + 65]] = True
    assert np.array_equal(np.isnan(o.f), hit)
    PR.same(o.f[~hit], clean.f[~hit], "entries away from the NaN")
    _check_fused(c, o, o.f, "NaN", exact=False)
    blocks = np.zeros(o.grid, dtype=bool)
    blocks[PR.block_of(np.flatnonzero(hit), o.grid)] = True
    assert blocks.any() and not blocks.all()
    for half, name in ((o.partials[:o.grid], "max"), (o.partials[o.grid:2 * o.grid], "sum")):
        assert np.array_equal(np.isnan(half), blocks), f"{name} partials: NaN in workgroups {np.flatnonzero(np.isnan(half))}, expected {np.flatnonzero(blocks)}"
    PR.same(o.partials[:o.grid][~blocks], clean.partials[:o.grid][~blocks], "max partials of the other workgroups")


def test_bratu_residual_overflow_gives_inf_not_nan(nls):
    c = PR.residual_case((65, 65, False, False), 1.0)
    k = 40 * 65 + 17
    c.u[k] = 800.0                                         # e⁸⁰⁰ overflows
    o = _residual(nls, c, fused=True)
    assert o.f[k] == -np.inf and np.count_nonzero(~np.isfinite(o.f)) == 1
    b = int(PR.block_of(k, o.grid))
    assert not np.any(np.isnan(o.partials[:2 * o.grid]))
    assert o.partials[b] == np.inf and o.partials[o.grid + b] == np.inf
    assert np.count_nonzero(np.isinf(o.partials[:2 * o.grid])) == 2


# ------------------------------------------------------------------------------------------- Gershgorin bounds, interval
@pytest.mark.parametrize("scale", [0.0, 1.0])
@pytest.mark.parametrize("ns", PR.GERSH_NS)
def test_bratu_gershgorin_three_ways(nls, ns, scale):
    """{−lo, hi} from the residual kernel's partials, from the fill kernel's partials, from k_csr_gershgorin over the finished matrix,
    and from the ordered reference on the device's own diagonal: one pair of bit patterns. The spectrum interval likewise."""
    PR.need_longdouble()
    c = PR.residual_case((ns, ns, False, False), scale)
    P = nls.Bratu2D(ns, c.lam, scale)
    diag, interval = _linearisation(P, c.u)
    PR.check_diag(c, diag, f"{ns}: diagonal")
    want = PR.gershgorin64(ns, c.c_lap, diag)
    o = _residual(nls, c, fused=True)
    g = o.grid
    PR.same([np.max(o.gpart[:g]), np.max(o.gpart[g:2 * g])], want, f"{ns}: the residual kernel's partials")
    J = P.jac_csr()
    P.jac_values(c.u, J)
    PR.same(_gersh(J), want, f"{ns}: the fill kernel's partials")
    J.set_values(J.values())                               # the same values; the cached bounds are gone
    PR.same(_gersh(J), want, f"{ns}: k_csr_gershgorin over the matrix")
    PR.same(interval, PR.interval64(c.c_lap, diag), f"{ns}: spectrum interval")
    J.close()
    P.close()


# ------------------------------------------------------------------------------------------------------------ Bratu fill
@pytest.mark.parametrize("ns", PR.FILL_NS)
def test_bratu_fill(nls, ns):
    """k_bratu_jac: off-diagonals −c_lap exactly, diagonals within the entrywise bound, every stored position written (the 256-row
    workgroup edge lies inside a grid line for 17 and 257, at the end of the matrix for 16); the coloured fill within 4u·M_k"""
    PR.need_longdouble()
    c = PR.residual_case((ns, ns, False, False), 0.0)
    P = nls.Bratu2D(ns, c.lam, 0.0)
    J = P.jac_csr()
    nnz = J.info()["nnz"]
    J.set_values(PR.canary(nnz))
    P.jac_values(c.u, J)
    closed = J.values()
    PR.check_bratu_fill(ns, c, closed, f"{ns}: closed form")
    J2 = P.jac_csr()
    J2.set_values(PR.canary(nnz))
    ncol = P.jac_values(c.u, J2, colored=True)
    assert 1 <= ncol <= 7
    PR.check_bratu_fill(ns, c, J2.values(), f"{ns}: coloured, {ncol} colours", colored=True, closed=closed)
    for M in (J, J2):
        M.close()
    P.close()


# ----------------------------------------------------------------------------------------------------------- Brusselator
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PR.BRUS_SHAPES, ids=PR.brus_id)
def test_brusselator_slab(nls, shape, kind):
    """k_brus_residual, k_brus_jvp (J·v and Jᵀ·v) on whole grids and slabs, with and without ghost lines, out_scale and skip:
    equal bits. The forcing disc depends on the global line j0 + jl."""
    c = PR.brus_case(shape, kind)
    what = f"{PR.brus_id(shape)} {kind}"
    PR.same(_brus(nls, c, 0), PR.brus_residual64(c), f"{what}: residual")
    for op in (1, 2):
        for scaled in (False, True):
            PR.same(_brus(nls, c, op, scaled), PR.brus_jvp64(c, op == 2, scaled), f"{what}: op {op} scaled {scaled}")
        PR.untouched(_brus(nls, c, op, False, skip=1), f"{what}: op {op} with the skip flag set")


@pytest.mark.parametrize("N", PR.BRUS_WHOLE)
def test_brusselator_public(nls, N):
    """nk_residual, nk_jvp, nk_vjp, nk_jac_values and nk_problem_initial_guess of a whole grid: equal bits with the ordered reference
    (the initial guess within 1 ulp: it holds a square root); nk_spmv of the filled matrix against J·v row by row"""
    PR.need_longdouble()
    c = PR.brus_case((N, N, 0, False))
    P = nls.Brusselator2D(N, c.A, c.B, c.alpha, c.dx)
    PR.same(P.residual(c.U), PR.brus_residual64(c), f"{N}: nk_residual")
    jv = P.jvp(c.V, c.U)
    PR.same(jv, PR.brus_jvp64(c, False, False), f"{N}: nk_jvp")
    PR.same(P.vjp(c.V, c.U), PR.brus_jvp64(c, True, False), f"{N}: nk_vjp")
    PR.within_ulps(P.initial_guess(), PR.brus_u0_64(N), 1, f"{N}: initial guess")
    J = P.jac_csr()
    assert J.info()["nnz"] == 12 * N * N
    J.set_values(PR.canary(12 * N * N))
    P.jac_values(c.U, J)
    closed, _ = PR.brus_fill64(c)
    PR.same(J.values(), closed, f"{N}: nk_jac_values")
    # J against J·v, row by row within 6u·Σ|a_ij v_j|. That bound has no room for cancellation INSIDE an entry: the kernels' roundings
    # scale with M_ij (4α + 2|uv| + A + 1 for the diagonal), not with |a_ij|. On the spread U above, where 2uv reaches 4α, one row of
    # 132 098 at N = 257 came out at 1.005 of it (9.537e-07 against 9.493e-07). So this check runs at a state a solve visits — the
    # initial guess, perturbed, where M_ii ≤ 1.3·|a_ii| — with V still spread over six decades.
    s = PR.brus_case((N, N, 0, False), "state")
    P.jac_values(s.U, J)
    closed, _ = PR.brus_fill64(s)
    PR.same(J.values(), closed, f"{N}: nk_jac_values at the perturbed initial guess")
    rowptr, col, _, _ = PR.brus_pattern(N)
    absrow = np.add.reduceat(np.abs(PR._ld(closed)) * np.abs(PR._ld(s.V[col])), rowptr[:-1])
    PR.within(J.matvec(s.V), PR._ld(P.jvp(s.V, s.U)), 6.0 * PR.U * absrow, f"{N}: nk_spmv of the filled matrix against J·v")
    J.close()
    P.close()


@pytest.mark.parametrize("N", PR.BRUS_COLORED)
def test_brusselator_colored_fill(nls, N):
    """colour-compressed assembly on the small periodic grids, where most columns lie within distance 2 of each other: the library's
    colour count is the greedy count, that colouring puts no two columns of one row into one colour, and the fill is within 6u·M_k
    of the closed-form one"""
    PR.need_longdouble()
    c = PR.brus_case((N, N, 0, False))
    P = nls.Brusselator2D(N, c.A, c.B, c.alpha, c.dx)
    J = P.jac_csr()
    nnz = J.info()["nnz"]
    J.set_values(PR.canary(nnz))
    ncol = P.jac_values(c.U, J, colored=True)
    rowptr, col, _, _ = PR.brus_pattern(N)
    color = PR.greedy_coloring(2 * N * N, rowptr, col)
    PR.check_coloring(2 * N * N, rowptr, col, color, f"{N}: greedy colouring")
    print(f"Brusselator {N} x {N}: {ncol} colours")
    assert ncol == color.max() + 1
    closed, M = PR.brus_fill64(c)
    PR.check_colored_fill(J.values(), closed, M, 6.0, f"{N}: coloured fill, {ncol} colours")
    J.close()
    P.close()


# ------------------------------------------------------------------------------------------------------------- quadratic
@pytest.mark.parametrize("n", PR.QUAD_N)
def test_quadratic(nls, n):
    c = PR.quad_case(n)
    q = PR.quad64(c)
    P = nls.Quadratic(n, c.p)
    PR.same(P.residual(c.u), q["f"], f"{n}: residual")
    PR.same(P.jvp(c.v, c.u), q["jv"], f"{n}: jvp")
    PR.same(P.vjp(c.v, c.u), q["jv"], f"{n}: vjp")
    J = P.jac_csr()
    J.set_values(PR.canary(n))
    P.jac_values(c.u, J)
    PR.same(J.values(), q["jac"], f"{n}: k_quad_jac")
    J.set_values(PR.canary(n))
    assert P.jac_values(c.u, J, colored=True) == 1
    PR.same(J.values(), q["jac"], f"{n}: coloured fill")
    J.close()
    P.close()
