"""Compiled grid problems with a radius-2 stencil on the device (csrc/nk_grid.hip: NK_GRID_STAR2 in 2-D and 3-D,
NK_GRID_DIAMOND2 in 2-D): the generated residual, dual-number JVP and Jacobian-fill kernels against the NumPy restatement
(tests/grid_core.py, tests/grid_r2_reference.py), entry by entry within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

then the contract (reads outside the stencil's shape, parameters, modules, close, radius 1 beside radius 2, 2-D beside 3-D) and
the solvers through the public interface against a dense NumPy Newton on the restatement. Every figure is printed before it is
asserted."""
import numpy as np
import pytest

import grid_core as GC
import grid_r2_reference as R
import grid_reference as R1
from grid_device import assert_parity, check, close_problems, device_quantities, problem, to_device, to_numpy

pytestmark = pytest.mark.gpu

LAMBDA = 3.0   # Bratu on (a box inside) the unit square / cube: well below the turning point in both dimensions


def _create(nls, source, shape, **kw):
    return nls.CompiledGridProblem(source, shape[0], shape[1], nz=shape[2] if len(shape) == 3 else None, **kw)


# ------------------------------------------------------------------------------------------------ parity with the restatement
CASES = [(name, shape) for name in sorted(R.PROBLEMS) for shape in R.SIZES[R.PROBLEMS[name].dim]]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in CASES])
def test_parity_with_the_restatement(nls, dev, name, shape):
    """2-D — 5 × 5: every periodic row wraps in both layers both ways, every Dirichlet node misses points; 37 × 29: five
    workgroups, the last ragged; 300 × 5: a wavefront spans lines. 3-D — 5 × 5 × 5; 7 × 6 × 5: one ragged workgroup;
    37 × 29 × 5: planes of 1073 nodes; 5 × 5 × 70: a wavefront spans planes. Residual, JVP, fill and the transposed product,
    then the consistency of fill and JVP: the filled matrix times v against the dual JVP within the sum of the two bounds.
    The upwind problems, sh and diamond_dirichlet have no elementary function in them: with -ffp-contract=off the device's
    +, −, × are the restatement's in the restatement's order. What the MI355X showed is recorded at EXACT below and asserted."""
    assert_parity(nls, dev, R.PROBLEMS[name], shape, exact=name in EXACT)


# The problems whose five quantities agreed BIT FOR BIT with the restatement at every shape of their dimension on the MI355X
# (100 of 100 comparisons, every entry): all six sources without an elementary function. lap4 and lap4_3 differ from NumPy in
# the last bits of exp at single entries (3 of 144 278 entries over all shapes; max error 7.1e-15 against that entry's bound of
# 1.1e-13) and are held to the rule.
EXACT = ("upwind2_dirichlet", "upwind2_periodic", "sh", "diamond_dirichlet", "upwind3_dirichlet", "upwind3_periodic")


# ------------------------------------------------------------------------------------------------ contract
@pytest.mark.parametrize("key,stencil,shape", [("star2", "star2", (6, 5)), ("diamond2", "diamond2", (6, 5)),
                                               ("star2_3", "star2", (6, 5, 5))])
def test_source_that_reads_outside_its_stencil_gives_nan(nls, dev, key, stencil, shape):
    n = int(np.prod(shape))
    P = _create(nls, R.OUTSIDE_SRC[key], shape, stencil=stencil)
    f = to_numpy(P.residual(to_device(np.linspace(-1, 1, n), dev)))
    assert f.shape == (n,) and np.all(np.isnan(f))
    P.close()


def test_star2_source_is_finite_under_diamond2(nls, dev):
    """the diamond contains the star: a source written for star2 is a valid diamond2 problem, with the same residual; and the
    star2 source that reads (1, 1) — NaN under star2 — is finite under diamond2"""
    shape = (37, 29)
    ref = GC.reference(R.PROBLEMS["lap4"], shape)
    P = _create(nls, R.LAP4_SRC, shape, stencil="diamond2", params=R.PROBLEMS["lap4"].params)
    check("lap4 under diamond2", to_numpy(P.residual(to_device(ref.u, dev))), ref.f, ref.f_bound)
    assert P.jac_csr().info()["nnz"] == GC.stencil_pattern(shape, 1, "diamond2", "dirichlet")[1].size
    P.close()
    Pd = _create(nls, R.OUTSIDE_SRC["star2"], (6, 5), stencil="diamond2")
    assert np.all(np.isfinite(to_numpy(Pd.residual(to_device(np.linspace(-1, 1, 30), dev)))))
    Pd.close()


def test_reinit_p_changes_the_residual_as_the_restatement_says(nls, dev):
    case, shape = R.PROBLEMS["diamond_dirichlet"], (37, 29)
    p0, p1 = R.DIAMOND_PARAMS, [-0.5, 0.125, 2.0]
    P = problem(nls, case, shape)
    ref0, ref1 = GC.reference(case, shape), GC.reference(case, shape, params=p1)
    prob = nls.NonlinearProblem(P, to_device(ref0.u, dev), p0)
    cache = nls.init(prob, nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES()), abstol=1e-10)
    check("fu after init", to_numpy(cache.fu), ref0.f, ref0.f_bound)
    nls.reinit_(cache, u0=to_device(ref0.u, dev), p=p1)
    check("fu after reinit_(p=...)", to_numpy(cache.fu), ref1.f, ref1.f_bound)
    assert float(np.max(np.abs(ref1.f - ref0.f))) > 1e6 * float(ref1.f_bound.max())
    # the Jacobian follows the parameters too (a fill cached for the same u is not reused)
    u = to_device(ref0.u, dev)
    check("Jᵀv with the new p", to_numpy(P.vjp(to_device(ref0.v, dev), u)), ref1.jtv, ref1.jtv_bound)
    P.set_p(p0)
    check("Jᵀv with the old p, same u buffer", to_numpy(P.vjp(to_device(ref0.v, dev), u)), ref0.jtv, ref0.jtv_bound)
    with pytest.raises(ValueError):
        P.set_p([1.0])
    cache.close()


def test_radius_1_beside_radius_2_and_a_fresh_problem_after_close(nls, dev):
    """the radius-1 Bratu source and the fourth-order one, alive together and called in turn: each keeps its kernels, its
    pattern and its parameters (the radius-2 programs carry an option of their own, so the cache keeps them apart)"""
    shape = (37, 29)
    a1, a2 = GC.reference(R1.PROBLEMS["bratu"], shape), GC.reference(R.PROBLEMS["lap4"], shape)
    P1 = nls.CompiledGridProblem(R1.BRATU_SRC, *shape, params=R1.PROBLEMS["bratu"].params)
    P2 = _create(nls, R.LAP4_SRC, shape, stencil="star2", params=R.PROBLEMS["lap4"].params)
    assert P1.jac_csr().info()["nnz"] == a1.vals.size and P2.jac_csr().info()["nnz"] == a2.vals.size
    for _ in range(2):
        g1, g2 = device_quantities(P1, a1.u, a1.v, dev), device_quantities(P2, a2.u, a2.v, dev)
        for k in ("f", "jv", "vals", "jtv"):
            check(f"radius-1 bratu beside lap4 {k}", g1[k], getattr(a1, k), getattr(a1, k + "_bound"))
            check(f"lap4 beside radius-1 bratu {k}", g2[k], getattr(a2, k), getattr(a2, k + "_bound"))
    P1.set_p([2.0, 0.5])   # the radius-1 problem's parameters are its own
    check("lap4 after the radius-1 set_p", to_numpy(P2.residual(to_device(a2.u, dev))), a2.f, a2.f_bound)
    P1.close()
    check("lap4 after the radius-1 close", to_numpy(P2.jvp(to_device(a2.v, dev), to_device(a2.u, dev))), a2.jv, a2.jv_bound)
    P2.close()
    P3 = _create(nls, R.LAP4_SRC, shape, stencil="star2", params=R.PROBLEMS["lap4"].params)
    check("a fresh lap4 after close", to_numpy(P3.residual(to_device(a2.u, dev))), a2.f, a2.f_bound)
    assert np.array_equal(to_numpy(P3.initial_guess(device=True)), np.zeros(37 * 29))
    P3.close()


def test_a_2d_and_a_3d_radius_2_problem_side_by_side(nls, dev):
    s2, s3 = (37, 29), (7, 6, 5)
    c2, c3 = R.PROBLEMS["upwind2_periodic"], R.PROBLEMS["upwind3_periodic"]
    a2, a3 = GC.reference(c2, s2), GC.reference(c3, s3)
    P2, P3 = problem(nls, c2, s2), problem(nls, c3, s3)
    assert not hasattr(P2, "nz") and P3.nz == 5
    for _ in range(2):
        g2, g3 = device_quantities(P2, a2.u, a2.v, dev), device_quantities(P3, a3.u, a3.v, dev)
        for k in ("f", "jv", "vals", "jtv"):
            check(f"2-D upwind beside 3-D {k}", g2[k], getattr(a2, k), getattr(a2, k + "_bound"))
            check(f"3-D upwind beside 2-D {k}", g3[k], getattr(a3, k), getattr(a3, k + "_bound"))
    q = [x + 1.0 for x in R.UPWIND2_PARAMS]
    P2.set_p(q)            # the 2-D problem's parameters are its own
    check("3-D after the 2-D set_p", to_numpy(P3.residual(to_device(a3.u, dev))), a3.f, a3.f_bound)
    b2 = GC.reference(c2, s2, params=q)
    check("2-D with its new p", to_numpy(P2.residual(to_device(a2.u, dev))), b2.f, b2.f_bound)
    P2.set_p(R.UPWIND2_PARAMS)


# ------------------------------------------------------------------------------------------------ through the public interface
_NEWTON = {}
SOLVE_SHAPES = {"lap4": (9, 8), "lap4_3": (8, 7, 6)}


def _bratu(nls, name, shape):
    P = problem(nls, R.PROBLEMS[name], shape)
    par = R.lap4_params(shape[0], LAMBDA)
    P.set_p(par)
    return P, par


def _restated_residual(name, shape, u, par):
    """the restatement's residual at u with its entrywise bound"""
    at = GC.Reference(R.PROBLEMS[name], shape, u, np.zeros(u.size), params=par)
    return at.f, at.f_bound


def _dense_newton(name, shape, par):
    """u_ref with ‖F(u_ref)‖∞ <= 1e-12 by a dense NumPy Newton on the restatement, ‖F(u_ref)‖∞ and ‖J(u_ref)⁻¹‖∞ (computed once)"""
    if (name, shape) not in _NEWTON:
        prob, u = R.PROBLEMS[name], np.zeros(int(np.prod(shape)))
        for _it in range(30):
            J, f = GC.dense_jacobian(prob, shape, u, params=par)
            if np.abs(f).max() <= 1e-12:
                break
            u = u - np.linalg.solve(J, f)
        assert np.abs(f).max() <= 1e-12
        _NEWTON[(name, shape)] = (u, float(np.abs(f).max()), float(np.linalg.norm(np.linalg.inv(J), np.inf)))
    return _NEWTON[(name, shape)]


def _algorithms(nls):
    G = nls.KrylovJL_GMRES
    return {
        "newton_matfree": nls.NewtonRaphson(linsolve=G()),
        "newton_concrete": nls.NewtonRaphson(linsolve=G(), concrete_jac=True),
        # The preconditioner objects act from the RIGHT here. The linear solver is handed the nonlinear abstol (1e-10) as its
        # absolute tolerance, as in the reference, and a left-preconditioned GMRES measures ‖M⁻¹r‖₂: this operator is scaled
        # by 12h², its diagonal is 60 (90 in 3-D), so ‖M⁻¹F‖₂ falls below 1e-10 while ‖F‖∞ is still 6e-10 … 1.2e-9; GMRES then
        # returns the zero step and Newton ends "Stalled" after 35 steps (measured on the MI355X with side = "left": Jacobi
        # |F| 6.3e-10 / 1.2e-9, ILU(0) 8.9e-10 / 3.7e-10, AMG Success / 5.1e-10, for lap4 / lap4_3 — each still within the
        # distance bound to the dense Newton). The radius-1 Bratu tests have a diagonal of 4 and 6 and do not meet this.
        # From the right GMRES measures the true residual.
        "newton_jacobi": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("jacobi", "right")), concrete_jac=True),
        "newton_ilu0": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("ilu0", "right")), concrete_jac=True),
        "newton_amg": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True),
        "trust_region": nls.TrustRegion(linsolve=G()),
        "dfsane": nls.DFSane(),
    }


@pytest.mark.parametrize("algname", ["newton_matfree", "newton_concrete", "newton_jacobi", "newton_ilu0", "newton_amg",
                                     "trust_region", "dfsane"])
@pytest.mark.parametrize("name", ["lap4", "lap4_3"])
def test_solves_lap4_like_a_dense_newton(nls, dev, name, algname):
    """lap4 at 9 × 8 (72 unknowns) and lap4_3 at 8 × 7 × 6 (336), λ = 3:
    |u_dev − u_ref|∞ <= 2·‖J(u_ref)⁻¹‖∞·(‖F(u_dev)‖∞ + ‖F(u_ref)‖∞), both residuals by the restatement, ‖J⁻¹‖∞ from the dense
    reference Jacobian (≈ 0.63 and 0.29); the factor 2 covers the second-order term of
    F(u_dev) − F(u_ref) = J(u_ref)(u_dev − u_ref) + O(|u_dev − u_ref|²). The fourth-order operator has positive outer
    off-diagonals: it is no M-matrix."""
    shape, abstol = SOLVE_SHAPES[name], 1e-10
    P, par = _bratu(nls, name, shape)
    u_ref, f_ref, jinv = _dense_newton(name, shape, par)
    kw = dict(abstol=abstol, maxiters=60)
    if algname == "dfsane":   # a residual-only method: more, cheaper steps; the plain ‖F‖∞ <= abstol test
        kw = dict(abstol=abstol, maxiters=2000, termination_condition=nls.AbsNormTerminationMode())
    sol = nls.solve(nls.NonlinearProblem(P, to_device(np.zeros(u_ref.size), dev)), _algorithms(nls)[algname], **kw)
    u_dev = to_numpy(sol.u)
    f_at, f_bound = _restated_residual(name, shape, u_dev, par)
    f_dev = float(np.abs(f_at).max())
    err, bound = float(np.abs(u_dev - u_ref).max()), 2.0 * jinv * (f_dev + f_ref)
    print(f"{name} {algname}: {sol.retcode} {sol.stats}; |u_dev - u_ref| {err:.3e}, bound {bound:.3e} "
          f"(|J^-1| {jinv:.3e}, |F(u_dev)| {f_dev:.3e}, |F(u_ref)| {f_ref:.3e})")
    assert sol.retcode == "Success"
    assert err <= bound
    assert f_dev <= abstol + float(f_bound.max())
    if algname == "newton_matfree":
        assert sol.stats.njacs == 0 and sol.stats.op_applies >= sol.stats.gmres_iters > 0
    elif algname.startswith("newton_"):
        assert sol.stats.njacs >= sol.stats.nsteps > 0
    elif algname == "dfsane":
        assert sol.stats.njacs == 0


@pytest.mark.parametrize("shape", [(600, 5), (16, 16)])
def test_default_sstep_gmres_on_the_filled_jacobian(nls, dev, shape):
    """600 × 5 (3000 unknowns): a row reaches two lines up and down, 1200 rows — more than the matrix-powers plan's 1024-row
    window — the streaming operator; 16 × 16: the resident plan may accept it. NewtonRaphson with the default s-step GMRES on
    the concrete Jacobian; the restatement's residual at the device's answer is <= abstol + its entrywise bound."""
    abstol = 1e-10
    P, par = _bratu(nls, "lap4", shape)
    n = shape[0] * shape[1]
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True)
    assert alg.linsolve.ortho == "sstep"
    sol = nls.solve(nls.NonlinearProblem(P, to_device(np.zeros(n), dev)), alg, abstol=abstol, maxiters=60)
    f, fb = _restated_residual("lap4", shape, to_numpy(sol.u), par)
    J = P.jac_csr()
    P.jac_values(sol.u, J)
    _Y, resident = J.powers(to_device(np.ones(n), dev), 4)
    print(f"lap4 {shape}: {sol.retcode} {sol.stats}; restated |F| {np.abs(f).max():.3e}, bound {fb.max():.3e}; "
          f"matrix powers of this Jacobian: {'resident' if resident else 'streaming'} kernel")
    assert sol.retcode == "Success" and sol.stats.njacs >= sol.stats.nsteps > 0 and sol.stats.gmres_iters > 0
    assert np.all(np.abs(f) <= abstol + fb)
    if shape == (600, 5):
        assert not resident


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    close_problems()
