"""Compiled grid problems in three dimensions on the device (csrc/nk_grid.hip, nk_problem_create_grid3): the generated
residual, dual-number JVP and Jacobian-fill kernels against the NumPy restatement (tests/grid_core.py, tests/grid3_reference.py), entry by entry
within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

then the contract (edge reads, parameters, modules, close, a 2-D problem beside a 3-D one) and the solvers through the public
interface against a dense NumPy Newton on the restatement. Every figure is printed before it is asserted."""
import numpy as np
import pytest

import grid3_reference as R
import grid_core as GC
import grid_reference as R2
from grid_device import assert_parity, check, close_problems, device_quantities, problem, to_device, to_numpy

pytestmark = pytest.mark.gpu

LAMBDA = 3.0   # Bratu on (a box inside) the unit cube: well below the 3-D turning point (grid3_reference.bratu3_params)


# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("nx,ny,nz", R.SIZES)
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_parity_with_the_restatement(nls, dev, name, nx, ny, nz):
    """7 × 6 × 5: one ragged workgroup; 3 × 3 × 3: every node on the boundary, every periodic row wraps three ways; 37 × 29 × 3:
    13 workgroups, the last ragged, planes of 1073 nodes so that workgroups straddle lines and planes; 5 × 3 × 70: planes of 15
    nodes, a wavefront spans more than four planes — the (i, j, k) decomposition. Residual, JVP, fill and the transposed
    product, then the consistency of fill and JVP: the filled matrix times v against the dual JVP within the sum of the two
    bounds.
    brusselator3, four3 and box3 have no elementary function in them: with -ffp-contract=off the device's +, −, × are the
    restatement's in the restatement's order. What the MI355X showed is recorded at EXACT below and asserted."""
    P, _ref = assert_parity(nls, dev, R.PROBLEMS[name], (nx, ny, nz), exact=name in EXACT)
    assert P.nz == nz


# The problems whose five quantities agreed BIT FOR BIT with the restatement at all four shapes on the MI355X (100 of 100
# comparisons, every entry): brusselator3 as expected, and so did four3 and the box problem — none of them has an elementary
# function. bratu3 differs from NumPy in the last bits of exp at a few entries (max error 8.9e-16 against bounds of
# 8.9e-16 … 4.9e-14) and is held to the rule.
EXACT = ("brusselator3", "four3", "box3_dirichlet", "box3_periodic")


# ------------------------------------------------------------------------------------------------ contract
def test_star_source_that_reads_an_edge_gives_nan(nls, dev):
    P = nls.CompiledGridProblem(R.EDGE_SRC, 5, 4, nz=3)
    f = to_numpy(P.residual(to_device(np.linspace(-1, 1, 60), dev)))
    assert f.shape == (60,) and np.all(np.isnan(f))
    P.close()
    Pb = nls.CompiledGridProblem(R.EDGE_SRC, 5, 4, stencil="box", nz=3)   # the same source is a valid box problem
    assert np.all(np.isfinite(to_numpy(Pb.residual(to_device(np.linspace(-1, 1, 60), dev)))))
    Pb.close()


# a radius-1 source that reads two nodes away
TWO_AWAY_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  f[0] = 6.0 * u(0, 0, 0) - u(-1, 0, 0) + u(0, 0, 2);
}
"""


@pytest.mark.parametrize("stencil", ["star", "box"])
def test_radius_1_source_that_reads_two_nodes_away_gives_nan(nls, dev, stencil):
    """every offset that is no point of the stencil reads NaN, at radius 1 as at radius 2: u(0, 0, 2) on a 6 x 5 x 5 Dirichlet
    grid (interior and boundary nodes) under star and box; the same source is a valid star2 problem"""
    u = to_device(np.linspace(-1, 1, 150), dev)
    P = nls.CompiledGridProblem(TWO_AWAY_SRC, 6, 5, stencil=stencil, nz=5)
    f = to_numpy(P.residual(u))
    assert f.shape == (150,) and np.all(np.isnan(f))
    P.close()
    P2 = nls.CompiledGridProblem(TWO_AWAY_SRC, 6, 5, stencil="star2", nz=5)
    assert np.all(np.isfinite(to_numpy(P2.residual(u))))
    P2.close()


def test_reinit_p_changes_the_residual_as_the_restatement_says(nls, dev):
    case, shape = R.PROBLEMS["box3_periodic"], (7, 6, 5)
    p0, p1 = R.BOX3_PARAMS, [-0.5, 0.125, 2.0]
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


def test_two_sources_alive_at_once_and_a_fresh_problem_after_close(nls, dev):
    s = (7, 6, 5)
    a, b = GC.reference(R.PROBLEMS["bratu3"], s), GC.reference(R.PROBLEMS["box3_dirichlet"], s)
    Pa = nls.CompiledGridProblem(R.BRATU3_SRC, s[0], s[1], params=R.PROBLEMS["bratu3"].params, nz=s[2])
    Pb = nls.CompiledGridProblem(R.BOX3_SRC, s[0], s[1], stencil="box", params=R.BOX3_PARAMS, nz=s[2])
    for _ in range(2):   # interleaved: each keeps its own kernels
        check("bratu3 beside box3", to_numpy(Pa.residual(to_device(a.u, dev))), a.f, a.f_bound)
        check("box3 beside bratu3", to_numpy(Pb.jvp(to_device(b.v, dev), to_device(b.u, dev))), b.jv, b.jv_bound)
    Pa.close()
    check("box3 after bratu3 closed", to_numpy(Pb.residual(to_device(b.u, dev))), b.f, b.f_bound)
    Pb.close()
    Pc = nls.CompiledGridProblem(R.BRATU3_SRC, s[0], s[1], params=R.PROBLEMS["bratu3"].params, nz=s[2])
    check("a fresh bratu3 after close", to_numpy(Pc.residual(to_device(a.u, dev))), a.f, a.f_bound)
    assert np.array_equal(to_numpy(Pc.initial_guess(device=True)), np.zeros(7 * 6 * 5))
    Pc.close()


def test_more_than_eight_parameters_reach_the_source(nls, dev):
    src = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  nk_real w = 0.0;
  for (int k = 0; k < 32; ++k) w += (k + 1) * p[k];
  f[0] = w * u(0, 0, 0) + (nk_real)(s.i + 10 * s.j + 100 * s.k) + (nk_real)(1000 * s.nx + 10000 * s.ny + 100000 * s.nz);
}
"""
    par = [float((7 * k) % 5 - 2) for k in range(32)]
    nx, ny, nz = 4, 3, 5
    P = nls.CompiledGridProblem(src, nx, ny, params=par, nz=nz)
    w = float(sum((k + 1) * par[k] for k in range(32)))
    u = np.linspace(-1, 1, nx * ny * nz)
    k, rem = np.divmod(np.arange(nx * ny * nz), nx * ny)
    j, i = np.divmod(rem, nx)
    site = (i + 10 * j + 100 * k) + (1000 * nx + 10000 * ny + 100000 * nz)
    assert np.array_equal(to_numpy(P.residual(to_device(u, dev))), w * u + site)   # small integers: exact
    par2 = [x + 1.0 for x in par]
    P.set_p(par2)
    w2 = float(sum((k + 1) * par2[k] for k in range(32)))
    assert np.array_equal(to_numpy(P.residual(to_device(u, dev))), w2 * u + site)
    P.close()


def test_a_2d_and_a_3d_problem_side_by_side(nls, dev):
    """the Bratu source of each dimension, alive together and called in turn: each keeps its kernels, its pattern and its
    parameters (the 3-D programs are cached apart from the 2-D ones of a related source)"""
    a2, a3 = GC.reference(R2.PROBLEMS["bratu"], (37, 29)), GC.reference(R.PROBLEMS["bratu3"], (7, 6, 5))
    P2 = nls.CompiledGridProblem(R2.BRATU_SRC, 37, 29, params=R2.PROBLEMS["bratu"].params)
    P3 = nls.CompiledGridProblem(R.BRATU3_SRC, 7, 6, params=R.PROBLEMS["bratu3"].params, nz=5)
    assert not hasattr(P2, "nz") and P3.nz == 5
    for _ in range(2):
        g2, g3 = device_quantities(P2, a2.u, a2.v, dev), device_quantities(P3, a3.u, a3.v, dev)
        for k in ("f", "jv", "vals", "jtv"):
            check(f"2-D bratu beside 3-D {k}", g2[k], getattr(a2, k), getattr(a2, k + "_bound"))
            check(f"3-D bratu beside 2-D {k}", g3[k], getattr(a3, k), getattr(a3, k + "_bound"))
    P2.set_p([2.0, 0.5])   # the 2-D problem's parameters are its own
    check("3-D after the 2-D set_p", to_numpy(P3.residual(to_device(a3.u, dev))), a3.f, a3.f_bound)
    P2.close()
    check("3-D after the 2-D close", to_numpy(P3.jvp(to_device(a3.v, dev), to_device(a3.u, dev))), a3.jv, a3.jv_bound)
    P3.close()


# ------------------------------------------------------------------------------------------------ through the public interface
_NEWTON = {}


def _bratu3(nls, shape):
    P = problem(nls, R.PROBLEMS["bratu3"], shape)
    par = R.bratu3_params(shape[0], LAMBDA)
    P.set_p(par)
    return P, par


def _restated_residual(shape, u, par):
    """the restatement's residual at u with its entrywise bound"""
    at = GC.Reference(R.PROBLEMS["bratu3"], shape, u, np.zeros(u.size), params=par)
    return at.f, at.f_bound


def _dense_newton(shape, par):
    """u_ref with ‖F(u_ref)‖∞ <= 1e-12 by a dense NumPy Newton on the restatement, ‖F(u_ref)‖∞ and ‖J(u_ref)⁻¹‖∞ (computed once)"""
    if shape not in _NEWTON:
        prob, u = R.PROBLEMS["bratu3"], np.zeros(shape[0] * shape[1] * shape[2])
        for _it in range(30):
            J, f = GC.dense_jacobian(prob, shape, u, params=par)
            if np.abs(f).max() <= 1e-12:
                break
            u = u - np.linalg.solve(J, f)
        assert np.abs(f).max() <= 1e-12
        _NEWTON[shape] = (u, float(np.abs(f).max()), float(np.linalg.norm(np.linalg.inv(J), np.inf)))
    return _NEWTON[shape]


def _algorithms(nls):
    G = nls.KrylovJL_GMRES
    return {
        "newton_matfree": nls.NewtonRaphson(linsolve=G()),
        "newton_concrete": nls.NewtonRaphson(linsolve=G(), concrete_jac=True),
        "newton_jacobi": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("jacobi", "left")), concrete_jac=True),
        "newton_ilu0": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("ilu0", "left")), concrete_jac=True),
        "newton_amg": nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("amg", "left")), concrete_jac=True),
        "trust_region": nls.TrustRegion(linsolve=G()),
        # J⁻¹ starts as I/6 — the Jacobi scaling of the 7-point operator, whose diagonal is 6 c_lap − c_exp eᵘ ≈ 6 — and keeps
        # 32 columns, the most the solver offers. The default start 2‖f‖/max(‖u‖, 1) with 10 columns diverges on Bratu once
        # the columns are overwritten (tests/lbroyden_reference.py says so of Bratu2D, and its restatement says so of this
        # problem: Unstable after 33 steps); with these settings the restatement converges in 30 steps, before any column
        # is overwritten, and in 29 … 32 steps for every α from 4 to 8.
        "lbroyden": nls.LimitedMemoryBroyden(threshold=32, alpha=6.0),
        "dfsane": nls.DFSane(),
    }


@pytest.mark.parametrize("algname", ["newton_matfree", "newton_concrete", "newton_jacobi", "newton_ilu0", "newton_amg",
                                     "trust_region", "lbroyden", "dfsane"])
def test_solves_bratu3_like_a_dense_newton(nls, dev, algname):
    """8 × 7 × 6 (336 unknowns), λ = 3: |u_dev − u_ref|∞ <= 2·‖J(u_ref)⁻¹‖∞·(‖F(u_dev)‖∞ + ‖F(u_ref)‖∞), both residuals by the
    restatement, ‖J⁻¹‖∞ from the dense reference Jacobian; the factor 2 covers the second-order term of
    F(u_dev) − F(u_ref) = J(u_ref)(u_dev − u_ref) + O(|u_dev − u_ref|²)."""
    shape, abstol = (8, 7, 6), 1e-10
    P, par = _bratu3(nls, shape)
    u_ref, f_ref, jinv = _dense_newton(shape, par)
    kw = dict(abstol=abstol, maxiters=60)
    if algname in ("dfsane", "lbroyden"):   # residual-only methods: more, cheaper steps; the plain ‖F‖∞ <= abstol test
        kw = dict(abstol=abstol, maxiters=2000, termination_condition=nls.AbsNormTerminationMode())
    sol = nls.solve(nls.NonlinearProblem(P, to_device(np.zeros(u_ref.size), dev)), _algorithms(nls)[algname], **kw)
    u_dev = to_numpy(sol.u)
    f_dev = float(np.abs(_restated_residual(shape, u_dev, par)[0]).max())
    err, bound = float(np.abs(u_dev - u_ref).max()), 2.0 * jinv * (f_dev + f_ref)
    print(f"bratu3 {algname}: {sol.retcode} {sol.stats}; |u_dev - u_ref| {err:.3e}, bound {bound:.3e} "
          f"(|J^-1| {jinv:.3e}, |F(u_dev)| {f_dev:.3e}, |F(u_ref)| {f_ref:.3e})")
    assert sol.retcode == "Success"
    assert err <= bound
    assert f_dev <= abstol + float(_restated_residual(shape, u_dev, par)[1].max())
    if algname == "newton_matfree":
        assert sol.stats.njacs == 0 and sol.stats.op_applies >= sol.stats.gmres_iters > 0
    elif algname.startswith("newton_"):
        assert sol.stats.njacs >= sol.stats.nsteps > 0
    elif algname in ("dfsane", "lbroyden"):
        assert sol.stats.njacs == 0


@pytest.mark.parametrize("shape", [(40, 30, 4), (16, 16, 8)])
def test_default_sstep_gmres_on_the_filled_jacobian(nls, dev, shape):
    """40 × 30 × 4 (4800 unknowns): planes of 1200 rows, more than the matrix-powers plan's 1024-row window — the streaming
    operator; 16 × 16 × 8: planes of 256 rows, which the resident plan may accept. NewtonRaphson with the default s-step GMRES
    on the concrete Jacobian; the restatement's residual at the device's answer is <= abstol + its entrywise bound."""
    abstol = 1e-10
    P, par = _bratu3(nls, shape)
    n = shape[0] * shape[1] * shape[2]
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True)
    assert alg.linsolve.ortho == "sstep"
    sol = nls.solve(nls.NonlinearProblem(P, to_device(np.zeros(n), dev)), alg, abstol=abstol, maxiters=60)
    f, fb = _restated_residual(shape, to_numpy(sol.u), par)
    J = P.jac_csr()
    P.jac_values(sol.u, J)
    _Y, resident = J.powers(to_device(np.ones(n), dev), 4)
    print(f"bratu3 {shape}: {sol.retcode} {sol.stats}; restated |F| {np.abs(f).max():.3e}, bound {fb.max():.3e}; "
          f"matrix powers of this Jacobian: {'resident' if resident else 'streaming'} kernel")
    assert sol.retcode == "Success" and sol.stats.njacs >= sol.stats.nsteps > 0 and sol.stats.gmres_iters > 0
    assert np.all(np.abs(f) <= abstol + fb)
    if shape == (40, 30, 4):
        assert not resident


def test_step_and_init_interface(nls, dev):
    """init / step_ / solve_ on the compiled 3-D Bratu problem"""
    shape = (8, 7, 6)
    P, par = _bratu3(nls, shape)
    u_ref, f_ref, jinv = _dense_newton(shape, par)
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True)
    c = nls.init(nls.NonlinearProblem(P, to_device(np.zeros(u_ref.size), dev)), alg, abstol=1e-10)
    f0 = c.fnorm_inf
    assert f0 == par[1]   # f(0) = −c_exp·e⁰ at every node
    nls.step_(c)
    print(f"after one step: fnorm {c.fnorm_inf:.6e} (from {f0:.6e})")
    assert c.nsteps == 1 and c.fnorm_inf < 0.5 * f0
    assert nls.solve_(c).retcode == "Success"
    f_dev = float(np.abs(_restated_residual(shape, to_numpy(c.u), par)[0]).max())
    assert float(np.abs(to_numpy(c.u) - u_ref).max()) <= 2.0 * jinv * (f_dev + f_ref)
    c.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    close_problems()
