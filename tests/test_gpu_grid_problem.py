"""Compiled grid problems on the device (csrc/nk_grid.hip): the generated residual, dual-number JVP and Jacobian-fill kernels
against the NumPy restatement (tests/grid_core.py, tests/grid_reference.py) and against the built-in Bratu and Brusselator problems, entry by entry
within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

(the rule of tests/test_gpu_broyden.py), then the contract (corner reads, parameters, modules, close) and the solvers through the
public interface. Every figure is printed before it is asserted."""
import numpy as np
import pytest

import grid_core as GC
import grid_reference as R
from grid_device import assert_parity, check, close_problems, device_quantities, problem, to_device, to_numpy

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("nx,ny", R.SIZES)
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_parity_with_the_restatement(nls, dev, name, nx, ny):
    """37 × 29: five workgroups, the last ragged; 3 × 3: every node on the boundary, the periodic rows all wrap; 300 × 5: long
    lines, 1500 nodes. Residual, JVP, fill and the transposed product, then the consistency of fill and JVP: the filled
    matrix times v against the dual JVP within the sum of the two bounds.
    The Brusselator has no elementary function in it: with -ffp-contract=off the device's +, −, × are the restatement's in
    the restatement's order, and every entry of all five quantities agrees BIT FOR BIT at all three sizes — asserted. The
    Bratu and box problems differ from NumPy in the last bit of exp at a few entries (≤ 2 ulp; measured max error 1.8e-15
    against bounds of 1e-15 … 5e-14) and are held to the rule."""
    assert_parity(nls, dev, R.PROBLEMS[name], (nx, ny), exact=(name == "brusselator"))


# ------------------------------------------------------------------------------------------------ parity with the built-ins
def _same_pattern(nls, Ja, Jb, dev, n):
    """two device matrices have the same pattern: same sizes, and with the same values 1, 2, 3, … in storage order they map seeded
    vectors to the same bits (tests/test_grid_reference.py holds the pattern itself against the built-in's written-out order)"""
    ia, ib = Ja.info(), Jb.info()
    assert (ia["nrows_local"], ia["nnz"]) == (ib["nrows_local"], ib["nnz"]), (ia, ib)
    w = np.arange(1, ia["nnz"] + 1, dtype=np.float64)
    Ja.set_values(w)
    Jb.set_values(w)
    x = to_device(np.random.default_rng(5).uniform(-1, 1, n), dev)
    assert np.array_equal(to_numpy(Ja.matvec(x)), to_numpy(Jb.matvec(x)))


def test_bratu_source_against_the_built_in(nls, dev):
    ns, name = 33, "bratu"
    B = nls.Bratu2D(ns, 6.0)
    P = problem(nls, R.PROBLEMS[name], (ns, ns))
    P.set_p(R.bratu_params(ns, 6.0))
    ref = GC.reference(R.PROBLEMS[name], (ns, ns), params=R.bratu_params(ns, 6.0))
    _same_pattern(nls, P.jac_csr(), B.jac_csr(), dev, ns * ns)
    got, blt = device_quantities(P, ref.u, ref.v, dev), device_quantities(B, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals", "jtv"):
        check(f"bratu source vs restatement {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"))
        check(f"bratu source vs built-in {k}", got[k], blt[k], getattr(ref, k + "_bound"))
    B.close()


def test_brusselator_source_against_the_built_in(nls, dev):
    """The built-in keeps 6 entries per row (the four neighbours of the row's own species and the two reaction terms); the
    compiled pattern keeps every (stencil point) × (component) entry, 10 per row, as nk_grid_pattern documents. So the patterns
    are compared as sets: the built-in's entries are a subset, the values agree there, and the four extra entries of every row
    are exact zeros. Residual, JVP and Jᵀv are compared entry by entry."""
    N, name = 24, "brusselator"
    B = nls.Brusselator2D(N)
    par = R.brusselator_params(N)
    P = problem(nls, R.PROBLEMS[name], (N, N))
    P.set_p(par)
    ref = GC.reference(R.PROBLEMS[name], (N, N), params=par)
    got, blt = device_quantities(P, ref.u, ref.v, dev), device_quantities(B, ref.u, ref.v, dev)
    for k in ("f", "jv", "jtv"):
        check(f"brusselator source vs restatement {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"))
        check(f"brusselator source vs built-in {k}", got[k], blt[k], getattr(ref, k + "_bound"))
    check("brusselator source vs restatement vals", got["vals"], ref.vals, ref.vals_bound)
    # the built-in matrix, column by column of the identity restricted to what a 6-per-row pattern can hold: probe with the
    # compiled pattern's own columns
    rp, ci = nls.grid_pattern(N, N, dof=2, stencil="star", boundary="periodic")
    n = 2 * N * N
    assert blt["vals"].size == 6 * n and got["vals"].size == 10 * n
    rows = np.repeat(np.arange(n), 10)
    # colours: columns with equal (i mod 3, j mod 3, species) never share a row of a radius-1 stencil on a 24 × 24 torus
    j, i = np.divmod(np.arange(N * N), N)
    colour = np.tile((i % 3) + 3 * (j % 3), 2) + 9 * np.repeat([0, 1], N * N)
    JB = B.jac_csr()
    B.jac_values(to_device(ref.u, dev), JB)
    dense_vals = np.empty(10 * n)
    for c in range(18):
        seed = (colour == c).astype(np.float64)
        y = to_numpy(JB.matvec(to_device(seed, dev)))
        sel = colour[ci] == c
        dense_vals[sel] = y[rows[sel]]
    check("brusselator built-in matrix on the compiled pattern", got["vals"], dense_vals, ref.vals_bound)
    structural = ref.vals_bound == 0.0
    assert structural.sum() == 4 * n and np.all(got["vals"][structural] == 0.0) and np.all(dense_vals[structural] == 0.0)
    B.close()


# ------------------------------------------------------------------------------------------------ contract
def test_star_source_that_reads_a_corner_gives_nan(nls, dev):
    P = nls.CompiledGridProblem(R.CORNER_SRC, 5, 4)
    f = to_numpy(P.residual(to_device(np.linspace(-1, 1, 20), dev)))
    assert f.shape == (20,) and np.all(np.isnan(f))
    P.close()
    Pb = nls.CompiledGridProblem(R.CORNER_SRC, 5, 4, stencil="box")   # the same source is a valid box problem
    assert np.all(np.isfinite(to_numpy(Pb.residual(to_device(np.linspace(-1, 1, 20), dev)))))
    Pb.close()


# a radius-1 source that reads two nodes away
TWO_AWAY_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  f[0] = 4.0 * u(0, 0) - u(-1, 0) + u(2, 0);
}
"""


@pytest.mark.parametrize("stencil", ["star", "box"])
def test_radius_1_source_that_reads_two_nodes_away_gives_nan(nls, dev, stencil):
    """every offset that is no point of the stencil reads NaN, at radius 1 as at radius 2: u(2, 0) on a 6 x 5 Dirichlet grid
    (interior and boundary nodes) under star and box; the same source is a valid star2 problem"""
    u = to_device(np.linspace(-1, 1, 30), dev)
    P = nls.CompiledGridProblem(TWO_AWAY_SRC, 6, 5, stencil=stencil)
    f = to_numpy(P.residual(u))
    assert f.shape == (30,) and np.all(np.isnan(f))
    P.close()
    P2 = nls.CompiledGridProblem(TWO_AWAY_SRC, 6, 5, stencil="star2")
    assert np.all(np.isfinite(to_numpy(P2.residual(u))))
    P2.close()


def test_reinit_p_changes_the_residual_as_the_restatement_says(nls, dev):
    import torch
    case, shape = R.PROBLEMS["box_periodic"], (37, 29)
    p0, p1 = R.BOX_PARAMS, [0.5, -1.5, 2.0]
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
    assert torch.cuda.is_available()


def test_two_sources_alive_at_once_and_a_fresh_problem_after_close(nls, dev):
    a, b = GC.reference(R.PROBLEMS["bratu"], (37, 29)), GC.reference(R.PROBLEMS["box_dirichlet"], (37, 29))
    Pa = nls.CompiledGridProblem(R.BRATU_SRC, 37, 29, params=R.PROBLEMS["bratu"].params)
    Pb = nls.CompiledGridProblem(R.BOX_SRC, 37, 29, dof=2, stencil="box", params=R.BOX_PARAMS)
    for _ in range(2):   # interleaved: each keeps its own kernels
        check("bratu beside box", to_numpy(Pa.residual(to_device(a.u, dev))), a.f, a.f_bound)
        check("box beside bratu", to_numpy(Pb.jvp(to_device(b.v, dev), to_device(b.u, dev))), b.jv, b.jv_bound)
    Pa.close()
    check("box after bratu closed", to_numpy(Pb.residual(to_device(b.u, dev))), b.f, b.f_bound)
    Pb.close()
    Pc = nls.CompiledGridProblem(R.BRATU_SRC, 37, 29, params=R.PROBLEMS["bratu"].params)
    check("a fresh bratu after close", to_numpy(Pc.residual(to_device(a.u, dev))), a.f, a.f_bound)
    assert np.array_equal(to_numpy(Pc.initial_guess(device=True)), np.zeros(37 * 29))
    Pc.close()


def test_more_than_eight_parameters_reach_the_source(nls, dev):
    src = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  nk_real w = 0.0;
  for (int k = 0; k < 32; ++k) w += (k + 1) * p[k];
  f[0] = w * u(0, 0) + (nk_real)(s.i + 10 * s.j) + (nk_real)(s.nx + 100 * s.ny);
}
"""
    par = [float((7 * k) % 5 - 2) for k in range(32)]
    P = nls.CompiledGridProblem(src, 4, 3, params=par)
    w = float(sum((k + 1) * par[k] for k in range(32)))
    u = np.linspace(-1, 1, 12)
    j, i = np.divmod(np.arange(12), 4)
    assert np.array_equal(to_numpy(P.residual(to_device(u, dev))), w * u + (i + 10 * j) + (4 + 100 * 3))   # small integers: exact
    par2 = [x + 1.0 for x in par]
    P.set_p(par2)
    w2 = float(sum((k + 1) * par2[k] for k in range(32)))
    assert np.array_equal(to_numpy(P.residual(to_device(u, dev))), w2 * u + (i + 10 * j) + (4 + 100 * 3))
    P.close()


# ------------------------------------------------------------------------------------------------ through the public interface
def _pair(nls, dev, which):
    """(compiled problem, built-in problem, u0, restatement problem, params, nx)"""
    if which == "bratu":
        ns = 33
        par = R.bratu_params(ns, 6.0)
        P = problem(nls, R.PROBLEMS["bratu"], (ns, ns))
        P.set_p(par)
        return P, nls.Bratu2D(ns, 6.0), to_device(np.zeros(ns * ns), dev), par, ns
    N = 24
    par = R.brusselator_params(N)
    P = problem(nls, R.PROBLEMS["brusselator"], (N, N))
    P.set_p(par)
    B = nls.Brusselator2D(N)
    return P, B, B.initial_guess(device=True), par, N


def _algorithms(nls, which):
    """The Brusselator at N = 24 has α/dx² = 5290 and |f(u0)|∞ ≈ 4e4. GMRES(30) capped at 300 iterations does not solve its
    Newton systems, and with a left preconditioner the forwarded absolute tolerance stops the inner solves at once — the
    built-in problem ends in MaxIters / Stalled exactly like the compiled one (same counters). So its linear solves get what the
    project's other Brusselator tests use: GMRES(60) with 3000 iterations unpreconditioned, and reltol 1e-9 / abstol 0 with the
    preconditioner on the right (tests/test_gpu_amg.py) for the `precs` objects."""
    if which == "brusselator":
        def G(precs=None):
            if precs is None:
                return nls.KrylovJL_GMRES(gmres_restart=60, maxiters=3000)
            return nls.KrylovJL_GMRES(gmres_restart=30, maxiters=600, reltol=1e-9, abstol=0.0, precs=nls.ObjectPrecs(precs.kind, "right"))
    else:
        G = nls.KrylovJL_GMRES
    return {
        "newton_matfree": (nls.NewtonRaphson(linsolve=G()), ("bratu", "brusselator")),
        "newton_concrete": (nls.NewtonRaphson(linsolve=G(), concrete_jac=True), ("bratu", "brusselator")),
        "newton_ilu0": (nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("ilu0", "left")), concrete_jac=True),
                        ("bratu", "brusselator")),
        "newton_amg": (nls.NewtonRaphson(linsolve=G(precs=nls.ObjectPrecs("amg", "left")), concrete_jac=True),
                       ("bratu", "brusselator")),
        "trust_region": (nls.TrustRegion(linsolve=G()), ("brusselator",)),      # needs Jᵀ: the filled Jacobian's transposed SpMV
        "dfsane": (nls.DFSane(), ("bratu",)),
    }


@pytest.mark.parametrize("which,algname", [(w, a) for a in ("newton_matfree", "newton_concrete", "newton_ilu0", "newton_amg",
                                                            "trust_region", "dfsane")
                                           for w in ("bratu", "brusselator")
                                           if not (a == "trust_region" and w == "bratu") and not (a == "dfsane" and w == "brusselator")])
def test_solves_like_the_built_in(nls, dev, which, algname):
    """Success, the built-in problem's step count, and a root of the BUILT-IN residual: ‖f_builtin(u)‖∞ <= abstol + the residual
    bound of the restatement at that u. Which kernels ran: the library does not count forward-difference residuals in nf, so
    the evidence that the dual JVP and the fill are what the solver calls is the parity tests above (nk_jvp and nk_jac_values
    are the solver's own paths, and a √eps JVP misses its bound by eight orders of magnitude) together with the work counters
    here: nf and njacs equal the built-in problem's, a matrix-free solve fills no Jacobian, a concrete one fills one per step."""
    abstol = 1e-9 if which == "bratu" else 1e-7   # (|f(u0)|∞ is 5e-3 for Bratu and 4e4 for the Brusselator)
    alg, _on = _algorithms(nls, which)[algname]
    P, B, u0, par, nx = _pair(nls, dev, which)
    kw = dict(abstol=abstol, maxiters=60)
    if algname == "dfsane":
        # DFSane is non-monotone by design and needs ≈ 1700 … 2200 steps on Bratu 33 (tests/dfsane_reference.py: 1812 in float64,
        # 2225 in long double). The default AbsNormSafeBest mode ends such a run as Stalled (no new best residual for 32 steps) on
        # the built-in problem exactly as on the compiled one, so the solve runs under the plain AbsNorm mode, as
        # tools/dfsane_bench.py and the restatement do.
        kw = dict(abstol=abstol, maxiters=10000, termination_condition=nls.AbsNormTerminationMode())
    sol = nls.solve(nls.NonlinearProblem(P, u0.clone()), alg, **kw)
    blt = nls.solve(nls.NonlinearProblem(B, u0.clone()), alg, **kw)
    print(f"{which} {algname}: compiled {sol.retcode} {sol.stats}, built-in {blt.retcode} {blt.stats}")
    assert sol.retcode == "Success" == blt.retcode
    assert sol.stats.nsteps == blt.stats.nsteps
    fb = to_numpy(B.residual(sol.u))
    name = "bratu" if which == "bratu" else "brusselator"
    at_root = GC.Reference(R.PROBLEMS[name], (nx, nx), to_numpy(sol.u), np.zeros(sol.u.numel()), params=par)
    print(f"  built-in residual at the compiled problem's root: {np.abs(fb).max():.3e}; residual bound there {at_root.f_bound.max():.3e}")
    assert float(np.abs(fb).max()) <= abstol + float(at_root.f_bound.max())
    assert sol.stats.nf == blt.stats.nf
    if algname == "newton_matfree":
        assert sol.stats.njacs == 0 == blt.stats.njacs and sol.stats.op_applies >= sol.stats.gmres_iters > 0
    elif algname.startswith("newton_"):
        assert sol.stats.njacs == blt.stats.njacs >= sol.stats.nsteps > 0
    elif algname == "dfsane":
        assert (sol.stats.njacs, sol.stats.op_applies) == (0, 0)
    B.close()


def test_step_and_init_interface(nls, dev):
    """init / step_ / solve_ on the compiled Bratu problem, step by step beside the built-in problem"""
    P, B, u0, par, ns = _pair(nls, dev, "bratu")
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True)
    c = nls.init(nls.NonlinearProblem(P, u0.clone()), alg, abstol=1e-9)
    cb = nls.init(nls.NonlinearProblem(B, u0.clone()), alg, abstol=1e-9)
    f0 = c.fnorm_inf
    assert f0 == cb.fnorm_inf == R.bratu_params(ns, 6.0)[1]   # f(0) = −c_exp·e⁰ at every node
    nls.step_(c)
    nls.step_(cb)
    print(f"after one step: |u - u_builtin| {np.abs(to_numpy(c.u) - to_numpy(cb.u)).max():.3e}, fnorm {c.fnorm_inf:.6e} vs {cb.fnorm_inf:.6e}")
    assert c.nsteps == cb.nsteps == 1 and c.fnorm_inf < 0.5 * f0
    assert nls.solve_(c).retcode == "Success" == nls.solve_(cb).retcode
    assert c.nsteps == cb.nsteps
    c.close()
    cb.close()
    B.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    close_problems()
