"""The geometric multigrid `precs` of compiled grid problems on the device (csrc/nk_gridmg.hip) against the NumPy restatement
tests/gridmg_reference.py: level shapes, every level matrix, one V-cycle inside GMRES, iteration counts, a full Newton solve,
the update after set_field / set_p, the coarsening stop of a radius-2 stencil and the refusals. Sizes are the smallest that give
three or more levels with coarse_max 4 or 5. Every figure is printed before it is asserted.

Not tested here: the refusal on a context of several ranks (NK_E_INVALID from nk_gridmg_create) cannot be reached without
starting ranks."""
import numpy as np
import pytest
import scipy.sparse as sp

import gridmg_reference as GM
from grid_device import create

pytestmark = pytest.mark.gpu

# name -> (shape, coarse_max)
CASES = {
    "bratu": ((33, 32), 4),
    "channel": ((17, 21), 5),
    "mixed": ((12, 9), 4),
    "coupled": ((17, 21), 5),
    "star3": ((9, 10, 12), 4),
    "fourth": ((21, 21), 4),
}
_SETUPS = {}


def _set_fields(P, prob, fields):
    nn = P.nn
    for k in range(prob.nfields):
        P.set_field(k, np.ascontiguousarray(fields[k * nn:(k + 1) * nn]))


def _solver(nls, P, ref, coarse_max, nu=2):
    n = ref.u.size
    op = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), ref.u)
    G = nls.GMRES(n, restart=30).set_operator(op)
    G.set_multigrid_preconditioner(P, ref.u, nu=nu, coarse_max=coarse_max)
    return G


def _setup(nls, name):
    """one problem, one solver and the shared reference per case for the whole module"""
    if name not in _SETUPS:
        shape, cm = CASES[name]
        ref = GM.reference(name, shape, cm)
        P = create(nls, ref.prob, shape)
        if ref.prob.nfields:
            _set_fields(P, ref.prob, ref.fields)
        _SETUPS[name] = (P, _solver(nls, P, ref, cm), ref)
    return _SETUPS[name]


def _level_matrix(nls, G, prob, l, shape):
    rp, ci = nls.grid_pattern(shape[0], shape[1], prob.dof, prob.stencil, prob.boundary, nz=shape[2] if prob.dim == 3 else None)
    vals = G.multigrid_level_matrix(l).values()
    n = rp.size - 1
    return sp.csr_matrix((vals, ci.astype(np.int64), rp.astype(np.int64)), shape=(n, n))


def _assert_levels(nls, G, ref):
    lv = G.multigrid_levels()
    print("levels", [x["sides"] for x in lv], "reference", ref.M.shapes)
    assert [x["sides"] for x in lv] == ref.M.shapes
    assert len(lv) >= 3
    for l, (info, rl) in enumerate(zip(lv, ref.M.levels)):
        A = _level_matrix(nls, G, ref.prob, l, rl["shape"])
        assert info["n"] == rl["A"].shape[0] and info["nnz"] == A.nnz
        err = abs(A - rl["A"]).max()
        scale = abs(rl["A"]).max()
        print(f"  level {l} {rl['shape']}: max |A - A_ref| = {err:.3e}, max |A_ref| = {scale:.3e}, rho {info['rho']:.15g} "
              f"reference {rl['rho']:.15g}")
        assert err <= 1e-12 * scale
        assert abs(info["rho"] - rl["rho"]) <= 1e-12 * rl["rho"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_level_shapes_and_matrices(nls, name):
    _P, G, ref = _setup(nls, name)
    _assert_levels(nls, G, ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_vcycle_and_iteration_count(nls, name):
    """G.solve(b, fixed_iters=1) is the reference's one-iteration result to 1e-9 relative; the count to rtol 1e-9 is within ±1 of
    the reference's and the true residual is <= 1.01e-9 ‖b‖"""
    _P, G, ref = _setup(nls, name)
    x1, _ = G.solve(ref.b, fixed_iters=1)
    e1 = np.linalg.norm(x1 - ref.x1) / np.linalg.norm(ref.x1)
    x, info = G.solve(ref.b, abstol=0.0, reltol=1e-9, maxiters=300)
    res = np.linalg.norm(ref.J @ x - ref.b) / np.linalg.norm(ref.b)
    print(f"{name}: one V-cycle rel. err {e1:.3e}; iterations {info['iters']} (reference {ref.iters}); true residual {res:.3e}")
    assert e1 <= 1e-9
    assert info["converged"] and abs(info["iters"] - ref.iters) <= 1
    assert res <= 1.01e-9


def test_newton_with_multigrid_precs_reaches_the_direct_solution(nls):
    """case (a): NewtonRaphson + GMRES with MultigridPrecs(2, 5) against plain Newton with direct solves on the restatement, and
    every step's Krylov count against the restatement's count + 1. The direct Newton is GM.sparse_newton, the loop of
    grid_core.dense_newton with a sparse LU in place of the dense solve: dense_newton takes the problems of the
    earlier tables, whose sources get their spacing from p, and 1056² dense matrices per step buy nothing."""
    prob, shape = GM.PROBLEMS["bratu"], CASES["bratu"][0]
    ref = GM.reference("bratu", shape, 5)
    P = create(nls, prob, shape)
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(gmres_restart=30, maxiters=300, reltol=1e-9, abstol=0.0,
                                                        precs=nls.MultigridPrecs(2, 5)))
    sol = nls.solve(nls.NonlinearProblem(P), alg, abstol=1e-8, maxiters=30, store_trace=True)
    uref = GM.sparse_newton(prob, shape, np.zeros(prob.dof * int(np.prod(shape))))
    err = float(np.max(np.abs(np.asarray(sol.u) - uref)))
    print(f"Newton: {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} Krylov iterations (reference count per solve "
          f"{ref.iters}), |u - u_direct|_inf = {err:.3e}, max |u| = {np.max(np.abs(uref)):.3e}")
    assert sol.retcode == "Success"
    assert err <= 1e-8
    per_step = [t["gmres_iters"] for t in sol.trace]
    print("Krylov iterations per step:", per_step)
    assert sum(per_step) == sol.stats.gmres_iters      # (the trace holds every linear solve)
    assert all(k <= ref.iters + 1 for k in per_step)


def test_update_after_set_field_and_set_p(nls):
    """new fields and a new p between two solves: the level fields and matrices follow and the fixed-iteration result is the
    reference's at the new data"""
    name = "channel"
    shape, cm = CASES[name]
    ref0, ref1 = GM.reference(name, shape, cm), GM.reference(name, shape, cm, variant=1)
    prob = ref0.prob
    P = create(nls, prob, shape)
    _set_fields(P, prob, ref0.fields)
    G = _solver(nls, P, ref0, cm)
    _assert_levels(nls, G, ref0)
    _set_fields(P, prob, ref1.fields)
    P.set_p(ref1.p)
    G.set_multigrid_preconditioner(P, ref1.u, nu=2, coarse_max=cm)
    for l, rl in enumerate(ref1.M.levels):
        nn = int(np.prod(rl["shape"]))
        for k in range(prob.nfields):
            got, want = G.multigrid_level_field(l, k), rl["fields"][k * nn:(k + 1) * nn]
            err = np.max(np.abs(got - want))
            print(f"  level {l} field {k}: max err {err:.3e}")
            assert err <= 1e-13 * max(1.0, np.max(np.abs(want)))
    _assert_levels(nls, G, ref1)
    x1, _ = G.solve(ref1.b, fixed_iters=1)
    e1 = np.linalg.norm(x1 - ref1.x1) / np.linalg.norm(ref1.x1)
    moved = np.linalg.norm(ref1.x1 - ref0.x1) / np.linalg.norm(ref0.x1)
    print(f"after the update: one V-cycle rel. err {e1:.3e} (the two references differ by {moved:.3e})")
    assert moved > 1e-3 and e1 <= 1e-9


def test_radius_two_hierarchy_stops_at_side_five(nls):
    _P, G, _ref = _setup(nls, "fourth")
    sides = [x["sides"] for x in G.multigrid_levels()]
    print(sides)
    assert sides == [(21, 21), (10, 10), (5, 5)] and min(min(s) for s in sides) >= 5


def test_default_coarse_max_and_smoothing_steps(nls):
    """coarse_max left out and nu = 3 through the same entry point: the default coarse_max for grid problems is 8"""
    prob, shape = GM.PROBLEMS["mixed"], (33, 28)
    ref = GM.reference("mixed", shape, 8, nu=3)
    P = create(nls, prob, shape)
    G = _solver(nls, P, ref, None, nu=3)
    assert [x["sides"] for x in G.multigrid_levels()] == ref.M.shapes
    x1, _ = G.solve(ref.b, fixed_iters=1)
    e1 = np.linalg.norm(x1 - ref.x1) / np.linalg.norm(ref.x1)
    print(f"nu = 3, default coarse_max: one V-cycle rel. err {e1:.3e}")
    assert e1 <= 1e-9


def test_hierarchy_follows_the_last_call(nls):
    """one solver object: another coarse_max or nu builds the grid hierarchy again; a built-in problem after a compiled one (and
    back) is served by its own hierarchy, with the results of a solver object that never saw the other"""
    prob, shape = GM.PROBLEMS["mixed"], CASES["mixed"][0]
    ref4, ref5, ref3 = GM.reference("mixed", shape, 4), GM.reference("mixed", shape, 5), GM.reference("mixed", shape, 4, nu=3)
    P = create(nls, prob, shape)
    G = _solver(nls, P, ref4, 4)
    assert [x["sides"] for x in G.multigrid_levels()] == ref4.M.shapes
    G.set_multigrid_preconditioner(P, ref5.u, nu=2, coarse_max=5)
    print([x["sides"] for x in G.multigrid_levels()], ref5.M.shapes)
    assert [x["sides"] for x in G.multigrid_levels()] == ref5.M.shapes != ref4.M.shapes
    x1, _ = G.solve(ref5.b, fixed_iters=1)
    assert np.linalg.norm(x1 - ref5.x1) <= 1e-9 * np.linalg.norm(ref5.x1)
    G.set_multigrid_preconditioner(P, ref3.u, nu=3, coarse_max=4)
    x1, _ = G.solve(ref3.b, fixed_iters=1)
    e3 = np.linalg.norm(x1 - ref3.x1) / np.linalg.norm(ref3.x1)
    print(f"after nu 2 -> 3: rel. err {e3:.3e}; the nu = 2 and nu = 3 references differ by "
          f"{np.linalg.norm(ref3.x1 - ref4.x1) / np.linalg.norm(ref4.x1):.3e}")
    assert e3 <= 1e-9
    # a Bratu2D problem of the same size on a solver object that holds a grid hierarchy, and back
    n = 16
    Pg = create(nls, GM.PROBLEMS["bratu"], (n, n))
    B = nls.Bratu2D(n, 1.0)
    u, b = np.zeros(n * n), np.random.default_rng(5).standard_normal(n * n)
    opg = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(Pg)), u)
    opb = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(B)), u)
    fresh_b, _ = nls.GMRES(n * n, restart=30).set_operator(opb).set_multigrid_preconditioner(B, u, 2, 4).solve(b, fixed_iters=3)
    fresh_g, _ = nls.GMRES(n * n, restart=30).set_operator(opg).set_multigrid_preconditioner(Pg, u, 2, 4).solve(b, fixed_iters=3)
    G2 = nls.GMRES(n * n, restart=30).set_operator(opg).set_multigrid_preconditioner(Pg, u, 2, 4)
    G2.set_operator(opb).set_multigrid_preconditioner(B, u, 2, 4)
    xb, _ = G2.solve(b, fixed_iters=3)
    with pytest.raises(nls.NKError, match="no multigrid preconditioner of a compiled grid problem"):
        G2.multigrid_levels()
    G2.set_operator(opg).set_multigrid_preconditioner(Pg, u, 2, 4)
    xg, _ = G2.solve(b, fixed_iters=3)
    print("built-in after compiled: bitwise", np.array_equal(xb, fresh_b), "; compiled after built-in: bitwise", np.array_equal(xg, fresh_g))
    assert np.array_equal(xb, fresh_b) and np.array_equal(xg, fresh_g)
    assert np.linalg.norm(xb - xg) > 1e-6 * np.linalg.norm(xb)      # (the two problems scale their residuals differently)


ZERO_DIAGONAL = """
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  f[0] = u(1, 0) - u(-1, 0) + u(0, 1) - u(0, -1);
}
"""


def test_refusals(nls):
    import torch
    # a callback problem that is no grid problem: refused as before
    n = 16
    f = nls.NonlinearFunction(lambda du, u, p: du.copy_(u * u - 2.0), jvp=lambda jv, v, u, p: jv.copy_(2.0 * u * v))
    u0 = torch.ones(n, dtype=torch.float64, device="cuda:0")
    prob = nls.NonlinearProblem(f, u0)
    G = nls.GMRES(n, restart=10).set_operator(nls.StatefulJacobianOperator(nls.JacobianOperator(prob), u0))
    with pytest.raises(nls.NKError, match="BRATU2D"):
        G.set_multigrid_preconditioner(prob, u0)
    with pytest.raises(nls.NKError, match="no multigrid preconditioner of a compiled grid problem"):
        G.multigrid_levels()
    # a zero diagonal entry: the update names the level and the row
    P = nls.CompiledGridProblem(ZERO_DIAGONAL, 12, 9, boundary="periodic")
    u = np.zeros(12 * 9)
    G2 = nls.GMRES(u.size, restart=10).set_operator(nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), u))
    with pytest.raises(nls.NKError, match=r"level 0 \(12 x 9 x 1\): the diagonal entry of row 0 is zero"):
        G2.set_multigrid_preconditioner(P, u, nu=2, coarse_max=4)
    # a level outside the hierarchy
    _P, G3, _ref = _setup(nls, "mixed")
    with pytest.raises(nls.NKError, match="level 7 outside"):
        G3.multigrid_level_matrix(7)
