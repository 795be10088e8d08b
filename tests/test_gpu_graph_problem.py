"""Compiled graph problems on the device (csrc/nk_graph.hip): the generated residual, dual-number JVP and Jacobian-fill kernels
against the NumPy restatement (tests/graph_core.py, tests/graph_reference.py), entry by entry within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

(grid_core's rule), then the contract (reproducible bits, the coloured assembly, parameters and data, modules, close, the
runtime errors) and the solvers through the public interface. Every figure is printed before it is asserted."""
import numpy as np
import pytest

import graph_core as GC
import graph_reference as R
from grid_device import QUANTITIES, check, device_quantities, to_device, to_numpy

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def create(nls, prob, G, params=None):
    return nls.CompiledGraphProblem(prob.source, *G.csr(), dof=prob.dof, params=prob.params if params is None else params,
                                    edge_data=prob.nedge, node_data=prob.nnode)


def set_data(P, W, A):
    for k in range(W.shape[0]):
        P.set_edge_data(k, W[k])
    for k in range(A.shape[0]):
        P.set_node_data(k, A[k])


def problem(nls, pname, gname):
    """one compiled problem per case for the whole module, holding the seeded data and the table's parameters (whoever changes
    them puts them back)"""
    key = (pname, gname)
    if key not in _PROBLEMS:
        prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
        _PROBLEMS[key] = create(nls, prob, G)
        set_data(_PROBLEMS[key], *GC.data(prob, G))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("pname,gname", R.CASES)
def test_parity_with_the_restatement(nls, dev, pname, gname):
    """Residual, JVP, fill, the transposed product and fill·v for every (problem, graph) pair of the table, then the consistency
    of fill and JVP: the filled matrix times v against the dual JVP within the sum of the two bounds. single: no edge at all;
    directed3: a node of degree 0 and a nonsymmetric pattern; tri 17×15 / 16×16: one node short of a workgroup and exactly one;
    ring257: the self slot first, last and in the middle, one node past a workgroup; hub301: a degree above a workgroup, the
    slots of one node across several workgroups of the fill."""
    prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
    ref, P = GC.reference(prob, G), problem(nls, pname, gname)
    assert (P.nn, P.ne, P.dof) == (G.nn, G.ne, prob.dof)
    assert P.n_local == ref.u.size and P.jac_csr().info()["nnz"] == ref.vals.size == prob.dof ** 2 * (G.ne + G.nn)
    got = device_quantities(P, ref.u, ref.v, dev)
    for k in QUANTITIES:
        check(f"{pname} {gname} {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"))
    diff = np.abs(got["spmv"] - got["jv"])
    print(f"{pname} {gname} fill·v vs dual JVP: max {diff.max():.3e}")
    assert np.all(diff <= ref.spmv_bound + ref.jv_bound)


@pytest.mark.parametrize("pname,gname", [("powerflow", "hub301"), ("react4", "tri17x15p"), ("sink", "ring257")])
def test_two_evaluations_give_identical_bits(nls, dev, pname, gname):
    ref, P = GC.reference(R.PROBLEMS[pname], R.GRAPHS[gname]), problem(nls, pname, gname)
    a, b = device_quantities(P, ref.u, ref.v, dev), device_quantities(P, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("pname,gname", [("cubic", "tri9x7p"), ("powerflow", "directed3"), ("react4", "ring257"), ("sink", "hub301")])
def test_coloured_assembly_agrees_with_the_direct_fill(nls, dev, pname, gname):
    """nk_jac_values_colored — one dual JVP per colour of the pattern — against the direct fill and the restatement"""
    ref, P = GC.reference(R.PROBLEMS[pname], R.GRAPHS[gname]), problem(nls, pname, gname)
    u, J = to_device(ref.u, dev), P.jac_csr()
    P.jac_values(u, J)
    direct = np.array(J.values())
    ncolors = P.jac_values(u, J, colored=True)
    coloured = np.array(J.values())
    print(f"{pname} {gname}: {ncolors} colours")
    assert ncolors >= P.dof * (int(R.GRAPHS[gname].deg.max()) + 1)
    check(f"{pname} {gname} coloured vs restatement", coloured, ref.vals, ref.vals_bound)
    check(f"{pname} {gname} coloured vs direct fill", coloured, direct, ref.vals_bound)


def test_the_node_per_thread_fill_gives_the_same_bits(nls, dev, monkeypatch):
    """NK_GRAPH_FILL_NODE=1 at creation: the A/B form of the fill (one node per thread, the slots in an inner loop) evaluates
    and stores the same numbers"""
    for pname, gname in (("powerflow", "hub301"), ("react4", "tri17x15p")):
        prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
        ref, P = GC.reference(prob, G), problem(nls, pname, gname)
        monkeypatch.setenv("NK_GRAPH_FILL_NODE", "1")
        Q = create(nls, prob, G)
        monkeypatch.delenv("NK_GRAPH_FILL_NODE")
        set_data(Q, ref.W, ref.A)
        u = to_device(ref.u, dev)
        JP, JQ = P.jac_csr(), Q.jac_csr()
        P.jac_values(u, JP)
        Q.jac_values(u, JQ)
        assert np.array(JP.values()).tobytes() == np.array(JQ.values()).tobytes()
        Q.close()


# ------------------------------------------------------------------------------------------------ contract
def test_set_p_and_set_edge_data_change_the_residual_as_the_restatement_says(nls, dev):
    pname, gname = "sink", "tri9x7p"
    prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
    P = problem(nls, pname, gname)
    p1 = [1.25, -0.5]
    ref0, ref1 = GC.reference(prob, G), GC.reference(prob, G, params=p1)
    u, v = to_device(ref0.u, dev), to_device(ref0.v, dev)
    prob_ = nls.NonlinearProblem(P, to_device(ref0.u, dev), prob.params)
    cache = nls.init(prob_, nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES()), abstol=1e-10)
    check("fu after init", to_numpy(cache.fu), ref0.f, ref0.f_bound)
    nls.reinit_(cache, u0=to_device(ref0.u, dev), p=p1)
    check("fu after reinit_(p=...)", to_numpy(cache.fu), ref1.f, ref1.f_bound)
    assert float(np.max(np.abs(ref1.f - ref0.f))) > 1e6 * float(ref1.f_bound.max())
    # the Jacobian follows the parameters (a fill cached for the same u is not reused) …
    check("Jᵀv with the new p", to_numpy(P.vjp(v, u)), ref1.jtv, ref1.jtv_bound)
    P.set_p(prob.params)
    check("Jᵀv with the old p, same u buffer", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    # … and the data: another set of edge and node data, then the first again
    ref2 = GC.reference(prob, G, data_seed=2)
    assert float(np.max(np.abs(ref2.jtv - ref0.jtv))) > 1e6 * float(ref2.jtv_bound.max())
    set_data(P, ref2.W, ref2.A)
    assert np.array_equal(to_numpy(P.edge_data(0)), ref2.W[0]) and np.array_equal(to_numpy(P.node_data(1)), ref2.A[1])
    check("f with the new data", to_numpy(P.residual(u)), ref2.f, ref2.f_bound)
    check("Jᵀv with the new data, same u buffer", to_numpy(P.vjp(v, u)), ref2.jtv, ref2.jtv_bound)
    P.set_edge_data(0, to_device(ref0.W[0], dev))   # (from device memory)
    check("Jᵀv after the first edge datum is back, same u buffer", to_numpy(P.vjp(v, u)),
          GC.Reference(prob, G, ref0.u, ref0.v, ref0.W, ref2.A).jtv, ref2.jtv_bound + ref0.jtv_bound)
    set_data(P, ref0.W, ref0.A)
    check("Jᵀv with the old data", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    with pytest.raises(ValueError):
        P.set_p([1.0])
    with pytest.raises(ValueError):
        P.set_edge_data(0, np.zeros(G.ne + 1))
    cache.close()


def test_fresh_data_are_zero_and_undeclared_data_read_nan(nls, dev):
    prob, G = R.PROBLEMS["sink"], R.GRAPHS["tri6x5"]
    P = create(nls, prob, G)
    assert np.array_equal(to_numpy(P.edge_data(0)), np.zeros(G.ne)) and np.array_equal(to_numpy(P.node_data(1)), np.zeros(G.nn))
    u = np.linspace(-1, 1, G.nn)
    assert np.array_equal(to_numpy(P.residual(to_device(u, dev))), np.full(G.nn, -prob.params[1]))   # Σ 0·(…) + 0·u + 0·exp(u) − p1
    assert np.array_equal(to_numpy(P.initial_guess(device=True)), np.zeros(G.nn))
    P.close()
    Q = nls.CompiledGraphProblem(R.UNDECLARED_DATA_SRC, *G.csr(), node_data=1)   # the source reads u.a(1)
    assert np.all(np.isnan(to_numpy(Q.residual(to_device(u, dev)))))
    Q.close()


def test_two_sources_alive_at_once_and_a_fresh_problem_after_close(nls, dev):
    pa, pb, G = R.PROBLEMS["cubic"], R.PROBLEMS["react4"], R.GRAPHS["tri16x16p"]
    a, b = GC.reference(pa, G), GC.reference(pb, G)
    Pa, Pb = create(nls, pa, G), create(nls, pb, G)
    set_data(Pa, a.W, a.A)
    for _ in range(2):   # interleaved: each keeps its own kernels
        check("cubic beside react4", to_numpy(Pa.residual(to_device(a.u, dev))), a.f, a.f_bound)
        check("react4 beside cubic", to_numpy(Pb.jvp(to_device(b.v, dev), to_device(b.u, dev))), b.jv, b.jv_bound)
    Pa.close()
    check("react4 after cubic closed", to_numpy(Pb.residual(to_device(b.u, dev))), b.f, b.f_bound)
    Pb.close()
    Pb.close()
    Pc = create(nls, pa, G)
    set_data(Pc, a.W, a.A)
    check("a fresh cubic after close", to_numpy(Pc.residual(to_device(a.u, dev))), a.f, a.f_bound)
    Pc.close()


def test_runtime_errors_name_their_cause(nls, dev):
    prob, G = R.PROBLEMS["sink"], R.GRAPHS["tri6x5"]
    P = problem(nls, "sink", "tri6x5")
    with pytest.raises(nls.NKError, match="edge datum k = 1 outside 0..0"):
        P.set_edge_data(1, np.zeros(G.ne))
    with pytest.raises(nls.NKError, match="node datum k = 2 outside 0..1"):
        P.set_node_data(2, np.zeros(G.nn))
    with pytest.raises(nls.NKError, match="node datum k = -1"):
        P.node_data(-1)
    with pytest.raises(nls.NKError, match="dof = 5"):
        nls.CompiledGraphProblem(prob.source, *G.csr(), dof=5, params=prob.params, edge_data=1, node_data=2)
    with pytest.raises(nls.NKError, match="nedge = 5"):
        nls.CompiledGraphProblem(prob.source, *G.csr(), params=prob.params, edge_data=5, node_data=2)
    with pytest.raises(nls.NKError, match="row 1.*self-loop"):
        nls.CompiledGraphProblem(prob.source, [0, 1, 2], [1, 1], params=prob.params, edge_data=1, node_data=2)
    with pytest.raises(nls.NKError, match="nk_nbrs"):
        nls.CompiledGraphProblem(R.GRID_CONTRACT_SRC, *G.csr())
    # the data calls on a problem that is no compiled graph problem
    import ctypes as C
    from nonlinearsolve_jl_amd import _lib as L
    import grid_reference as GR
    B = nls.CompiledGridProblem(GR.BRATU_SRC, 5, 4, params=[1.0, 0.04])
    buf = np.zeros(20)
    for fn in (L.lib().nk_problem_set_graph_data, L.lib().nk_problem_get_graph_data):
        assert fn(B._h, 0, 0, C.c_void_p(buf.ctypes.data), L.HOST) == -1
        assert b"not a compiled graph problem" in L.lib().nk_last_error()
    B.close()
    # the geometric multigrid needs a grid: the message points to the AMG object
    g = nls.GMRES(P.n_local)
    with pytest.raises(nls.NKError, match="algebraic multigrid"):
        g.set_multigrid_preconditioner(P, to_device(np.zeros(P.n_local), dev))
    g.close()


# ------------------------------------------------------------------------------------------------ through the public interface
def _solve_case(nls, pname, G, seed=1):
    prob = R.PROBLEMS[pname]
    W, A = GC.data(prob, G, seed)
    P = create(nls, prob, G)
    set_data(P, W, A)
    u0 = np.zeros(prob.dof * G.nn)
    if pname == "powerflow":
        u0[G.nn:] = 1.0   # the flat start: θ = 0, V = 1
    u_ref, steps = GC.dense_newton(prob, G, u0, W, A)
    J_ref, f_ref = GC.dense_jacobian(prob, G, u_ref, W, A)
    print(f"{pname} {G.name}: dense Newton {steps} steps, |f(u_ref)|∞ {np.abs(f_ref).max():.3e}")
    assert 4 <= steps <= 8
    return P, u0, u_ref, J_ref


def test_sink_solves_with_gmres_and_the_amg_precs(nls, dev):
    """NewtonRaphson, GMRES, the aggregation AMG `precs` on the right, on tri(48, 48, permuted). J is a strictly diagonally
    dominant M-matrix with excess >= min κ = 0.05, so ‖J⁻¹‖∞ <= 20: ‖F‖∞ <= 1e-10 gives 2e-9, ×5 for the reference's own stop"""
    P, u0, u_ref, J_ref = _solve_case(nls, "sink", GC.tri(48, 48, 1, True))
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True)
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), alg, abstol=1e-10, maxiters=60)
    err = float(np.abs(to_numpy(sol.u) - u_ref).max())
    print(f"sink: {sol.retcode} {sol.stats}, |u - u_ref|∞ {err:.3e}")
    assert sol.retcode == "Success" and sol.stats.njacs >= sol.stats.nsteps > 0
    assert err <= 1e-8
    P.close()


def test_powerflow_solves_with_trust_region_on_the_concrete_jacobian(nls, dev):
    """TrustRegion with the linear solver of tests/test_gpu_grid_problem.py::test_solves_like_the_built_in (GMRES(60), 3000
    iterations), from the flat start on tri(16, 16, permuted): the same root as the dense Newton within 2·‖J_ref⁻¹‖∞·abstol"""
    abstol = 1e-9
    P, u0, u_ref, J_ref = _solve_case(nls, "powerflow", GC.tri(16, 16, 1, True))
    alg = nls.TrustRegion(linsolve=nls.KrylovJL_GMRES(gmres_restart=60, maxiters=3000), concrete_jac=True)
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), alg, abstol=abstol, maxiters=60)
    bound = 2.0 * float(np.abs(np.linalg.inv(J_ref)).sum(axis=1).max()) * abstol
    err = float(np.abs(to_numpy(sol.u) - u_ref).max())
    print(f"powerflow: {sol.retcode} {sol.stats}, |u - u_ref|∞ {err:.3e}, bound {bound:.3e}")
    assert sol.retcode == "Success" and sol.stats.njacs > 0
    assert err <= bound
    P.close()


def test_cubic_solves_matrix_free(nls, dev):
    abstol = 1e-10
    P, u0, u_ref, J_ref = _solve_case(nls, "cubic", R.GRAPHS["tri9x7p"])
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES()), abstol=abstol,
                    maxiters=60)
    bound = 2.0 * float(np.abs(np.linalg.inv(J_ref)).sum(axis=1).max()) * abstol
    err = float(np.abs(to_numpy(sol.u) - u_ref).max())
    print(f"cubic: {sol.retcode} {sol.stats}, |u - u_ref|∞ {err:.3e}, bound {bound:.3e}")
    assert sol.retcode == "Success" and sol.stats.njacs == 0 and sol.stats.op_applies >= sol.stats.gmres_iters > 0
    assert err <= bound
    P.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    for P in _PROBLEMS.values():
        P.close()
        P.close()
    _PROBLEMS.clear()
