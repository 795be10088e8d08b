"""Compiled element problems on the device (csrc/nk_elem.hip): the generated element-residual, dual-number JVP and element-matrix
kernels and the gather against the NumPy restatement (tests/elem_core.py, tests/elem_reference.py), entry by entry within the
restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

(grid_core's rule), without a mask and with one, then the contract (reproducible bits, the coloured assembly, parameters, data
and fixed unknowns, modules, close, the runtime errors) and the solvers through the public interface. Every figure is printed
before it is asserted."""
import numpy as np
import pytest

import elem_core as EC
import elem_reference as R
from grid_device import QUANTITIES, check, device_quantities, to_device, to_numpy

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def create(nls, prob, M, params=None):
    return nls.CompiledElementProblem(prob.source, M.conn32(), M.nn, dof=prob.dof, params=prob.params if params is None else params,
                                      node_data=prob.nnode, elem_data=prob.nelem)


def set_data(P, A, W):
    for k in range(A.shape[0]):
        P.set_node_data(k, A[k])
    for k in range(W.shape[0]):
        P.set_elem_data(k, W[k])


def set_fixed(P, ref):
    """the mask and values of a reference, or nothing fixed"""
    if ref.mask is None:
        P.set_fixed(np.zeros(P.n_local, dtype=np.int32))
    else:
        P.set_fixed(ref.mask, ref.values)


def problem(nls, pname, mname):
    """one compiled problem per (problem, mesh) for the whole module, holding the seeded data and the table's parameters
    (whoever changes them puts them back; the mask is set by every user)"""
    key = (pname, mname)
    if key not in _PROBLEMS:
        prob, M = R.PROBLEMS[pname], R.MESHES[mname]
        _PROBLEMS[key] = create(nls, prob, M)
        set_data(_PROBLEMS[key], *EC.data(prob, M))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("pname,mname,masked", R.CASES)
def test_parity_with_the_restatement(nls, dev, pname, mname, masked):
    """Residual, JVP, fill, the transposed product and fill·v for every (problem, mesh) pair of the table, free and with fixed
    unknowns, then the consistency of fill and JVP: the filled matrix times v against the dual JVP within the sum of the two
    bounds. The indexed problems (no elementary function, integer data) must agree bit for bit."""
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = EC.reference(prob, M, masked), problem(nls, pname, mname)
    set_fixed(P, ref)
    assert (P.nn, P.ne, P.npe, P.dof) == (M.nn, M.ne, M.npe, prob.dof)
    assert P.n_local == ref.u.size and P.jac_csr().info()["nnz"] == ref.vals.size == prob.dof ** 2 * (M.G.ne + M.nn)
    got = device_quantities(P, ref.u, ref.v, dev)
    tag = f"{pname} {mname} {'fixed' if masked else 'free'}"
    for k in QUANTITIES:
        check(f"{tag} {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"), exact=pname in R.EXACT)
    diff = np.abs(got["spmv"] - got["jv"])
    print(f"{tag} fill·v vs dual JVP: max {diff.max():.3e}")
    assert np.all(diff <= ref.spmv_bound + ref.jv_bound)
    print(f"{tag}: bit for bit: " + ", ".join(k for k in QUANTITIES if np.array_equal(got[k], getattr(ref, k))))


@pytest.mark.parametrize("pname,mname", [("bratu", "fan300"), ("react2", "tri257p"), ("quad4", "quad7x5"), ("truss", "truss")])
def test_two_evaluations_give_identical_bits(nls, dev, pname, mname):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = EC.reference(prob, M, True), problem(nls, pname, mname)
    set_fixed(P, ref)
    a, b = device_quantities(P, ref.u, ref.v, dev), device_quantities(P, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("pname,mname", [("diffusion", "tri30"), ("react2", "strip"), ("tetdiff", "tet3x3x2"), ("bratu", "fan300")])
def test_coloured_assembly_agrees_with_the_direct_fill(nls, dev, pname, mname):
    """nk_jac_values_colored — one dual JVP per colour of the pattern — against the direct fill and the restatement, with fixed
    rows"""
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = EC.reference(prob, M, True), problem(nls, pname, mname)
    set_fixed(P, ref)
    u, J = to_device(ref.u, dev), P.jac_csr()
    P.jac_values(u, J)
    direct = np.array(J.values())
    ncolors = P.jac_values(u, J, colored=True)
    coloured = np.array(J.values())
    print(f"{pname} {mname}: {ncolors} colours; coloured == direct as numbers: {np.array_equal(coloured, direct)}")
    assert ncolors >= P.dof * (int(M.G.deg.max()) + 1)
    check(f"{pname} {mname} coloured vs restatement", coloured, ref.vals, ref.vals_bound)
    check(f"{pname} {mname} coloured vs direct fill", coloured, direct, ref.vals_bound)


# ------------------------------------------------------------------------------------------------ contract
def test_parameters_data_and_fixed_unknowns_change_the_result_as_the_restatement_says(nls, dev):
    pname, mname = "tetdiff", "tet3x3x2"
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    P = problem(nls, pname, mname)
    p1 = [-1.25]
    ref0, ref1 = EC.reference(prob, M), EC.reference(prob, M, params=p1)
    set_fixed(P, ref0)
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
    # … the data: another set of node and element data, one array at a time …
    ref2 = EC.reference(prob, M, data_seed=2)
    assert float(np.max(np.abs(ref2.jtv - ref0.jtv))) > 1e6 * float(ref2.jtv_bound.max())
    P.set_elem_data(0, ref2.W[0])
    mixed = EC.Reference(prob, M, ref0.u, ref0.v, ref0.A, ref2.W)
    assert float(np.max(np.abs(mixed.jtv - ref0.jtv))) > 1e6 * float(mixed.jtv_bound.max())
    check("f with the new element datum", to_numpy(P.residual(u)), mixed.f, mixed.f_bound)
    check("Jᵀv with the new element datum, same u buffer", to_numpy(P.vjp(v, u)), mixed.jtv, mixed.jtv_bound)
    P.set_node_data(3, to_device(ref2.A[3], dev))   # (from device memory)
    assert np.array_equal(to_numpy(P.elem_data(0)), ref2.W[0]) and np.array_equal(to_numpy(P.node_data(3)), ref2.A[3])
    check("f with the new source term too", to_numpy(P.residual(u)), ref2.f, ref2.f_bound)
    check("Jᵀv with the new data, same u buffer", to_numpy(P.vjp(v, u)), ref2.jtv, ref2.jtv_bound)
    set_data(P, ref0.A, ref0.W)
    check("Jᵀv with the old data", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    # … and the fixed unknowns: a mask with values, another set of values, then nothing fixed
    ref3 = EC.reference(prob, M, True)
    assert float(np.max(np.abs(ref3.jtv - ref0.jtv))) > 1e6 * float(ref3.jtv_bound.max())
    P.set_fixed(ref3.mask, ref3.values)
    m, g = P.fixed()
    assert m.dtype == np.int32 and np.array_equal(m, ref3.mask) and np.array_equal(g, ref3.values)
    check("f with fixed unknowns", to_numpy(P.residual(u)), ref3.f, ref3.f_bound)
    check("Jᵀv with fixed unknowns, same u buffer", to_numpy(P.vjp(v, u)), ref3.jtv, ref3.jtv_bound)
    guess = to_numpy(P.initial_guess(device=True))
    assert np.array_equal(guess, np.where(ref3.mask != 0, ref3.values, 0.0)) and np.any(guess != 0)
    P.set_fixed(ref3.mask)   # values = None: zeros
    fx = ref3.mask != 0
    f = to_numpy(P.residual(u))
    assert np.array_equal(f[fx], ref0.u[fx]) and np.array_equal(f[~fx], ref3.f[~fx])
    assert np.array_equal(P.fixed()[1], np.zeros(P.n_local))
    set_fixed(P, ref0)
    check("Jᵀv with nothing fixed again, same u buffer", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    with pytest.raises(ValueError):
        P.set_p([1.0, 2.0])
    with pytest.raises(ValueError):
        P.set_elem_data(0, np.zeros(M.ne + 1))
    with pytest.raises(ValueError):
        P.set_fixed(np.zeros(M.nn + 1))
    cache.close()


def test_fresh_data_are_zero_and_undeclared_data_read_nan(nls, dev):
    prob, M = R.PROBLEMS["hex8"], R.MESHES["hex3x2x2"]
    P = create(nls, prob, M)
    assert np.array_equal(to_numpy(P.elem_data(0)), np.zeros(M.ne)) and np.array_equal(to_numpy(P.node_data(0)), np.zeros(M.nn))
    m, g = P.fixed()
    assert not m.any() and not g.any()
    u = np.linspace(-1, 1, M.nn)
    count = np.bincount(M.conn.ravel(), minlength=M.nn)
    got = to_numpy(P.residual(to_device(u, dev)))   # 0·(…) + 0.125·(p1·u − 0) per element of the node, added one by one
    want = np.zeros(M.nn)
    for _ in range(int(count.max())):
        want = np.where(count > 0, want + 0.125 * (prob.params[1] * u - 0.0), want)
        count = count - 1
    assert np.array_equal(got, want)
    assert np.array_equal(to_numpy(P.initial_guess(device=True)), np.zeros(M.nn))
    P.close()
    T = R.MESHES["tri30"]
    Q = nls.CompiledElementProblem(R.UNDECLARED_DATA_SRC, T.conn32(), T.nn, node_data=1)   # reads u.x(0, 1), u.w(0), u.at(3)
    assert np.all(np.isnan(to_numpy(Q.residual(to_device(np.linspace(-1, 1, T.nn), dev)))))
    Q.close()


def test_two_sources_alive_at_once_and_a_fresh_problem_after_close(nls, dev):
    pa, pb, M = R.PROBLEMS["diffusion"], R.PROBLEMS["react2"], R.MESHES["tri256p"]
    a, b = EC.reference(pa, M), EC.reference(pb, M)
    Pa, Pb = create(nls, pa, M), create(nls, pb, M)
    set_data(Pa, a.A, a.W)
    set_data(Pb, b.A, b.W)
    for _ in range(2):   # interleaved: each keeps its own kernels and its own element buffers
        check("diffusion beside react2", to_numpy(Pa.residual(to_device(a.u, dev))), a.f, a.f_bound)
        check("react2 beside diffusion", to_numpy(Pb.jvp(to_device(b.v, dev), to_device(b.u, dev))), b.jv, b.jv_bound)
    Pa.close()
    check("react2 after diffusion closed", to_numpy(Pb.residual(to_device(b.u, dev))), b.f, b.f_bound)
    Pb.close()
    Pb.close()
    Pc = create(nls, pa, M)
    set_data(Pc, a.A, a.W)
    check("a fresh diffusion after close", to_numpy(Pc.residual(to_device(a.u, dev))), a.f, a.f_bound)
    Pc.close()


def test_runtime_errors_name_their_cause(nls, dev):
    prob, M = R.PROBLEMS["tetdiff"], R.MESHES["tet3x3x2"]
    P = problem(nls, "tetdiff", "tet3x3x2")
    with pytest.raises(nls.NKError, match="element datum k = 1 outside 0..0"):
        P.set_elem_data(1, np.zeros(M.ne))
    with pytest.raises(nls.NKError, match="node datum k = 4 outside 0..3"):
        P.set_node_data(4, np.zeros(M.nn))
    with pytest.raises(nls.NKError, match="node datum k = -1"):
        P.node_data(-1)
    kw = dict(params=prob.params, node_data=4, elem_data=1)
    with pytest.raises(nls.NKError, match="dof = 5"):
        nls.CompiledElementProblem(prob.source, M.conn32(), M.nn, dof=5, **kw)
    with pytest.raises(nls.NKError, match="nelem = 5"):
        nls.CompiledElementProblem(prob.source, M.conn32(), M.nn, params=prob.params, node_data=4, elem_data=5)
    first = int(np.flatnonzero((M.conn == M.nn - 1).any(axis=1))[0])
    with pytest.raises(nls.NKError, match=f"element {first}: node {M.nn - 1} .*outside 0..{M.nn - 2}"):
        nls.CompiledElementProblem(prob.source, M.conn32(), M.nn - 1, **kw)
    bad = M.conn32().copy()
    bad[7, 3] = bad[7, 1]
    with pytest.raises(nls.NKError, match="element 7: node .* twice"):
        nls.CompiledElementProblem(prob.source, bad, M.nn, **kw)
    with pytest.raises(nls.NKError, match="nk_elemv"):
        nls.CompiledElementProblem(R.GRID_CONTRACT_SRC, M.conn32(), M.nn)
    # the data and fixed-unknown calls on a problem that is no compiled element problem
    import ctypes as C
    from nonlinearsolve_jl_amd import _lib as L
    import grid_reference as GR
    B = nls.CompiledGridProblem(GR.BRATU_SRC, 5, 4, params=[1.0, 0.04])
    buf, ibuf = np.zeros(20), np.zeros(20, dtype=np.int32)
    for fn in (L.lib().nk_problem_set_elem_data, L.lib().nk_problem_get_elem_data):
        assert fn(B._h, 0, 0, C.c_void_p(buf.ctypes.data), L.HOST) == -1
        assert b"not a compiled element problem" in L.lib().nk_last_error()
    for fn in (L.lib().nk_problem_set_elem_fixed, L.lib().nk_problem_get_elem_fixed):
        assert fn(B._h, C.c_void_p(ibuf.ctypes.data), C.c_void_p(buf.ctypes.data), L.HOST) == -1
        assert b"not a compiled element problem" in L.lib().nk_last_error()
    B.close()
    # the geometric multigrid needs a grid: the message points to the AMG object
    g = nls.GMRES(P.n_local)
    with pytest.raises(nls.NKError, match="algebraic multigrid"):
        g.set_multigrid_preconditioner(P, to_device(np.zeros(P.n_local), dev))
    g.close()


# ------------------------------------------------------------------------------------------------ through the public interface
def _solve_case(nls, pname, M, mask, values, params):
    """the problem with its data and fixed unknowns, the start (zeros with the fixed values written in: initial_guess), the dense
    Newton's root on the restatement and the Jacobian there"""
    prob = R.PROBLEMS[pname]
    A, W = EC.data(prob, M)
    P = create(nls, prob, M, params)
    set_data(P, A, W)
    P.set_fixed(mask, values)
    u0 = to_numpy(P.initial_guess(device=True))
    assert np.array_equal(u0, np.where(mask != 0, 0.0 if values is None else values, 0.0))
    u_ref, steps = EC.dense_newton(prob, M, u0, A, W, params=params, mask=mask, values=values)
    J_ref, f_ref = EC.dense_jacobian(prob, M, u_ref, A, W, params=params, mask=mask, values=values)
    print(f"{pname} {M.name}: dense Newton {steps} steps, |f(u_ref)|∞ {np.abs(f_ref).max():.3e}")
    assert 3 <= steps <= 8 and np.abs(f_ref).max() <= 1e-13
    return P, u0, u_ref, J_ref


def _assert_root(sol, u_ref, J_ref, abstol, what):
    """within 2·‖J_ref⁻¹‖∞·abstol of the dense Newton's root: ‖F(u)‖∞ <= abstol moves u by at most ‖J⁻¹‖∞·abstol to first order,
    and the factor 2 covers the second order and the reference's own stop (the rule of test_gpu_graph_problem.py)"""
    bound = 2.0 * float(np.abs(np.linalg.inv(J_ref)).sum(axis=1).max()) * abstol
    err = float(np.abs(to_numpy(sol.u) - u_ref).max())
    print(f"{what}: {sol.retcode} {sol.stats}, |u - u_ref|∞ {err:.3e}, bound {bound:.3e}")
    assert sol.retcode == "Success"
    assert err <= bound


def test_bratu_solves_with_gmres_and_the_amg_precs(nls, dev):
    """P1 Bratu (λ = 5) on a renumbered 24 × 24 triangulation with its boundary fixed at 0: NewtonRaphson, GMRES, the
    aggregation AMG `precs` on the right, on the concrete Jacobian"""
    abstol = 1e-10
    M = EC.renumbered(EC.rectangle(24, 24, 1), 4)
    mask = np.zeros(M.nn, dtype=np.int32)
    mask[M.boundary] = 1
    P, u0, u_ref, J_ref = _solve_case(nls, "bratu", M, mask, None, [5.0])
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True)
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), alg, abstol=abstol, maxiters=60)
    assert sol.stats.njacs >= sol.stats.nsteps > 0
    _assert_root(sol, u_ref, J_ref, abstol, "bratu")
    P.close()


def test_truss_solves_with_trust_region_on_the_concrete_jacobian(nls, dev):
    """the truss with its supports (nodes 1, 5, 6, both components) fixed and a body load in p"""
    abstol = 1e-9
    M = R.MESHES["truss"]
    mask = np.zeros((2, M.nn), dtype=np.int32)
    mask[:, M.boundary] = 1
    P, u0, u_ref, J_ref = _solve_case(nls, "truss", M, mask.ravel(), None, [0.0, -0.05])
    alg = nls.TrustRegion(linsolve=nls.KrylovJL_GMRES(gmres_restart=60, maxiters=3000), concrete_jac=True)
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), alg, abstol=abstol, maxiters=60)
    assert sol.stats.njacs > 0
    _assert_root(sol, u_ref, J_ref, abstol, "truss")
    P.close()


def test_tet_diffusion_solves_matrix_free(nls, dev):
    """tet diffusion with nonzero fixed values on two faces (0.5 on x = lo, −0.25 on x = hi), matrix-free Newton–GMRES"""
    abstol = 1e-10
    M = R.MESHES["tet3x3x2"]
    mask = np.zeros(M.nn, dtype=np.int32)
    mask[M.boundary] = 1
    values = np.where(mask != 0, np.where(M.X[0] < 0.5, 0.5, -0.25), 0.0)
    P, u0, u_ref, J_ref = _solve_case(nls, "tetdiff", M, mask, values, [4.0])
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES()), abstol=abstol,
                    maxiters=60)
    assert sol.stats.njacs == 0 and sol.stats.op_applies >= sol.stats.gmres_iters > 0
    _assert_root(sol, u_ref, J_ref, abstol, "tetdiff")
    P.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    for P in _PROBLEMS.values():
        P.close()
        P.close()
    _PROBLEMS.clear()
