"""Compiled element problems of several element blocks on the device (csrc/nk_elem.hip, "Blocks"): the block form of the
generated kernels and the one gather over all blocks against the NumPy restatement (tests/elemblk_core.py,
tests/elemblk_reference.py), entry by entry within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

(grid_core's rule), free and with fixed unknowns; the split meshes against the ONE-BLOCK problem on the same mesh bit for bit;
then the contract (reproducible bits, the coloured assembly, block data, parameters and fixed unknowns, fresh data, modules,
close, the runtime errors) and one solve through the public interface. Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import elem_reference as R1
import elemblk_core as BC
import elemblk_reference as R
from grid_device import QUANTITIES, check, device_quantities, to_device, to_numpy

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


def create(nls, prob, M, params=None):
    c, parts = M.conns32(), prob.parts
    return nls.CompiledElementProblem(parts[0].source, c[0], M.nn, dof=prob.dof, params=prob.params if params is None else params,
                                      node_data=prob.nnode, elem_data=parts[0].nelem,
                                      blocks=[nls.ElementBlock(p.source, cn, elem_data=p.nelem) for p, cn in zip(parts[1:], c[1:])])


def set_data(P, A, Ws):
    for k in range(A.shape[0]):
        P.set_node_data(k, A[k])
    for b, W in enumerate(Ws):
        for k in range(W.shape[0]):
            P.set_elem_data(k, W[k], block=b)


def set_fixed(P, ref):
    if ref.mask is None:
        P.set_fixed(np.zeros(P.n_local, dtype=np.int32))
    else:
        P.set_fixed(ref.mask, ref.values)


def problem(nls, pname, mname):
    """one compiled problem per case for the whole module, holding the seeded data and the table's parameters (whoever changes
    them puts them back; the mask is set by every user)"""
    key = (pname, mname)
    if key not in _PROBLEMS:
        prob, M = R.PROBLEMS[pname], R.MESHES[mname]
        _PROBLEMS[key] = create(nls, prob, M)
        set_data(_PROBLEMS[key], *BC.data(prob, M))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("pname,mname,masked", R.CASES)
def test_parity_with_the_restatement(nls, dev, pname, mname, masked):
    """Residual, JVP, fill, the transposed product and fill·v for every case, free and with fixed unknowns, then fill·v against
    the dual JVP within the sum of the two bounds. The indexed cases must agree bit for bit."""
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = BC.reference(prob, M, masked), problem(nls, pname, mname)
    set_fixed(P, ref)
    assert P.blocks == [(B.ne, B.npe, p.nelem) for B, p in zip(M.blocks, prob.parts)]
    assert (P.nn, P.ne, P.npe, P.dof) == (M.nn, M.blocks[0].ne, M.blocks[0].npe, prob.dof)
    assert P.n_local == ref.u.size and P.jac_csr().info()["nnz"] == ref.vals.size == prob.dof ** 2 * (M.G.ne + M.nn)
    got = device_quantities(P, ref.u, ref.v, dev)
    tag = f"{pname} {mname} {'fixed' if masked else 'free'}"
    for k in QUANTITIES:
        check(f"{tag} {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"), exact=pname in R.EXACT)
    diff = np.abs(got["spmv"] - got["jv"])
    print(f"{tag} fill·v vs dual JVP: max {diff.max():.3e}")
    assert np.all(diff <= ref.spmv_bound + ref.jv_bound)
    print(f"{tag}: bit for bit: " + ", ".join(k for k in QUANTITIES if np.array_equal(got[k], getattr(ref, k))))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pname,mname,one", R.SPLITS)
def test_a_split_mesh_gives_the_bits_of_the_one_block_problem(nls, dev, pname, mname, one, masked):
    """the same elements in the same order through two blocks and through one: F, J·v and the CSR values are the same bits,
    exp included — any difference is a defect of the block mechanism"""
    prob, M, M1 = R.PROBLEMS[pname], R.MESHES[mname], R1.MESHES["tri257p"]
    ref, P = BC.reference(prob, M, masked), problem(nls, pname, mname)
    key = ("one-block", one)
    if key not in _PROBLEMS:
        p1 = R1.PROBLEMS[one]
        _PROBLEMS[key] = nls.CompiledElementProblem(p1.source, M1.conn32(), M1.nn, dof=p1.dof, params=p1.params, node_data=p1.nnode)
        for k in range(ref.A.shape[0]):
            _PROBLEMS[key].set_node_data(k, ref.A[k])
    P1 = _PROBLEMS[key]
    set_fixed(P, ref)
    set_fixed(P1, ref)
    assert P1.blocks == [(M1.ne, 3, 0)] and len(P.blocks) == 2
    a, b = device_quantities(P, ref.u, ref.v, dev), device_quantities(P1, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals"):
        print(f"{pname} {mname} {'fixed' if masked else 'free'} {k}: {int(np.sum(a[k] != b[k]))} of {a[k].size} entries differ")
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("pname,mname", [("robin", "tri30+edges"), ("springs", "tri30+springs"), ("split-react2", "tri257p/256"),
                                         ("three", "tri30+edges+six")])
def test_two_evaluations_give_identical_bits(nls, dev, pname, mname):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = BC.reference(prob, M, True), problem(nls, pname, mname)
    set_fixed(P, ref)
    a, b = device_quantities(P, ref.u, ref.v, dev), device_quantities(P, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("pname,mname", [("robin", "tri30+edges"), ("springs", "tri30+springs"), ("points", "strip+points"),
                                         ("quadtri", "quadtri8x5")])
def test_coloured_assembly_agrees_with_the_direct_fill(nls, dev, pname, mname):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    ref, P = BC.reference(prob, M, True), problem(nls, pname, mname)
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
def test_block_data_parameters_and_fixed_unknowns_change_the_result_as_the_restatement_says(nls, dev):
    pname, mname = "three", "tri30+edges+six"
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    P = problem(nls, pname, mname)
    ref0 = BC.reference(prob, M)
    set_fixed(P, ref0)
    u, v = to_device(ref0.u, dev), to_device(ref0.v, dev)
    check("Jᵀv", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    # one datum of one block at a time; a Jacobian cached for the same u buffer is filled again
    ref2 = BC.reference(prob, M, data_seed=2)
    W = [w.copy() for w in ref0.Ws]
    for b, k in ((2, 3), (1, 0), (2, 0)):
        W[b][k] = ref2.Ws[b][k]
        P.set_elem_data(k, to_device(W[b][k], dev) if b == 1 else W[b][k], block=b)
        mixed = BC.Reference(prob, M, ref0.u, ref0.v, ref0.A, W)
        assert float(np.max(np.abs(mixed.jtv - ref0.jtv))) > 1e6 * float(mixed.jtv_bound.max())
        check(f"f with datum {k} of block {b} replaced", to_numpy(P.residual(u)), mixed.f, mixed.f_bound)
        check(f"Jᵀv with datum {k} of block {b} replaced, same u buffer", to_numpy(P.vjp(v, u)), mixed.jtv, mixed.jtv_bound)
        assert np.array_equal(to_numpy(P.elem_data(k, block=b)), W[b][k])
    set_data(P, ref0.A, ref0.Ws)
    check("Jᵀv with the old data", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    # the parameters reach every block (p1 is the bars' alone)
    p1 = [1.0, -0.75]
    ref1 = BC.reference(prob, M, params=p1)
    assert float(np.max(np.abs(ref1.jtv - ref0.jtv))) > 1e6 * float(ref1.jtv_bound.max())
    P.set_p(p1)
    check("f with the new p", to_numpy(P.residual(u)), ref1.f, ref1.f_bound)
    check("Jᵀv with the new p, same u buffer", to_numpy(P.vjp(v, u)), ref1.jtv, ref1.jtv_bound)
    P.set_p(prob.params)
    # the fixed unknowns
    ref3 = BC.reference(prob, M, True)
    P.set_fixed(ref3.mask, ref3.values)
    check("f with fixed unknowns", to_numpy(P.residual(u)), ref3.f, ref3.f_bound)
    check("Jᵀv with fixed unknowns, same u buffer", to_numpy(P.vjp(v, u)), ref3.jtv, ref3.jtv_bound)
    guess = to_numpy(P.initial_guess(device=True))
    assert np.array_equal(guess, np.where(ref3.mask != 0, ref3.values, 0.0)) and np.any(guess != 0)
    set_fixed(P, ref0)
    check("Jᵀv with nothing fixed again, same u buffer", to_numpy(P.vjp(v, u)), ref0.jtv, ref0.jtv_bound)
    with pytest.raises(ValueError):
        P.set_elem_data(0, np.zeros(M.blocks[2].ne + 1), block=2)
    with pytest.raises(ValueError):
        P.set_p([1.0])


def test_fresh_block_data_are_zero_and_a_datum_outside_the_blocks_count_reads_nan(nls, dev):
    prob, M = R.PROBLEMS["points"], R.MESHES["strip+points"]
    P = create(nls, prob, M)
    assert np.array_equal(to_numpy(P.elem_data(0, block=1)), np.zeros(3)) and np.array_equal(to_numpy(P.node_data(1)), np.zeros(M.nn))
    # the stiffness of the springs is still zero: with the coordinates set, the residual is the triangles' alone
    A, Ws = BC.data(prob, M)
    for k in range(2):
        P.set_node_data(k, A[k])
    u = np.linspace(-1, 1, M.nn)
    got = to_numpy(P.residual(to_device(u, dev)))
    ref = BC.Reference(prob, M, u, u, A, [Ws[0], np.zeros_like(Ws[1])])
    check("zero stiffness", got, ref.f, ref.f_bound)
    assert got[5] == 0.0
    P.close()
    # both blocks have one datum and read u.w(NK_BLOCK): block 0 its own datum 0 (zero), block 1 a datum 1 it does not have,
    # so only block 1's nodes turn NaN
    T = R1.MESHES["tri30"]
    src_w = "template <typename T> __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) { f[0] = u.at(0) + u.w(NK_BLOCK); }"
    Q = nls.CompiledElementProblem(src_w, np.array([[0], [1], [2]]), T.nn, elem_data=1,
                                   blocks=[nls.ElementBlock(src_w, np.array([[1], [4]]), elem_data=1)])
    out = to_numpy(Q.residual(to_device(np.ones(T.nn), dev)))
    assert np.array_equal(np.isnan(out), np.isin(np.arange(T.nn), [1, 4])) and out[0] == 1.0 and out[2] == 1.0 and out[3] == 0.0
    Q.close()


def test_a_blocks_problem_and_a_plain_one_alive_at_once_and_a_fresh_one_after_close(nls, dev):
    pb, Mb = R.PROBLEMS["robin"], R.MESHES["tri30+edges"]
    p1, M1 = R1.PROBLEMS["bratu"], R1.MESHES["tri30"]
    b = BC.reference(pb, Mb)
    import elem_core as EC
    a = EC.reference(p1, M1)
    Pb, Pa = create(nls, pb, Mb), nls.CompiledElementProblem(p1.source, M1.conn32(), M1.nn, params=p1.params, node_data=2)
    set_data(Pb, b.A, b.Ws)
    for k in range(2):
        Pa.set_node_data(k, a.A[k])
    for _ in range(2):   # interleaved: each keeps its own kernels and its own element buffers
        check("robin beside bratu", to_numpy(Pb.residual(to_device(b.u, dev))), b.f, b.f_bound)
        check("bratu beside robin", to_numpy(Pa.jvp(to_device(a.v, dev), to_device(a.u, dev))), a.jv, a.jv_bound)
    Pb.close()
    check("bratu after robin closed", to_numpy(Pa.residual(to_device(a.u, dev))), a.f, a.f_bound)
    Pa.close()
    Pa.close()
    Pc = create(nls, pb, Mb)
    set_data(Pc, b.A, b.Ws)
    check("a fresh robin after close", to_numpy(Pc.residual(to_device(b.u, dev))), b.f, b.f_bound)
    Pc.close()


def test_runtime_errors_name_their_cause(nls, dev):
    from nonlinearsolve_jl_amd import _lib as L
    import graph_reference as GR
    prob, M = R.PROBLEMS["three"], R.MESHES["tri30+edges+six"]
    P = problem(nls, "three", "tri30+edges+six")
    with pytest.raises(nls.NKError, match="block = 3 outside 0..2"):
        P.set_elem_data(0, np.zeros(4), block=3)
    with pytest.raises(nls.NKError, match="block = 3 outside 0..2"):
        P.elem_data(0, block=3)
    with pytest.raises(nls.NKError, match="block 1: element datum k = 1 outside 0..0"):
        P.set_elem_data(1, np.zeros(M.blocks[1].ne), block=1)
    with pytest.raises(nls.NKError, match="block 0: element datum k = 0 outside 0..-1"):
        P.elem_data(0)
    buf = np.zeros(64)
    assert L.lib().nk_problem_set_elem_block_data(P._h, -1, 0, C.c_void_p(buf.ctypes.data), L.HOST) == -1
    assert b"block = -1" in L.lib().nk_last_error()
    # the block calls on a one-block problem with block = 0, and its shape
    Q = nls.CompiledElementProblem(R1.PROBLEMS["tetdiff"].source, R1.MESHES["tet3x3x2"].conn32(), R1.MESHES["tet3x3x2"].nn,
                                   params=[0.5], node_data=4, elem_data=1)
    ne = R1.MESHES["tet3x3x2"].ne
    w = np.linspace(1, 2, ne)
    assert L.lib().nk_problem_set_elem_block_data(Q._h, 0, 0, C.c_void_p(w.ctypes.data), L.HOST) == 0
    assert np.array_equal(to_numpy(Q.elem_data(0)), w)
    out = np.zeros(ne)
    assert L.lib().nk_problem_get_elem_block_data(Q._h, 0, 0, C.c_void_p(out.ctypes.data), L.HOST) == 0 and np.array_equal(out, w)
    assert L.lib().nk_problem_get_elem_block_data(Q._h, 1, 0, C.c_void_p(out.ctypes.data), L.HOST) == -1
    assert b"block = 1 outside 0..0" in L.lib().nk_last_error()
    nb, nes, npes, nel = C.c_int(), (C.c_int64 * 8)(), (C.c_int * 8)(), (C.c_int * 8)()
    assert L.lib().nk_problem_elem_blocks(Q._h, C.byref(nb), 8, nes, npes, nel) == 0
    assert (nb.value, nes[0], npes[0], nel[0]) == (1, ne, 4, 1)
    assert L.lib().nk_problem_elem_blocks(P._h, C.byref(nb), 2, nes, npes, nel) == 0 and nb.value == 3
    assert [(nes[k], npes[k], nel[k]) for k in range(2)] == [(40, 3, 0), (18, 2, 1)]
    Q.close()
    # creation: the block and the element are named before anything is compiled; so is the block of a wrong source
    c = M.conns32()
    bad = c[1].copy()
    bad[5, 1] = M.nn
    with pytest.raises(nls.NKError, match=f"block 1, element 5: node {M.nn} .*outside 0..{M.nn - 1}"):
        nls.CompiledElementProblem("not compiled", c[0], M.nn, blocks=[nls.ElementBlock("not compiled", bad)])
    with pytest.raises(nls.NKError, match="block 1: nelem = 5"):
        nls.CompiledElementProblem("not compiled", c[0], M.nn, blocks=[nls.ElementBlock("not compiled", c[1], elem_data=5)])
    with pytest.raises(nls.NKError, match="nblocks = 9"):
        nls.CompiledElementProblem("not compiled", c[0], M.nn, blocks=[nls.ElementBlock("not compiled", c[1])] * 8)
    with pytest.raises(nls.NKError, match="element block 1 residual source does not compile.*nk_elemv"):
        nls.CompiledElementProblem(prob.parts[0].source, c[0], M.nn, params=prob.params, node_data=2,
                                   blocks=[nls.ElementBlock(R1.SYNTAX_ERROR_SRC, c[1])])
    # the graph-data setters on an element problem and the reverse
    for fn in (L.lib().nk_problem_set_graph_data, L.lib().nk_problem_get_graph_data):
        assert fn(P._h, 0, 0, C.c_void_p(buf.ctypes.data), L.HOST) == -1
        assert b"not a compiled graph problem" in L.lib().nk_last_error()
    gp, G = GR.PROBLEMS["indexed"], GR.GRAPHS["directed3"]
    B = nls.CompiledGraphProblem(gp.source, *G.csr(), dof=gp.dof, params=gp.params, edge_data=gp.nedge, node_data=gp.nnode)
    for fn in (L.lib().nk_problem_set_elem_block_data, L.lib().nk_problem_get_elem_block_data):
        assert fn(B._h, 0, 0, C.c_void_p(buf.ctypes.data), L.HOST) == -1
        assert b"not a compiled element problem" in L.lib().nk_last_error()
    assert L.lib().nk_problem_elem_blocks(B._h, C.byref(nb), 0, None, None, None) == -1
    assert b"not a compiled element problem" in L.lib().nk_last_error()
    B.close()


# ------------------------------------------------------------------------------------------------ through the public interface
def test_robin_solves_with_gmres_and_the_amg_precs(nls, dev):
    """P1 Bratu (λ = 0.1) with the radiation term (p1 = 0.2) on all boundary edges and one Dirichlet side (x = lo at 0.5; a larger
    λ has no solution with three radiating sides, from u = 0 the radiation term has no slope): NewtonRaphson on the
    concrete Jacobian, GMRES, the aggregation AMG `precs`. Within 2·‖J⁻¹‖∞·abstol of the dense Newton's root on the
    restatement (the rule of test_gpu_elem_problem.py::_assert_root)"""
    abstol, params = 1e-10, [0.1, 0.2]
    prob, M = R.PROBLEMS["robin"], R.MESHES["tri30+edges"]
    A, Ws = BC.data(prob, M)
    mask = np.zeros(M.nn, dtype=np.int32)
    mask[[i for i in M.boundary if i % 6 == 0]] = 1
    values = np.where(mask != 0, 0.5, 0.0)
    P = create(nls, prob, M, params)
    set_data(P, A, Ws)
    P.set_fixed(mask, values)
    u0 = to_numpy(P.initial_guess(device=True))
    assert np.array_equal(u0, values) and mask.sum() == 5
    u_ref, steps = BC.dense_newton(prob, M, u0, A, Ws, params=params, mask=mask, values=values)
    J_ref, f_ref = BC.dense_jacobian(prob, M, u_ref, A, Ws, params=params, mask=mask, values=values)
    print(f"robin: dense Newton {steps} steps, |f(u_ref)|∞ {np.abs(f_ref).max():.3e}")
    assert 3 <= steps <= 8 and np.abs(f_ref).max() <= 1e-13
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True)
    sol = nls.solve(nls.NonlinearProblem(P, to_device(u0, dev)), alg, abstol=abstol, maxiters=60)
    bound = 2.0 * float(np.abs(np.linalg.inv(J_ref)).sum(axis=1).max()) * abstol
    err = float(np.abs(to_numpy(sol.u) - u_ref).max())
    print(f"robin: {sol.retcode} {sol.stats}, |u - u_ref|∞ {err:.3e}, bound {bound:.3e}")
    assert sol.retcode == "Success" and sol.stats.njacs >= sol.stats.nsteps > 0
    assert err <= bound
    P.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    for P in _PROBLEMS.values():
        P.close()
        P.close()
    _PROBLEMS.clear()
