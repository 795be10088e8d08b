"""Compiled graph problems without a GPU: nk_graph_pattern against the NumPy pattern (tests/graph_core.py) and every documented
adjacency error with the row it names; the restatement against itself — its Jacobian against central differences of its own
residual, its vectorised residual against a node-by-node walk — with the defects those assertions must reject planted into
it; every source of tests/graph_reference.py through hiprtc for gfx950; and the generated kernels' resource notes (no private
segment)."""
import ctypes as C
import os

import numpy as np
import pytest

import graph_core as GC
import graph_reference as R
from nonlinearsolve_jl_amd import _lib as L
from test_grid_reference import LLVM, _kernel_notes

KERNELS = {0: ("nk_graph_residual", "nk_graph_jvp"), 1: ("nk_graph_jac",)}


def _nls():
    import nonlinearsolve_jl_amd as nls
    return nls


# ------------------------------------------------------------------------------------------------ the pattern
@pytest.mark.parametrize("dof", [1, 2, 4])
@pytest.mark.parametrize("gname", sorted(R.GRAPHS))
def test_pattern_equals_the_restatement(gname, dof):
    G = R.GRAPHS[gname]
    rp, ci = _nls().graph_pattern(*G.csr(), dof=dof)
    rp_ref, ci_ref = GC.pattern(G, dof)
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    # columns ascend strictly within every row, every row has dof·(deg + 1) entries, and the slot numbering is the header's
    inner = np.ones(ci.size, dtype=bool)
    inner[rp[:-1]] = False
    assert np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0)
    assert np.array_equal(np.diff(rp), np.tile(dof * (G.deg + 1), dof))
    S = G.ne + G.nn
    i, s = G.slot_node, G.slot_s
    for c in range(dof):
        for c2 in range(dof):
            at = c * dof * S + dof * (G.rowptr[i] + i) + c2 * (G.deg[i] + 1) + s
            col = np.where(s == G.spos[i], i, G.colind[np.minimum(G.rowptr[i] + s - (s > G.spos[i]), max(G.ne - 1, 0))] if G.ne else i)
            assert np.array_equal(ci[at], c2 * G.nn + col)


def test_the_graphs_are_what_the_table_says():
    g = R.GRAPHS
    assert (g["single"].nn, g["single"].ne) == (1, 0)
    assert g["directed3"].deg.tolist() == [1, 0, 1] and not g["directed3"].symmetric
    for name, nn in (("tri6x5", 30), ("tri9x7p", 63), ("tri17x15p", 255), ("tri16x16p", 256)):
        assert g[name].nn == nn and g[name].symmetric and g[name].deg.min() >= 2 and g[name].deg.max() <= 8
    r = g["ring257"]
    assert (r.spos[0], r.spos[256], r.spos[100]) == (0, 2, 1) and r.nn == 257
    h = g["hub301"]
    assert h.deg[150] == 300 and h.spos[150] == 150 and np.all(np.delete(h.deg, 150) == 3) and h.symmetric


def test_pattern_sizes_only():
    G = R.GRAPHS["tri9x7p"]
    rp, ci = G.csr()
    nnz = C.c_int64()
    prp, pci = C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data)
    assert L.lib().nk_graph_pattern(G.nn, prp, pci, 2, None, None, C.byref(nnz)) == 0
    assert nnz.value == 4 * (G.ne + G.nn)
    jrp = np.zeros(2 * G.nn + 1, dtype=np.int32)
    assert L.lib().nk_graph_pattern(G.nn, prp, pci, 2, C.c_void_p(jrp.ctypes.data), None, C.byref(nnz)) == 0
    assert jrp[-1] == nnz.value


def _pattern_error(rowptr, colind, dof=1):
    with pytest.raises(_nls().NKError) as ei:
        _nls().graph_pattern(np.array(rowptr, dtype=np.int32), np.array(colind, dtype=np.int32), dof=dof)
    return str(ei.value)


def test_adjacency_errors_name_the_row_and_the_rule():
    msg = _pattern_error([0, 2, 1, 3], [1, 2, 0])
    assert "row 1" in msg and "decreases" in msg
    msg = _pattern_error([0, 1, 2, 3], [1, 3, 0])
    assert "row 1" in msg and "column 3" in msg and "outside 0..2" in msg
    msg = _pattern_error([0, 1, 2, 3], [1, -1, 0])
    assert "row 1" in msg and "column -1" in msg
    msg = _pattern_error([0, 1, 3, 4], [1, 2, 2, 0])
    assert "row 1" in msg and "ascending" in msg and "duplicate" in msg
    msg = _pattern_error([0, 1, 3, 4], [1, 2, 0, 0])
    assert "row 1" in msg and "ascending" in msg
    msg = _pattern_error([0, 1, 2, 4], [1, 0, 1, 2])
    assert "row 2" in msg and "self-loop" in msg
    msg = _pattern_error([1, 1, 2], [0, 0])
    assert "row 0" in msg and "0-based" in msg
    msg = _pattern_error([0, 1, 2], [1, 0], dof=5)
    assert "dof = 5" in msg
    # the first offending row is the one named
    msg = _pattern_error([0, 1, 2, 3, 4], [1, 1, 2, 0])
    assert "row 1" in msg and "self-loop" in msg
    with pytest.raises(ValueError, match="colind has"):
        _nls().graph_pattern([0, 1, 2], [1])
    nnz = C.c_int64()
    rp = np.array([0, 0], dtype=np.int32)
    assert L.lib().nk_graph_pattern(0, C.c_void_p(rp.ctypes.data), None, 1, None, None, C.byref(nnz)) == -1
    assert b"nn = 0" in L.lib().nk_last_error()


# ------------------------------------------------------------------------------------------------ the restatement against itself
SELF_CHECK_CASES = [("sink", "tri9x7p"), ("cubic", "ring257"), ("powerflow", "tri6x5"), ("indexed", "directed3"),
                    ("indexed", "hub301"), ("react4", "tri9x7p"), ("react4", "directed3"), ("sink", "hub301"), ("sink", "single")]


def _jacobian_agrees_with_differences(prob, G, defect=None):
    """J·v and fill·v of the restatement against central differences of its own residual in long double, Jᵀv against the dense
    matrix of the values"""
    u, v = GC.inputs(prob, G)
    W, A = GC.data(prob, G)
    a = GC.evaluate(prob, G, u, v, W, A, defect=defect)
    h = GC.LD(2.0) ** -20
    uL, vL = u.astype(GC.LD), v.astype(GC.LD)
    up = GC.evaluate(prob, G, uL + h * vL, v, W, A, T=GC.LD, defect=defect).f
    um = GC.evaluate(prob, G, uL - h * vL, v, W, A, T=GC.LD, defect=defect).f
    fd = ((up - um) / (2 * h)).astype(np.float64)
    tol = 1e-8 * max(1.0, float(np.max(np.abs(fd))))   # O(h²) truncation
    rp, ci = GC.pattern(G, prob.dof)
    n = rp.size - 1
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = a.vals
    return bool(np.max(np.abs(fd - a.jv)) < tol and np.max(np.abs(fd - a.spmv)) < tol and
                np.allclose(dense.T @ v, a.jtv, rtol=0, atol=1e-12 * max(1.0, float(np.abs(a.vals).max()))))


def _vector_agrees_with_the_walk(prob, G, defect=None):
    """the vectorised residual against the node-by-node walk, within the residual's own bound"""
    u, v = GC.inputs(prob, G)
    W, A = GC.data(prob, G)
    a = GC.evaluate(prob, G, u, v, W, A, defect=defect)
    bound = GC.FLOOR_ULPS * GC.EPS * a.f_mag
    return bool(np.all(np.abs(a.f - GC.scalar_residual(prob, G, u, W, A)) <= bound))


@pytest.mark.parametrize("pname,gname", SELF_CHECK_CASES)
def test_restatement_jacobian_against_its_own_residual(pname, gname):
    prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
    assert _jacobian_agrees_with_differences(prob, G)
    assert _vector_agrees_with_the_walk(prob, G)
    ref = GC.reference(prob, G)
    assert np.all(np.abs(ref.spmv - ref.jv) <= ref.spmv_bound + ref.jv_bound)
    for k in ("f", "jv", "vals"):
        assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))


@pytest.mark.parametrize("defect,pname,gname,check", [
    ("self_slot_off_by_one", "sink", "ring257", _jacobian_agrees_with_differences),
    ("self_slot_off_by_one", "cubic", "hub301", _jacobian_agrees_with_differences),
    ("transposed_block", "react4", "tri9x7p", _jacobian_agrees_with_differences),
    ("transposed_block", "powerflow", "tri6x5", _jacobian_agrees_with_differences),
    ("no_self_seed", "sink", "tri9x7p", _jacobian_agrees_with_differences),
    ("no_self_seed", "react4", "single", _jacobian_agrees_with_differences),
    ("dropped_last_edge", "sink", "tri9x7p", _vector_agrees_with_the_walk),
    ("dropped_last_edge", "indexed", "directed3", _vector_agrees_with_the_walk),
    ("datum_by_neighbour", "sink", "tri9x7p", _vector_agrees_with_the_walk),
    ("datum_by_neighbour", "powerflow", "hub301", _vector_agrees_with_the_walk),
])
def test_the_assertions_reject_planted_defects(defect, pname, gname, check):
    prob, G = R.PROBLEMS[pname], R.GRAPHS[gname]
    assert defect in GC.DEFECTS
    assert check(prob, G) and not check(prob, G, defect=defect)


def test_slack_node_and_data_ranges():
    """the seeded data keep the ranges the solves were checked with, symmetric on a symmetric graph; node 0 is the slack node"""
    prob, G = R.PROBLEMS["powerflow"], R.GRAPHS["tri16x16p"]
    W, A = GC.data(prob, G)
    assert W[0].min() >= 0.5 and W[0].max() <= 1.5 and W[1].min() >= -8.0 and W[1].max() <= -4.0
    assert np.abs(A[0]).max() <= 0.3 and np.abs(A[1]).max() <= 0.1 and A[2].tolist() == [1.0] + [0.0] * (G.nn - 1)
    eo = G.edge_of()
    assert all(W[0, e] == W[0, eo[(j, i)]] for (i, j), e in eo.items())
    u = np.concatenate([np.zeros(G.nn), np.ones(G.nn)])
    f = GC.evaluate(prob, G, u, u, W, A).f
    assert f[0] == 0.0 and f[G.nn] == 0.0


# ------------------------------------------------------------------------------------------------ the sources through hiprtc
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    p = R.PROBLEMS[name]
    assert _nls().graph_compile_check(p.source, p.dof, len(p.params), p.nedge, p.nnode) > 2000


@pytest.mark.parametrize("src,token", [(R.GRID_CONTRACT_SRC, "nk_node"), (R.SYNTAX_ERROR_SRC, "no_such_symbol")])
def test_a_wrong_source_gets_the_contract_and_the_log(src, token):
    with pytest.raises(_nls().NKError) as ei:
        _nls().graph_compile_check(src, 1, 0, 0, 0)
    msg = str(ei.value)
    assert token in msg and "nk_node" in msg and "nk_nbrs" in msg and "nk_vertex" in msg and "u.nbr(e, c)" in msg


def test_count_errors_name_the_value():
    lib, nb, src = L.lib(), C.c_int64(), R.SINK_SRC.encode()
    for args, what in (((5, 2, 1, 2), "dof = 5"), ((0, 2, 1, 2), "dof = 0"), ((1, 33, 1, 2), "nparams = 33"),
                       ((1, 2, 5, 2), "nedge = 5"), ((1, 2, 1, -1), "nnode = -1")):
        assert lib.nk_graph_compile_check(src, *args, C.byref(nb)) == -1
        assert what in lib.nk_last_error().decode()


def _code_object(p, jac):
    nb = C.c_int64()
    args = (p.source.encode(), p.dof, len(p.params), p.nedge, p.nnode, jac)
    assert L.lib().nk_graph_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_graph_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_graph_code_object(*args, small, 16, C.byref(nb)) != 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, name):
    """all three kernels of every table problem are register programs: the view, the duals with their run-time seeds and the
    dof × dof block never reach scratch memory"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.access(readelf, os.X_OK):
        pytest.skip("llvm-readelf not installed")
    for jac, kernels in KERNELS.items():
        co = _code_object(R.PROBLEMS[name], jac)
        assert co[:4] == b"\x7fELF"
        path = tmp_path / f"{name}_{jac}.co"
        path.write_bytes(co)
        notes = _kernel_notes(readelf, path)
        assert set(notes) == set(kernels), sorted(notes)
        for k in kernels:
            print(f"{name}: {k}: private segment {notes[k][0]}, VGPRs {notes[k][1]}")
            assert notes[k][0] == 0, (k, notes)
