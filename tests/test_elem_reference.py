"""Compiled element problems without a GPU: nk_elem_adjacency and nk_elem_pattern against the NumPy node graph and pattern
(tests/elem_core.py) and against nk_graph_pattern of the adjacency; every documented mesh error and limit with the element it
names; the restatement against itself — its Jacobian against central differences of its own residual (fixed rows included), its
vectorised residual against an element-by-element walk — with the defects those assertions must reject planted into it; every
source of tests/elem_reference.py through hiprtc for gfx950; and the generated kernels' resource notes (no private segment)."""
import ctypes as C
import os

import numpy as np
import pytest

import elem_core as EC
import elem_reference as R
from nonlinearsolve_jl_amd import _lib as L
from test_grid_reference import LLVM, _kernel_notes

KERNELS = {0: ("nk_elem_residual", "nk_elem_jvp"), 1: ("nk_elem_jac",)}


def _nls():
    import nonlinearsolve_jl_amd as nls
    return nls


# ------------------------------------------------------------------------------------------------ the node graph and the pattern
@pytest.mark.parametrize("mname", sorted(R.MESHES))
def test_adjacency_equals_the_restatement(mname):
    M = R.MESHES[mname]
    rp, ci = _nls().elem_adjacency(M.conn32(), M.nn)
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, M.G.rowptr) and np.array_equal(ci, M.G.colind)
    assert M.G.symmetric


@pytest.mark.parametrize("dof", [1, 2, 4])
@pytest.mark.parametrize("mname", sorted(R.MESHES))
def test_pattern_equals_the_restatement_and_the_graph_pattern(mname, dof):
    M = R.MESHES[mname]
    if M.npe * dof > 16:
        with pytest.raises(_nls().NKError, match="exceeds 16"):
            _nls().elem_pattern(M.conn32(), M.nn, dof=dof)
        return
    rp, ci = _nls().elem_pattern(M.conn32(), M.nn, dof=dof)
    rp_ref, ci_ref = EC.pattern(M, dof)
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    grp, gci = _nls().graph_pattern(*_nls().elem_adjacency(M.conn32(), M.nn), dof=dof)
    assert np.array_equal(rp, grp) and np.array_equal(ci, gci)


def test_the_meshes_are_what_the_table_says():
    m = R.MESHES
    assert (m["tri1"].nn, m["tri1"].ne) == (3, 1) and (m["tri2"].nn, m["tri2"].ne) == (4, 2)
    assert [(m[k].nn, m[k].ne) for k in ("tri30", "tri255p", "tri256p", "tri257p")] == [(30, 40), (255, 448), (256, 450), (257, 452)]
    nat = EC.rectangle(17, 15, 1)
    assert not np.array_equal(nat.conn, m["tri255p"].conn) and sorted(map(sorted, nat.conn.tolist())) != sorted(map(sorted, m["tri255p"].conn.tolist()))
    f = m["fan300"]
    assert f.nn == 301 and f.ne == 300 and int(np.sum(f.conn == 150)) == 300 and f.G.deg[150] == 300
    s = m["strip"]
    assert sorted(set(range(14)) - set(s.conn.ravel().tolist())) == [5, 13] and s.G.deg[5] == 0 and s.G.deg[13] == 0
    assert (m["quad7x5"].ne, m["quad7x5"].npe) == (35, 4) and (m["tet3x3x2"].ne, m["tet3x3x2"].npe) == (108, 4)
    assert (m["hex3x2x2"].ne, m["hex3x2x2"].npe) == (12, 8)
    assert sorted(set(m["truss"].G.deg.tolist())) == [1, 2, 3, 4, 5, 6] and m["truss"].npe == 2
    # every triangle and quad is positively or negatively oriented but never degenerate; tets have volume
    for k in R.TRIANGLES:
        X, c = m[k].X, m[k].conn
        d = (X[0, c[:, 1]] - X[0, c[:, 0]]) * (X[1, c[:, 2]] - X[1, c[:, 0]]) - (X[0, c[:, 2]] - X[0, c[:, 0]]) * (X[1, c[:, 1]] - X[1, c[:, 0]])
        assert np.all(np.abs(d) > 1e-4), k


def test_sizes_only():
    M = R.MESHES["tri30"]
    cn = M.conn32()
    n = C.c_int64()
    pc = C.c_void_p(cn.ctypes.data)
    assert L.lib().nk_elem_adjacency(M.nn, M.ne, 3, pc, None, None, C.byref(n)) == 0 and n.value == M.G.ne
    assert L.lib().nk_elem_pattern(M.nn, M.ne, 3, pc, 2, None, None, C.byref(n)) == 0 and n.value == 4 * (M.G.ne + M.nn)
    jrp = np.zeros(2 * M.nn + 1, dtype=np.int32)
    assert L.lib().nk_elem_pattern(M.nn, M.ne, 3, pc, 2, C.c_void_p(jrp.ctypes.data), None, C.byref(n)) == 0 and jrp[-1] == n.value


def _mesh_error(conn, nn, dof=1):
    with pytest.raises(_nls().NKError) as ei:
        _nls().elem_pattern(np.array(conn, dtype=np.int32), nn, dof=dof)
    return str(ei.value)


def test_mesh_errors_name_the_element_and_the_rule():
    msg = _mesh_error([[0, 1, 2], [1, 2, 4]], 4)
    assert "element 1" in msg and "node 4" in msg and "outside 0..3" in msg
    msg = _mesh_error([[0, 1, 2], [1, -1, 2]], 4)
    assert "element 1" in msg and "node -1" in msg
    msg = _mesh_error([[0, 1, 2], [1, 3, 2], [3, 2, 3]], 4)
    assert "element 2" in msg and "node 3 twice" in msg and "local nodes 0 and 2" in msg
    # the first offending element is the one named
    msg = _mesh_error([[0, 1, 2], [2, 2, 9], [9, 9, 9]], 4)
    assert "element 1" in msg and "twice" in msg
    assert "npe = 1 " in _mesh_error([[0], [1]], 4)
    assert "npe = 9 " in _mesh_error([list(range(9))], 9)
    assert "dof = 5" in _mesh_error([[0, 1, 2]], 3, dof=5) and "dof = 0" in _mesh_error([[0, 1, 2]], 3, dof=0)
    assert "npe·dof = 8·4 = 32 exceeds 16" in _mesh_error([list(range(8))], 8, dof=4)
    assert "nn = 0" in _mesh_error([[0, 1, 2]], 0)
    with pytest.raises(ValueError, match="conn has shape"):
        _nls().elem_pattern(np.zeros((0, 3), dtype=np.int32), 3)
    n = C.c_int64()
    cn = np.zeros(3, dtype=np.int32)
    assert L.lib().nk_elem_adjacency(3, 0, 3, C.c_void_p(cn.ctypes.data), None, None, C.byref(n)) == -1
    assert b"ne = 0" in L.lib().nk_last_error()
    # ne·(npe·dof)² must fit in int32: refused from the sizes alone, before conn is read
    assert L.lib().nk_elem_pattern(10, 2 ** 23, 8, C.c_void_p(cn.ctypes.data), 2, None, None, C.byref(n)) == -1
    assert b"exceeds INT32_MAX" in L.lib().nk_last_error()


# ------------------------------------------------------------------------------------------------ the restatement against itself
SELF_CHECK_CASES = [("diffusion", "tri255p"), ("bratu", "fan300"), ("bratu", "strip"), ("react2", "tri30"), ("plap", "quad7x5"),
                    ("tetdiff", "tet3x3x2"), ("truss", "truss"), ("quad4", "quad7x5"), ("hex8", "hex3x2x2"), ("indexed3", "tri2"),
                    ("diffusion", "tri1")]


def _setup(prob, M, masked):
    u, v = EC.inputs(prob, M)
    A, W = EC.data(prob, M)
    mask, values = EC.fixed(prob, M) if masked else (None, None)
    return u, v, A, W, mask, values


def _jacobian_agrees_with_differences(prob, M, masked=True, defect=None):
    """J·v and fill·v of the restatement against central differences of its own residual in long double, Jᵀv against the dense
    matrix of the values"""
    u, v, A, W, mask, values = _setup(prob, M, masked)
    kw = dict(mask=mask, values=values, defect=defect)
    a = EC.evaluate(prob, M, u, v, A, W, **kw)
    h = EC.LD(2.0) ** -20
    uL, vL = u.astype(EC.LD), v.astype(EC.LD)
    up = EC.evaluate(prob, M, uL + h * vL, v, A, W, T=EC.LD, **kw).f
    um = EC.evaluate(prob, M, uL - h * vL, v, A, W, T=EC.LD, **kw).f
    fd = ((up - um) / (2 * h)).astype(np.float64)
    tol = 1e-8 * max(1.0, float(np.max(np.abs(fd))), float(np.abs(a.vals).max()))   # O(h²) truncation
    rp, ci = EC.pattern(M, prob.dof)
    n = rp.size - 1
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = a.vals
    return bool(np.max(np.abs(fd - a.jv)) < tol and np.max(np.abs(fd - a.spmv)) < tol and
                np.allclose(dense.T @ v, a.jtv, rtol=0, atol=1e-12 * max(1.0, float(np.abs(a.vals).max()))))


def _vector_agrees_with_the_walk(prob, M, masked=True, defect=None):
    """the vectorised residual against the element-by-element walk, within the residual's own bound"""
    u, v, A, W, mask, values = _setup(prob, M, masked)
    a = EC.evaluate(prob, M, u, v, A, W, mask=mask, values=values, defect=defect)
    bound = EC.FLOOR_ULPS * EC.EPS * a.f_mag
    return bool(np.all(np.abs(a.f - EC.scalar_residual(prob, M, u, A, W, mask=mask, values=values)) <= bound))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pname,mname", SELF_CHECK_CASES)
def test_restatement_jacobian_against_its_own_residual(pname, mname, masked):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    assert _jacobian_agrees_with_differences(prob, M, masked)
    assert _vector_agrees_with_the_walk(prob, M, masked)
    ref = EC.reference(prob, M, masked)
    assert np.all(np.abs(ref.spmv - ref.jv) <= ref.spmv_bound + ref.jv_bound)
    for k in ("f", "jv", "vals"):
        assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))
    if masked:   # the fixed rows are what the header says
        fx = ref.mask != 0
        assert fx.any() and not fx.all()
        assert np.array_equal(ref.f[fx], (ref.u - ref.values)[fx]) and np.array_equal(ref.jv[fx], ref.v[fx])
        J, _ = EC.dense_jacobian(prob, M, ref.u, ref.A, ref.W, mask=ref.mask, values=ref.values)
        assert np.array_equal(J[fx], np.eye(fx.size)[fx])
        free = EC.reference(prob, M, False)
        assert np.array_equal(ref.f[~fx], free.f[~fx]) and np.array_equal(J[~fx], EC.dense_jacobian(prob, M, ref.u, ref.A, ref.W)[0][~fx])


@pytest.mark.parametrize("defect,pname,mname,check", [
    ("ab_transposed", "diffusion", "tri30", _jacobian_agrees_with_differences),
    ("ab_transposed", "hex8", "hex3x2x2", _jacobian_agrees_with_differences),
    ("transposed_block", "react2", "tri30", _jacobian_agrees_with_differences),
    ("transposed_block", "quad4", "quad7x5", _jacobian_agrees_with_differences),
    ("dropped_last_element", "bratu", "fan300", _vector_agrees_with_the_walk),
    ("dropped_last_element", "tetdiff", "tet3x3x2", _vector_agrees_with_the_walk),
    ("datum_by_node", "tetdiff", "tet3x3x2", _vector_agrees_with_the_walk),
    ("datum_by_node", "truss", "truss", _vector_agrees_with_the_walk),
    ("fixed_row_left_as_sum", "bratu", "tri30", _vector_agrees_with_the_walk),
    ("fixed_row_left_as_sum", "react2", "strip", _vector_agrees_with_the_walk),
    ("fixed_offdiagonal_kept", "diffusion", "tri255p", _jacobian_agrees_with_differences),
    ("fixed_offdiagonal_kept", "react2", "tri30", _jacobian_agrees_with_differences),
])
def test_the_assertions_reject_planted_defects(defect, pname, mname, check):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    assert defect in EC.DEFECTS
    assert check(prob, M) and not check(prob, M, defect=defect)


def test_the_gather_adds_in_ascending_element_order_from_zero():
    """the plan of the restatement against a plain loop: a row's contributions in the order of the elements, whatever the
    order of the nodes inside them"""
    M = R.MESHES["tri255p"]
    rng = np.random.default_rng(5)
    vals = rng.uniform(-1, 1, M.ne * 3) * 10.0 ** rng.integers(-8, 8, M.ne * 3)
    got = EC._Plan(M.conn.ravel(), M.nn)(vals, np.float64)
    want = np.zeros(M.nn)
    for e in range(M.ne):
        for a in range(3):
            want[M.conn[e, a]] += vals[3 * e + a]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the sources through hiprtc
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    p = R.PROBLEMS[name]
    assert _nls().elem_compile_check(p.source, p.npe, p.dof, len(p.params), p.nnode, p.nelem) > 2000


@pytest.mark.parametrize("src,token", [(R.GRID_CONTRACT_SRC, "nk_element"), (R.SYNTAX_ERROR_SRC, "no_such_symbol")])
def test_a_wrong_source_gets_the_contract_and_the_log(src, token):
    with pytest.raises(_nls().NKError) as ei:
        _nls().elem_compile_check(src, 3, 1, 0, 0, 0)
    msg = str(ei.value)
    assert token in msg and "nk_element" in msg and "nk_elemv" in msg and "nk_cell" in msg and "u.at(a, c)" in msg


def test_count_errors_name_the_value():
    lib, nb, src = L.lib(), C.c_int64(), R.BRATU_SRC.encode()
    for args, what in (((1, 1, 1, 2, 0), "npe = 1"), ((9, 1, 1, 2, 0), "npe = 9"), ((3, 5, 1, 2, 0), "dof = 5"), ((3, 0, 1, 2, 0), "dof = 0"),
                       ((8, 3, 1, 2, 0), "exceeds 16"), ((3, 1, 33, 2, 0), "nparams = 33"), ((3, 1, 1, 5, 0), "nnode = 5"),
                       ((3, 1, 1, 2, -1), "nelem = -1")):
        assert lib.nk_elem_compile_check(src, *args, C.byref(nb)) == -1
        assert what in lib.nk_last_error().decode()


def _code_object(p, jac):
    nb = C.c_int64()
    args = (p.source.encode(), p.npe, p.dof, len(p.params), p.nnode, p.nelem, jac)
    assert L.lib().nk_elem_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_elem_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_elem_code_object(*args, small, 16, C.byref(nb)) != 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, name):
    """all three kernels of every table problem are register programs: the view, the duals with their run-time seeds, f[] (the
    sources' loops over the local nodes are unrolled) and the (npe·dof)² element matrix never reach scratch memory"""
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
