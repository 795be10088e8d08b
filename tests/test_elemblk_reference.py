"""Element blocks without a GPU: nk_elem_blocks_adjacency and nk_elem_blocks_pattern against the NumPy union graph
(tests/elemblk_core.py) and against nk_elem_pattern for one block; the sizes-only calls; every refusal with the block and the
element it names; the restatement against itself — its Jacobian against central differences of its own residual, its vectorised
residual against a scalar walk block after block — with the defects those assertions must reject planted into it; every source
of tests/elemblk_reference.py through hiprtc in the block form; and the block-form kernels' resource notes (no private segment)."""
import ctypes as C
import os

import numpy as np
import pytest

import elem_core as EC
import elem_reference as R1
import elemblk_core as BC
import elemblk_reference as R
import graph_core as GC
from nonlinearsolve_jl_amd import _lib as L
from test_grid_reference import LLVM, _kernel_notes

KERNELS = {0: ("nk_elem_residual", "nk_elem_jvp"), 1: ("nk_elem_jac",)}


def _nls():
    import nonlinearsolve_jl_amd as nls
    return nls


def _arrays(conns):
    """the parallel arrays of the C entry points (and what keeps them alive)"""
    cns = [np.ascontiguousarray(c, dtype=np.int32) for c in conns]
    k = len(cns)
    ne = (C.c_int64 * k)(*[c.shape[0] for c in cns])
    npe = (C.c_int * k)(*[c.shape[1] for c in cns])
    ptrs = (C.c_void_p * k)(*[c.ctypes.data for c in cns])
    return k, ne, npe, ptrs, cns


# ------------------------------------------------------------------------------------------------ the union graph and the pattern
@pytest.mark.parametrize("mname", sorted(R.MESHES))
def test_adjacency_is_the_union_graph(mname):
    M = R.MESHES[mname]
    c = M.conns32()
    rp, ci = _nls().elem_adjacency(c[0], M.nn, blocks=c[1:])
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, M.G.rowptr) and np.array_equal(ci, M.G.colind)
    assert M.G.symmetric


@pytest.mark.parametrize("dof", [1, 2])
@pytest.mark.parametrize("mname", sorted(R.MESHES))
def test_pattern_is_the_graph_pattern_of_the_union(mname, dof):
    M = R.MESHES[mname]
    c = M.conns32()
    rp, ci = _nls().elem_pattern(c[0], M.nn, dof=dof, blocks=c[1:])
    rp_ref, ci_ref = BC.pattern(M, dof)
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    grp, gci = _nls().graph_pattern(*_nls().elem_adjacency(c[0], M.nn, blocks=c[1:]), dof=dof)
    assert np.array_equal(rp, grp) and np.array_equal(ci, gci)


@pytest.mark.parametrize("mname", ["tri30", "quad7x5", "truss", "strip"])
def test_one_block_is_the_plain_pattern(mname):
    M = R1.MESHES[mname]
    for dof in (1, 2):
        a, b = _nls().elem_pattern(M.conn32(), M.nn, dof=dof, blocks=[]), _nls().elem_pattern(M.conn32(), M.nn, dof=dof)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = _nls().elem_adjacency(M.conn32(), M.nn, blocks=[]), _nls().elem_adjacency(M.conn32(), M.nn)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_bar_block_alone_creates_entries_and_a_point_block_none():
    M, T = R.MESHES["tri30+springs"], R1.MESHES["tri30"]
    for i, j in R.SPRINGS:
        assert j not in T.G.colind[T.G.rowptr[i]:T.G.rowptr[i + 1]] and j in M.G.colind[M.G.rowptr[i]:M.G.rowptr[i + 1]]
    assert M.G.ne == T.G.ne + 2 * len(R.SPRINGS)
    S, P = R1.MESHES["strip"], R.MESHES["strip+points"]
    assert np.array_equal(S.G.rowptr, P.G.rowptr) and np.array_equal(S.G.colind, P.G.colind) and P.G.deg[5] == 0
    assert len(R._EDGES30) == 18 and all(len(set(e)) == 2 for e in R._EDGES30)
    assert [b.npe for b in R.MESHES["tri2x8"].blocks] == [3, 2, 1, 3, 2, 1, 2, 1]


def test_sizes_only():
    M = R.MESHES["tri30+edges"]
    k, ne, npe, ptrs, _keep = _arrays(M.conns32())
    n = C.c_int64()
    assert L.lib().nk_elem_blocks_adjacency(M.nn, k, ne, npe, ptrs, None, None, C.byref(n)) == 0 and n.value == M.G.ne
    assert L.lib().nk_elem_blocks_pattern(M.nn, k, ne, npe, ptrs, 2, None, None, C.byref(n)) == 0 and n.value == 4 * (M.G.ne + M.nn)
    jrp = np.zeros(2 * M.nn + 1, dtype=np.int32)
    assert L.lib().nk_elem_blocks_pattern(M.nn, k, ne, npe, ptrs, 2, C.c_void_p(jrp.ctypes.data), None, C.byref(n)) == 0
    assert jrp[-1] == n.value


# ------------------------------------------------------------------------------------------------ refusals
def _error(conns, nn, dof=1):
    with pytest.raises(_nls().NKError) as ei:
        _nls().elem_pattern(np.array(conns[0], dtype=np.int32), nn, dof=dof, blocks=[np.array(c, dtype=np.int32) for c in conns[1:]])
    return str(ei.value)


def test_refusals_name_the_block_and_the_element():
    tri = [[0, 1, 2], [1, 3, 2]]
    msg = _error([tri, [[0, 1], [1, 2], [3, 4]]], 4)
    assert "block 1, element 2: node 4" in msg and "outside 0..3" in msg
    msg = _error([tri, [[0, 1]], [[2], [-1]]], 4)
    assert "block 2, element 1: node -1" in msg
    msg = _error([tri, [[0, 1], [2, 2]]], 4)
    assert "block 1, element 1: node 2 twice" in msg and "local nodes 0 and 1" in msg
    # the first offending block and element are the ones named
    msg = _error([[[0, 1, 2], [1, 1, 2]], [[9, 9]]], 4)
    assert "block 0, element 1" in msg and "twice" in msg
    msg = _error([tri, [[0, 9]], [[7, 7]]], 4)
    assert "block 1, element 0: node 9" in msg
    assert "block 1: npe = 9 outside 1..8" in _error([tri, [list(range(9))]], 9)
    assert "block 1: npe·dof = 8·4 = 32 exceeds 16" in _error([tri, [list(range(8))]], 8, dof=4)
    assert "dof = 5" in _error([tri, [[0, 1]]], 4, dof=5) and "dof = 0" in _error([tri, [[0, 1]]], 4, dof=0)
    assert "nn = 0" in _error([tri, [[0, 1]]], 0)
    with pytest.raises(ValueError, match="conn has shape"):
        _nls().elem_pattern(np.array(tri, dtype=np.int32), 4, blocks=[np.zeros((0, 2), dtype=np.int32)])


def test_refusals_of_the_c_entry_points():
    lib, n = L.lib(), C.c_int64()
    tri = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    k, ne, npe, ptrs, _keep = _arrays([tri] * 9)

    def err(rc):
        assert rc == -1
        return lib.nk_last_error().decode()

    assert "nblocks = 0 outside 1..8" in err(lib.nk_elem_blocks_adjacency(4, 0, ne, npe, ptrs, None, None, C.byref(n)))
    assert "nblocks = 9 outside 1..8" in err(lib.nk_elem_blocks_adjacency(4, 9, ne, npe, ptrs, None, None, C.byref(n)))
    assert "nblocks = 9" in err(lib.nk_elem_blocks_pattern(4, 9, ne, npe, ptrs, 1, None, None, C.byref(n)))
    assert lib.nk_elem_blocks_adjacency(4, 8, ne, npe, ptrs, None, None, C.byref(n)) == 0
    assert "NULL" in err(lib.nk_elem_blocks_adjacency(4, 2, None, npe, ptrs, None, None, C.byref(n)))
    # a NULL block, npe = 0 and 9, ne = 0: the block is named
    k, ne, npe, ptrs, _keep = _arrays([tri, tri[:, :2], tri])
    ptrs[1] = None
    assert "block 1, NULL conn" in err(lib.nk_elem_blocks_adjacency(4, 3, ne, npe, ptrs, None, None, C.byref(n)))
    k, ne, npe, ptrs, _keep = _arrays([tri, tri[:, :2], tri])
    npe[2] = 0
    assert "block 2: npe = 0 outside 1..8" in err(lib.nk_elem_blocks_adjacency(4, 3, ne, npe, ptrs, None, None, C.byref(n)))
    npe[2] = 9
    assert "block 2: npe = 9 outside 1..8" in err(lib.nk_elem_blocks_pattern(4, 3, ne, npe, ptrs, 1, None, None, C.byref(n)))
    npe[2] = 3
    ne[1] = 0
    assert "block 1: ne = 0" in err(lib.nk_elem_blocks_adjacency(4, 3, ne, npe, ptrs, None, None, C.byref(n)))
    # dof²·Σ npe²·ne must fit in int32: refused from the sizes alone, before any conn is read — each block fits, the sum does not
    ne[0], ne[1], ne[2] = 2 ** 26, 2 ** 27, 2 ** 27
    assert "block 2" in err(lib.nk_elem_blocks_pattern(10, 3, ne, npe, ptrs, 1, None, None, C.byref(n)))
    assert "exceeds INT32_MAX" in lib.nk_last_error().decode()
    # npe = 1 is allowed here and refused by the plain entry points, whose messages stay
    pt = np.array([[0], [3]], dtype=np.int32)
    k, ne, npe, ptrs, _keep = _arrays([pt])
    assert lib.nk_elem_blocks_adjacency(4, 1, ne, npe, ptrs, None, None, C.byref(n)) == 0 and n.value == 0
    assert "npe = 1 outside 2..8" in err(lib.nk_elem_adjacency(4, 2, 1, C.c_void_p(pt.ctypes.data), None, None, C.byref(n)))


def test_block_code_object_refusals():
    lib, nb, src = L.lib(), C.c_int64(), R1.BRATU_SRC.encode()
    for args, what in (((0, 0, 1, 1, 2, 0), "block 0: npe = 0"), ((3, 9, 1, 1, 2, 0), "block 3: npe = 9"), ((1, 3, 5, 1, 2, 0), "dof = 5"),
                       ((2, 8, 3, 1, 2, 0), "block 2: npe·dof = 8·3 = 24 exceeds 16"), ((0, 3, 1, 33, 2, 0), "nparams = 33"),
                       ((0, 3, 1, 1, 5, 0), "nnode = 5"), ((4, 3, 1, 1, 2, 5), "block 4: nelem = 5"), ((8, 3, 1, 1, 2, 0), "block = 8"),
                       ((-1, 3, 1, 1, 2, 0), "block = -1")):
        assert lib.nk_elem_block_code_object(src, *args, 0, None, 0, C.byref(nb)) == -1
        assert what in lib.nk_last_error().decode(), (what, lib.nk_last_error())


# ------------------------------------------------------------------------------------------------ the restatement against itself
def _setup(prob, M, masked):
    u, v = BC.inputs(prob, M)
    A, Ws = BC.data(prob, M)
    mask, values = BC.fixed(prob, M) if masked else (None, None)
    return u, v, A, Ws, mask, values


def _jacobian_agrees_with_differences(prob, M, masked=True, defect=None):
    """J·v and fill·v of the restatement against central differences of its own residual in long double, Jᵀv against the dense
    matrix of the values (the check of test_elem_reference.py)"""
    u, v, A, Ws, mask, values = _setup(prob, M, masked)
    kw = dict(mask=mask, values=values, defect=defect)
    a = BC.evaluate(prob, M, u, v, A, Ws, **kw)
    h = EC.LD(2.0) ** -20
    uL, vL = u.astype(EC.LD), v.astype(EC.LD)
    up = BC.evaluate(prob, M, uL + h * vL, v, A, Ws, T=EC.LD, **kw).f
    um = BC.evaluate(prob, M, uL - h * vL, v, A, Ws, T=EC.LD, **kw).f
    fd = ((up - um) / (2 * h)).astype(np.float64)
    tol = 1e-8 * max(1.0, float(np.max(np.abs(fd))), float(np.abs(a.vals).max()))   # O(h²) truncation
    rp, ci = BC.pattern(M, prob.dof)
    n = rp.size - 1
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = a.vals
    return bool(np.max(np.abs(fd - a.jv)) < tol and np.max(np.abs(fd - a.spmv)) < tol and
                np.allclose(dense.T @ v, a.jtv, rtol=0, atol=1e-12 * max(1.0, float(np.abs(a.vals).max()))))


def _vector_agrees_with_the_walk(prob, M, masked=True, defect=None, bitwise=False):
    """the vectorised residual against the element-by-element walk, block after block, within the residual's own bound;
    bitwise (sources without elementary functions): the same bits, which holds only in the same order of summation"""
    u, v, A, Ws, mask, values = _setup(prob, M, masked)
    a = BC.evaluate(prob, M, u, v, A, Ws, mask=mask, values=values, defect=defect)
    walk = BC.scalar_residual(prob, M, u, A, Ws, mask=mask, values=values)
    if bitwise:
        return bool(np.array_equal(a.f, walk))
    return bool(np.all(np.abs(a.f - walk) <= EC.FLOOR_ULPS * EC.EPS * a.f_mag))


def _vector_equals_the_walk(prob, M, masked=True, defect=None):
    return _vector_agrees_with_the_walk(prob, M, masked, defect, bitwise=True)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pname,mname", R.PAIRS)
def test_restatement_jacobian_against_its_own_residual(pname, mname, masked):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    assert _jacobian_agrees_with_differences(prob, M, masked)
    assert _vector_agrees_with_the_walk(prob, M, masked)
    if pname in R.EXACT:
        assert _vector_equals_the_walk(prob, M, masked)
    ref = BC.reference(prob, M, masked)
    assert np.all(np.abs(ref.spmv - ref.jv) <= ref.spmv_bound + ref.jv_bound)
    for k in ("f", "jv", "vals"):
        assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))
    if masked:
        fx = ref.mask != 0
        assert fx.any() and not fx.all()
        assert np.array_equal(ref.f[fx], (ref.u - ref.values)[fx]) and np.array_equal(ref.jv[fx], ref.v[fx])


@pytest.mark.parametrize("pname,mname,one", R.SPLITS)
def test_a_split_mesh_restates_the_one_block_problem_bit_for_bit(pname, mname, one):
    """the same source on the same elements in the same order: elem_core's evaluation of the uncut mesh gives the same bits"""
    prob, M, M1 = R.PROBLEMS[pname], R.MESHES[mname], R1.MESHES["tri257p"]
    ref = BC.reference(prob, M, True)
    e = EC.evaluate(R1.PROBLEMS[one], M1, ref.u, ref.v, ref.A, np.zeros((0, M1.ne)), mask=ref.mask, values=ref.values)
    for k in ("f", "jv", "vals", "jtv", "spmv"):
        assert np.array_equal(getattr(ref, k), getattr(e, k)), k
    assert np.array_equal(M.G.colind, M1.G.colind)


@pytest.mark.parametrize("defect,pname,mname,check", [
    ("blocks_reversed", "indexed", "tri30+edges+points", _vector_equals_the_walk),
    ("blocks_reversed", "eight", "tri2x8", _vector_equals_the_walk),
    ("base_dropped", "robin", "tri30+edges", _vector_agrees_with_the_walk),
    ("base_dropped", "quadtri", "quadtri8x5", _jacobian_agrees_with_differences),
    ("datum_stride_of_block0", "three", "tri30+edges+six", _vector_agrees_with_the_walk),
    ("block_off_by_one", "indexed", "tri30+edges+points", _vector_agrees_with_the_walk),
    ("block_off_by_one", "eight", "tri2x8", _vector_agrees_with_the_walk),
])
def test_the_assertions_reject_planted_defects(defect, pname, mname, check):
    prob, M = R.PROBLEMS[pname], R.MESHES[mname]
    assert defect in BC.DEFECTS
    assert check(prob, M) and not check(prob, M, defect=defect)


@pytest.mark.parametrize("mname", ["tri30+springs", "tri30+edges+six"])
def test_the_pattern_assertion_rejects_a_block_whose_pairs_are_missing(mname):
    """the comparison of test_adjacency_is_the_union_graph with the last block's pairs left out of the restatement's graph"""
    M = R.MESHES[mname]
    c = M.conns32()
    rp, ci = _nls().elem_adjacency(c[0], M.nn, blocks=c[1:])
    good = GC.Graph("g", M.nn, BC.union_pairs([b.conn for b in M.blocks]))
    bad = GC.Graph("b", M.nn, BC.union_pairs([b.conn for b in M.blocks], defect="pairs_missing"))
    assert "pairs_missing" in BC.DEFECTS
    assert np.array_equal(rp, good.rowptr) and np.array_equal(ci, good.colind)
    assert not (np.array_equal(rp, bad.rowptr) and np.array_equal(ci, bad.colind))


def test_the_running_sum_continues_from_block_to_block():
    """the plan of the restatement against a plain loop over blocks, then elements, then local nodes"""
    M = R.MESHES["tri30+edges+points"]
    rng = np.random.default_rng(6)
    total = sum(b.ne * b.npe for b in M.blocks)
    vals = rng.uniform(-1, 1, total) * 10.0 ** rng.integers(-8, 8, total)
    got = EC._Plan(np.concatenate([b.conn.ravel() for b in M.blocks]), M.nn)(vals, np.float64)
    want, q = np.zeros(M.nn), 0
    for b in M.blocks:
        for e in range(b.ne):
            for a in range(b.npe):
                want[b.conn[e, a]] += vals[q]
                q += 1
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the sources through hiprtc
def _code_object(part, prob, k, jac):
    nb = C.c_int64()
    args = (part.source.encode(), k, part.npe, prob.dof, len(prob.params), prob.nnode, part.nelem, jac)
    assert L.lib().nk_elem_block_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_elem_block_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_elem_block_code_object(*args, small, 16, C.byref(nb)) != 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_block_form_kernels_compile_for_gfx950_without_a_private_segment(tmp_path, name):
    """every source of every case compiled in the block form, with its block's NK_BLOCK, NK_NPE and NK_NELEM; all three
    kernels are register programs (the method of test_elem_reference.py::test_generated_kernels_have_no_private_segment)"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    have = os.access(readelf, os.X_OK)
    prob = R.PROBLEMS[name]
    for k, part in enumerate(prob.parts):
        for jac, kernels in KERNELS.items():
            co = _code_object(part, prob, k, jac)
            assert co[:4] == b"\x7fELF" and len(co) > 1000
            if not have:
                continue
            path = tmp_path / f"{name}_{k}_{jac}.co"
            path.write_bytes(co)
            notes = _kernel_notes(readelf, path)
            assert set(notes) == set(kernels), sorted(notes)
            for kn in kernels:
                print(f"{name} block {k}: {kn}: private segment {notes[kn][0]}, VGPRs {notes[kn][1]}")
                assert notes[kn][0] == 0, (kn, notes)
    if not have:
        pytest.skip("llvm-readelf not installed")


def test_a_wrong_block_source_names_its_block_before_the_contract_and_the_log():
    nb = C.c_int64()
    assert L.lib().nk_elem_block_code_object(R1.SYNTAX_ERROR_SRC.encode(), 2, 3, 1, 0, 0, 0, 0, None, 0, C.byref(nb)) == -1
    msg = L.lib().nk_last_error().decode()
    assert "element block 2 residual source does not compile" in msg
    assert msg.index("block 2") < msg.index("nk_elemv") < msg.index("no_such_symbol") and "NK_BLOCK" in msg
    # NK_BLOCK is defined in a plain problem too (0), so one source serves both
    assert _nls().elem_compile_check(R.BLOCK_INDEXED_SRC, 3, 1, 0, 1, 1) > 2000
