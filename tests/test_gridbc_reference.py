"""Compiled grid problems with a boundary kind per side, without a GPU: the restatement (tests/grid_core.py, tests/gridbc_reference.py) against itself
(analytic merged Jacobians against differences of its own long-double residual; its index maps against examples written out by
hand), nk_grid_pattern / nk_grid3_pattern against its pattern for every case, every source through the compile-check entry
points for gfx950, the canonical form of the boundary code (a packed all-periodic or all-Dirichlet code gives the code objects
of 1 and 0, byte for byte), the argument errors with their messages, the generated kernels' resource notes (no private segment),
and that the conservation test of the device suite cannot pass vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid3_reference as G3
import grid_core as GC
import grid_reference as G1
import gridbc_reference as R
import gridf_reference as GF
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
KERNELS = {2: {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)},
           3: {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}}
MN, MF, DI, PE = "mirror_node", "mirror_face", "dirichlet", "periodic"
_CASES = [(name, shape) for name in sorted(R.PROBLEMS) for shape in R.sizes(R.PROBLEMS[name])]
_IDS = [f"{n}-{'x'.join(map(str, s))}" for n, s in _CASES]


# ------------------------------------------------------------------------------------------------ the restatement against itself
def test_index_maps_are_numpy_pads():
    """positions −2 … n+1 of an axis of 5 nodes, written out"""
    assert list(GC.axis_map(5, DI, DI)) == [-1, -1, 0, 1, 2, 3, 4, -1, -1]
    assert list(GC.axis_map(5, PE, PE)) == [3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert list(GC.axis_map(5, MN, MN)) == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert list(GC.axis_map(5, MF, MF)) == [1, 0, 0, 1, 2, 3, 4, 4, 3]
    assert list(GC.axis_map(5, MN, DI)) == [2, 1, 0, 1, 2, 3, 4, -1, -1]
    assert list(GC.axis_map(3, MF, MN)) == [1, 0, 0, 1, 2, 1, 0]
    # u and a field next to each other: x mirror-node, y Dirichlet — the Dirichlet side wins at the corner
    F = np.array([[10.0 * j + i for i in range(3)] for j in range(3)])[None]
    U, A = GC.Grid(F, (MN, MN, DI, DI)), GC.Fields(F, (MN, MN, DI, DI))
    assert np.array_equal(U(-1, 0), [[1, 0, 1], [11, 10, 11], [21, 20, 21]])
    assert np.array_equal(U(-1, -1), [[0, 0, 0], [1, 0, 1], [11, 10, 11]])
    assert np.array_equal(A(-1, -1), [[0, 1, 2], [1, 0, 1], [11, 10, 11]])      # outside: the field at the node itself
    assert np.array_equal(U(1, 1), [[11, 12, 11], [21, 22, 21], [0, 0, 0]])


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_restatement_jacobians_against_its_own_residual(name):
    """the merged analytic Jacobian the device is held against: J·v and the CSR values against central differences of the
    restatement's residual in long double, Jᵀv against the values; at the smallest shape (every row at a wall) and at 6 × 5
    (7 × 6 × 5)"""
    prob = R.PROBLEMS[name]
    for shape in (R.sizes(prob)[0], (7, 6, 5) if prob.dim == 3 else (6, 5)):
        ref = GC.reference(prob, shape)
        h = GC.LD(2.0) ** -20
        up = GC.evaluate(prob, shape, ref.u.astype(GC.LD) + h * ref.v.astype(GC.LD), ref.v, ref.fields, T=GC.LD).f
        um = GC.evaluate(prob, shape, ref.u.astype(GC.LD) - h * ref.v.astype(GC.LD), ref.v, ref.fields, T=GC.LD).f
        fd = ((up - um) / (2 * h)).astype(np.float64)
        assert np.max(np.abs(fd - ref.jv)) < 1e-8 * max(1.0, np.max(np.abs(ref.jv)))   # O(h²) truncation
        assert np.all(np.abs(ref.spmv - ref.jv) <= ref.spmv_bound + ref.jv_bound)
        rp, ci = GC.pattern(shape, prob.dof, prob.offsets(), prob.sides)
        dense = np.zeros((rp.size - 1, rp.size - 1))
        dense[np.repeat(np.arange(rp.size - 1), np.diff(rp)), ci] = ref.vals
        assert np.allclose(dense.T @ ref.v, ref.jtv, rtol=0, atol=1e-12 * np.abs(ref.vals).max())
        for k in ("f", "jv", "vals"):
            assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))


# ------------------------------------------------------------------------------------------------ the library's pattern
def _lib_pattern(prob, shape):
    lib, nnz = L.lib(), C.c_int64()
    code, st = GC.sides_code(prob.boundary), GC.STENCIL_ID[prob.stencil]
    if prob.dim == 3:
        def call(rp, ci):
            return lib.nk_grid3_pattern(*shape, prob.dof, st, code, rp, ci, C.byref(nnz))
    else:
        def call(rp, ci):
            return lib.nk_grid_pattern(*shape, prob.dof, st, code, rp, ci, C.byref(nnz))
    assert call(None, None) == 0, lib.nk_last_error()
    rp, ci = np.empty(prob.dof * int(np.prod(shape)) + 1, dtype=np.int32), np.empty(nnz.value, dtype=np.int32)
    assert call(C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data)) == 0
    return rp, ci


@pytest.mark.parametrize("name,shape", _CASES, ids=_IDS)
def test_library_pattern_is_the_restatements(name, shape):
    import nonlinearsolve_jl_amd as nls
    prob = R.PROBLEMS[name]
    rp, ci = _lib_pattern(prob, shape)
    ref_rp, ref_ci = GC.pattern(shape, prob.dof, prob.offsets(), prob.sides)
    assert np.array_equal(rp, ref_rp) and np.array_equal(ci, ref_ci)
    for r in (0, rp.size // 2, rp.size - 2):                                   # ascending, every column once
        assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)
    # the public spelling: the tuple of kinds, and the dict by axis
    rp2, ci2 = nls.grid_pattern(shape[0], shape[1], prob.dof, prob.stencil, prob.boundary, nz=shape[2] if prob.dim == 3 else None)
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci)
    by_axis = {a: (prob.boundary[2 * t], prob.boundary[2 * t + 1]) for t, a in enumerate("xyz"[:prob.dim])}
    rp3, ci3 = nls.grid_pattern(shape[0], shape[1], prob.dof, prob.stencil, by_axis, nz=shape[2] if prob.dim == 3 else None)
    assert np.array_equal(rp3, rp) and np.array_equal(ci3, ci)


def test_patterns_written_out_by_hand():
    """3 × 3 star, mirror-node on all sides (nodes 0 1 2 / 3 4 5 / 6 7 8): at a wall the two points of an axis land on one node.
    5 × 5 star2: the row of node (1, 0) with x mirror-face below and mirror-node above, y mirror-node below"""
    import nonlinearsolve_jl_amd as nls
    rp, ci = nls.grid_pattern(3, 3, boundary=(MN,) * 4)
    rows = [list(ci[rp[r]:rp[r + 1]]) for r in range(9)]
    assert rows == [[0, 1, 3], [0, 1, 2, 4], [1, 2, 5], [0, 3, 4, 6], [1, 3, 4, 5, 7], [2, 4, 5, 8], [3, 6, 7], [4, 6, 7, 8],
                    [5, 7, 8]]
    rp, ci = nls.grid_pattern(3, 3, boundary=(MF,) * 4)                        # mirror-face: the ghost is the node itself
    assert [list(ci[rp[r]:rp[r + 1]]) for r in (0, 4, 8)] == [[0, 1, 3], [1, 3, 4, 5, 7], [5, 7, 8]]
    rp, ci = nls.grid_pattern(5, 5, stencil="star2", boundary={"x": (MF, MN), "y": (MN, DI)})
    # node (1, 0) = 1: x offsets −2 −1 0 1 2 land on i = 0 (face: −1 ↦ 0), 0, 1, 2, 3; y offsets −2 −1 1 2 on j = 2, 1, 1, 2
    assert list(ci[rp[1]:rp[2]]) == [0, 1, 2, 3, 6, 11]
    # node (3, 4) = 23: x + 2 = 5 ↦ 3 (node: n−1+k ↦ n−1−k) is the centre; y + 1, y + 2 left through the Dirichlet side
    assert list(ci[rp[23]:rp[24]]) == [13, 18, 21, 22, 23, 24]
    # the channel of the docstring, by axis: missing axes are Dirichlet
    a = nls.grid_pattern(4, 3, boundary={"x": PE})
    b = nls.grid_pattern(4, 3, boundary=(PE, PE, DI, DI))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and list(a[1][:4]) == [0, 1, 3, 4]


# ------------------------------------------------------------------------------------------------ compilation
def _args(p, code=None):
    return (p.source.encode(), p.dim, p.dof, GC.STENCIL_ID[p.stencil], GC.sides_code(p.boundary) if code is None else code,
            len(p.params), p.nfields)


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    p = R.PROBLEMS[name]
    lib, nb, nb2 = L.lib(), C.c_int64(), C.c_int64()
    assert lib.nk_grid_fields_compile_check(*_args(p), C.byref(nb)) == 0, lib.nk_last_error()
    assert nb.value > 2000
    if not p.nfields:   # the entry point of the problem's own dimension
        fn = lib.nk_grid3_compile_check if p.dim == 3 else lib.nk_grid_compile_check
        a = _args(p)
        assert fn(a[0], a[2], a[3], a[4], a[5], C.byref(nb2)) == 0, lib.nk_last_error()
        assert nb2.value == nb.value
    assert nls.grid_compile_check(p.source, dof=p.dof, stencil=p.stencil, boundary=p.boundary, nparams=len(p.params),
                                  dim=p.dim, fields=p.nfields) == nb.value


def _code_object(fn, *args):
    nb = C.c_int64()
    assert fn(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert fn(*args, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("jac", [0, 1])
def test_a_packed_uniform_code_is_the_plain_code(jac):
    """NK_GRID_SIDES(all periodic) and NK_GRID_SIDES(all Dirichlet-0) are codes 1 and 0: the code objects byte for byte, through
    all three code-object entry points, and the pattern"""
    lib = L.lib()
    for kind, plain in ((PE, 1), (DI, 0)):
        p = G1.PROBLEMS["box_periodic"]
        a = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil])
        packed = GC.sides_code(GC.uniform(kind, 2))
        assert packed not in (0, 1)
        old = _code_object(lib.nk_grid_code_object, *a, plain, len(p.params), jac)
        assert old[:4] == b"\x7fELF"
        assert _code_object(lib.nk_grid_code_object, *a, packed, len(p.params), jac) == old
        assert _code_object(lib.nk_grid_fields_code_object, a[0], 2, *a[1:], packed, len(p.params), 0, jac) == old
        p3 = G3.PROBLEMS["brusselator3"]
        a3 = (p3.source.encode(), p3.dof, GC.STENCIL_ID[p3.stencil])
        old3 = _code_object(lib.nk_grid3_code_object, *a3, plain, len(p3.params), jac)
        assert _code_object(lib.nk_grid3_code_object, *a3, GC.sides_code(GC.uniform(kind, 3)), len(p3.params), jac) == old3
        pf = GF.PROBLEMS["react2"]
        af = (pf.source.encode(), 2, pf.dof, GC.STENCIL_ID[pf.stencil])
        assert (_code_object(lib.nk_grid_fields_code_object, *af, packed, len(pf.params), pf.nfields, jac) ==
                _code_object(lib.nk_grid_fields_code_object, *af, plain, len(pf.params), pf.nfields, jac))
    # and a mirror program is another program
    p = G1.PROBLEMS["bratu"]
    a = (p.source.encode(), p.dof, 0)
    assert (_code_object(lib.nk_grid_code_object, *a, GC.sides_code(GC.uniform(MN, 2)), 2, jac) !=
            _code_object(lib.nk_grid_code_object, *a, 0, 2, jac))
    import nonlinearsolve_jl_amd as nls
    for kind, plain in ((PE, "periodic"), (DI, "dirichlet")):
        x, y = nls.grid_pattern(7, 5, 2, "box", (kind,) * 4), nls.grid_pattern(7, 5, 2, "box", plain)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def _status(fn, *args):
    st = fn(*args)
    return st, L.lib().nk_last_error().decode(errors="replace")


def test_argument_errors_name_their_cause():
    import nonlinearsolve_jl_amd as nls
    lib, nb = L.lib(), C.c_int64()
    src = G1.BRATU_SRC.encode()
    # one side of an axis periodic
    st, msg = _status(lib.nk_grid_compile_check, src, 1, 0, GC.sides_code((PE, MN, DI, DI)), 2, C.byref(nb))
    assert st == -1 and "x axis" in msg and "x-lo is NK_GRID_PERIODIC" in msg and "x-hi is NK_GRID_MIRROR_NODE" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, 0, GC.sides_code((DI, DI, MF, MF, DI, PE)), None, None, C.byref(nb))
    assert st == -1 and "z axis" in msg and "z-hi is NK_GRID_PERIODIC" in msg
    # an unknown kind
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, 0, GC.sides_code((0, 0, 0, 7)), None, None, C.byref(nb))
    assert st == -1 and "y-hi = 7" in msg and "unknown kind" in msg
    st, msg = _status(lib.nk_grid_code_object, src, 1, 0, 2, 2, 0, None, 0, C.byref(nb))   # a bare kind is no code
    assert st == -1 and "boundary = 2" in msg and "NK_GRID_SIDES" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, 0, -1, None, None, C.byref(nb))
    assert st == -1 and "boundary = -1" in msg
    # a z kind in 2-D
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, 0, GC.sides_code((MN, MN, MN, MN, MN, 0)), None, None, C.byref(nb))
    assert st == -1 and "z-lo = 2" in msg and "2-D" in msg
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 2, 1, 0, GC.sides_code((0, 0, 0, 0, 0, 3)), 2, 0, C.byref(nb))
    assert st == -1 and "z-hi = 3" in msg
    # the side minimum is unchanged
    st, msg = _status(lib.nk_grid_pattern, 4, 5, 1, 16, GC.sides_code(GC.uniform(MN, 2)), None, None, C.byref(nb))
    assert st == -1 and "nx >= 5" in msg
    # the Python spellings
    with pytest.raises(ValueError, match="mirror"):
        nls.grid_pattern(5, 5, boundary="mirror")
    with pytest.raises(ValueError, match="4 sides"):
        nls.grid_pattern(5, 5, boundary=(MN, MN))
    with pytest.raises(ValueError, match="6 sides"):
        nls.grid_pattern(5, 5, boundary=(MN,) * 4, nz=5)
    with pytest.raises(ValueError, match="'neumann'"):
        nls.grid_pattern(5, 5, boundary={"x": "neumann"})
    with pytest.raises(ValueError, match="axes"):
        nls.grid_pattern(5, 5, boundary={"z": MN})
    with pytest.raises(nls.NKError, match="y axis"):
        nls.grid_pattern(5, 5, boundary={"y": (PE, DI)})
    assert L.grid_sides(2, 3, 1, 1) == GC.sides_code((MN, MF, PE, PE)) == (1 << 24) | 0x1132


# ------------------------------------------------------------------------------------------------ resources
def _kernel_notes(readelf, path):
    """kernel name → (private segment, vgprs, LDS bytes) from the code object's metadata notes"""
    notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", block)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        ls = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        if nm and ps and not nm.group(1).endswith(".kd"):
            out[nm.group(1)] = (int(ps.group(1)), int(vg.group(1)) if vg else -1, int(ls.group(1)) if ls else -1)
    return out


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, monkeypatch, name, direct):
    """all three kernels of every case, with both forms of the fill, are register programs — the merge is compares and selects
    on registers — and the staged fill's LDS piece is what it is without mirrors: 256·npts·dof doubles (rows only get shorter)"""
    monkeypatch.setenv("NK_GRID_FILL_DIRECT", str(direct))
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.access(readelf, os.X_OK):
        pytest.skip("llvm-readelf not installed")
    p = R.PROBLEMS[name]
    for jac, kernels in KERNELS[p.dim].items():
        co = _code_object(L.lib().nk_grid_fields_code_object, *_args(p), jac)
        assert co[:4] == b"\x7fELF"
        path = tmp_path / f"{name}_{jac}.co"
        path.write_bytes(co)
        notes = _kernel_notes(readelf, path)
        assert set(notes) == set(kernels), sorted(notes)
        for k in kernels:
            print(f"{name}: {k}: private segment {notes[k][0]}, VGPRs {notes[k][1]}, LDS {notes[k][2]}")
            assert notes[k][0] == 0, (k, notes)
        if jac == 1:
            assert notes[kernels[0]][2] == (0 if direct else 256 * len(p.offsets()) * p.dof * 8)


# ------------------------------------------------------------------------------------------------ conservation, on the CPU
def heat_fields(shape, level):
    """the fields of the conservation problem: the previous level, a positive coefficient, no source"""
    f = GC.seeded_fields(3, shape)
    return np.stack([level, f[1], np.zeros_like(level)])


def test_conservation_bound_separates_mirror_face_from_dirichlet():
    """vardiff as implicit Euler, F(u) = (u − a₀)/dt − Σ_faces ½(κ + κ_nb)(u_nb − u), 24 × 20, dt = 0.05, one exact step by a
    dense Newton on the restatement. With mirror-face walls ΣF telescopes to (Σu − Σa₀)/dt, so
    |Σu_new − Σa₀| <= dt·‖F(u_new)‖₁ + 8·nn·eps·Σ|u|; with Dirichlet-0 walls the same quantity is more than 1e6 times that
    bound: the device test that asserts the bound cannot pass by accident"""
    shape, dt = (24, 20), 0.05
    nn, params = 24 * 20, [1.0 / dt, 1.0]
    a0 = 1.0 + 0.5 * np.cos(0.3 * np.arange(nn))
    out = {}
    for tag, prob in (("mirror_face", R.PROBLEMS["vardiff_mirror_face"]), ("dirichlet", R.DIRICHLET_TWIN["vardiff_mirror_face"])):
        fields = heat_fields(shape, a0)
        u = GC.dense_newton(prob, shape, a0, fields, params=params)
        f = GC.evaluate(prob, shape, u, u, fields, params=params).f
        drift = abs(float(np.sum(u.astype(GC.LD)) - np.sum(a0.astype(GC.LD))))
        bound = dt * float(np.abs(f).sum()) + 8 * nn * GC.EPS * float(np.abs(u).sum())
        print(f"{tag}: |sum u - sum a0| {drift:.3e}, bound {bound:.3e}, |F|_1 {np.abs(f).sum():.3e}")
        out[tag] = (drift, bound)
    assert out["mirror_face"][0] <= out["mirror_face"][1]
    assert out["dirichlet"][0] >= 1e6 * out["dirichlet"][1]
