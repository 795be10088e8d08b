"""Compiled grid problems in three dimensions without a GPU: nk_grid3_pattern against the NumPy restatement
(tests/grid_core.py, tests/grid3_reference.py), the restatement against itself (analytic Jacobians against differences of its own residual), the
sources through hiprtc for gfx950, the argument errors with their messages, and the generated kernels' resource notes (no
private segment). The 2-D entry points are still what a call without `nz` reaches."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid3_reference as R
import grid_core as GC
import grid_reference as R2
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
SHAPES = [(3, 3, 3), (3, 4, 5), (7, 6, 5), (37, 5, 3), (4, 3, 40)]
KERNELS = {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}


def _lib_pattern(nx, ny, nz, dof, stencil, boundary):
    import nonlinearsolve_jl_amd as nls
    return nls.grid_pattern(nx, ny, dof=dof, stencil=stencil, boundary=boundary, nz=nz)


@pytest.mark.parametrize("nx,ny,nz", SHAPES)
@pytest.mark.parametrize("boundary", ["dirichlet", "periodic"])
@pytest.mark.parametrize("stencil,dof", R.PERMITTED)
def test_pattern_equals_the_restatement(nx, ny, nz, stencil, dof, boundary):
    """(the box stops at dof 1: dof 2 with the box is an argument error, test_argument_errors_name_their_cause)"""
    rp, ci = _lib_pattern(nx, ny, nz, dof, stencil, boundary)
    rp_ref, ci_ref = GC.stencil_pattern((nx, ny, nz), dof, stencil, boundary)
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    # columns ascend strictly within every row
    inner = np.ones(ci.size, dtype=bool)
    inner[rp[:-1]] = False
    assert np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0)
    npts = len(GC.STENCILS[(3, stencil)])
    if boundary == "periodic":
        assert np.all(np.diff(rp) == npts * dof)
    else:   # every shape has an interior node and a corner node
        assert np.diff(rp).max() == npts * dof and np.diff(rp).min() == (8 if stencil == "box" else 4) * dof


@pytest.mark.parametrize("stencil,dof", [("star", 1), ("star", 4), ("box", 1)])
def test_periodic_3x3x3_rows_have_distinct_columns(stencil, dof):
    rp, ci = _lib_pattern(3, 3, 3, dof, stencil, "periodic")
    npts = len(GC.STENCILS[(3, stencil)])
    for r in range(rp.size - 1):
        row = ci[rp[r]:rp[r + 1]]
        assert row.size == npts * dof == np.unique(row).size
        if stencil == "box":   # every node of the 3 × 3 × 3 torus neighbours every node
            assert np.array_equal(row, np.arange(27))


def test_pattern_sizes_only():
    nnz = C.c_int64()
    assert L.lib().nk_grid3_pattern(7, 6, 5, 1, 1, 0, None, None, C.byref(nnz)) == 0
    assert nnz.value == GC.stencil_pattern((7, 6, 5), 1, "box", "dirichlet")[1].size
    rp = np.zeros(2 * 7 * 6 * 5 + 1, dtype=np.int32)
    assert L.lib().nk_grid3_pattern(7, 6, 5, 2, 0, 1, C.c_void_p(rp.ctypes.data), None, C.byref(nnz)) == 0
    assert rp[-1] == nnz.value == 2 * 7 * 6 * 5 * 14
    assert L.lib().nk_grid3_pattern(7, 6, 5, 2, 0, 1, C.c_void_p(rp.ctypes.data), None, None) == 0


def test_two_dimensional_calls_are_unchanged():
    """without nz the 2-D entry points answer: the 5-point pattern of a 5 × 4 grid, and the 2-D contract in the messages"""
    import nonlinearsolve_jl_amd as nls
    rp, ci = nls.grid_pattern(5, 4)
    rp2, ci2 = GC.stencil_pattern((5, 4))
    assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2) and rp.size == 21
    assert nls.grid_compile_check(R2.BRATU_SRC, nparams=2) == nls.grid_compile_check(R2.BRATU_SRC, nparams=2, dim=2) > 2000
    with pytest.raises(nls.NKError, match="nk_nbhd<T>"):          # a 3-D source is no 2-D source
        nls.grid_compile_check(R.BRATU3_SRC, nparams=2)
    with pytest.raises(nls.NKError, match="nk_nbhd3<T>"):         # … and the other way round
        nls.grid_compile_check(R2.BRATU_SRC, nparams=2, dim=3)
    with pytest.raises(ValueError, match="dim"):
        nls.grid_compile_check(R2.BRATU_SRC, nparams=2, dim=4)
    with pytest.raises(nls.NKError, match="9-point box"):          # the 2-D box keeps its dof <= 2
        nls.grid_pattern(5, 4, dof=3, stencil="box")
    assert nls.grid_pattern(5, 4, dof=2, stencil="box")[0].size == 41


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_restatement_jacobians_against_its_own_residual(name):
    """the analytic formulas the device is held against: J·v and the CSR values against central differences of the
    restatement's residual in long double, Jᵀv against the values"""
    prob, shape = R.PROBLEMS[name], (5, 4, 3)
    ref = GC.reference(prob, shape)
    h = GC.LD(2.0) ** -20
    up = GC.evaluate(prob, shape, ref.u.astype(GC.LD) + h * ref.v.astype(GC.LD), ref.v, T=GC.LD).f
    um = GC.evaluate(prob, shape, ref.u.astype(GC.LD) - h * ref.v.astype(GC.LD), ref.v, T=GC.LD).f
    fd = ((up - um) / (2 * h)).astype(np.float64)
    assert np.max(np.abs(fd - ref.jv)) < 1e-8 * max(1.0, np.max(np.abs(ref.jv)))   # O(h²) truncation
    assert np.all(np.abs(ref.spmv - ref.jv) <= ref.spmv_bound + ref.jv_bound)
    rp, ci = GC.pattern(shape, prob.dof, prob.offsets(), prob.sides)
    dense = np.zeros((rp.size - 1, rp.size - 1))
    dense[np.repeat(np.arange(rp.size - 1), np.diff(rp)), ci] = ref.vals
    assert np.allclose(dense.T @ ref.v, ref.jtv, rtol=0, atol=1e-12 * np.abs(ref.vals).max())
    assert np.array_equal(dense, GC.dense_jacobian(prob, shape, ref.u)[0])
    for k in ("f", "jv", "vals"):
        assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))


def test_brusselator3_tells_directions_and_signs_apart():
    """what the upwinded weights are for: swapping +k with −k, or j with k, changes the restatement's residual far beyond its bound"""
    shape = (4, 4, 4)
    prob = R.PROBLEMS["brusselator3"]
    ref = GC.reference(prob, shape)
    p = list(prob.params)
    for a, b in ((6, 7), (4, 6), (2, 3)):
        q = list(p)
        q[a], q[b] = p[b], p[a]
        f = GC.evaluate(prob, shape, ref.u, ref.v, params=q).f
        assert np.max(np.abs(f - ref.f)) > 1e10 * ref.f_bound.max()


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    p = R.PROBLEMS[name]
    nbytes = nls.grid_compile_check(p.source, dof=p.dof, stencil=p.stencil, boundary=p.boundary, nparams=len(p.params), dim=3)
    assert nbytes > 2000


def test_edge_source_compiles():
    """(reading an edge offset of the star is a run-time NaN, not a compile error: tests/test_gpu_grid3_problem.py)"""
    import nonlinearsolve_jl_amd as nls
    assert nls.grid_compile_check(R.EDGE_SRC, dim=3) > 2000


def _status(fn, *args):
    st = fn(*args)
    return st, L.lib().nk_last_error().decode(errors="replace")


def test_argument_errors_name_their_cause():
    lib, nb, src = L.lib(), C.c_int64(), R.BRATU3_SRC.encode()
    st, msg = _status(lib.nk_grid3_compile_check, R.SYNTAX_ERROR_SRC.encode(), 1, 0, 0, 2, C.byref(nb))
    assert st == -1 and "no_such_symbol" in msg and "nk_point" in msg and "nk_nbhd3" in msg and "nk_site3" in msg
    st, msg = _status(lib.nk_grid3_compile_check, src, 5, 0, 0, 2, C.byref(nb))
    assert st == -1 and "dof = 5" in msg
    st, msg = _status(lib.nk_grid3_compile_check, src, 2, 1, 0, 2, C.byref(nb))
    assert st == -1 and "27-point box" in msg and "dof = 2" in msg
    st, msg = _status(lib.nk_grid3_compile_check, src, 1, 0, 0, 33, C.byref(nb))
    assert st == -1 and "nparams = 33" in msg
    st, msg = _status(lib.nk_grid3_compile_check, None, 1, 0, 0, 2, C.byref(nb))
    assert st == -1 and "NULL" in msg
    st, msg = _status(lib.nk_grid3_code_object, src, 1, 0, 0, 2, 0, None, 0, None)
    assert st == -1 and "NULL" in msg
    nnz = C.c_int64()
    for shape in ((2, 5, 5), (5, 2, 5), (5, 5, 2)):
        st, msg = _status(lib.nk_grid3_pattern, *shape, 1, 0, 0, None, None, C.byref(nnz))
        assert st == -1 and "%d x %d x %d" % shape in msg and "nz >= 3" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, 0, 0, None, None, None)
    assert st == -1 and "NULL" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 5, 0, 0, None, None, C.byref(nnz))
    assert st == -1 and "dof = 5" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 2, 1, 0, None, None, C.byref(nnz))
    assert st == -1 and "box" in msg and "dof = 2" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, 2, 0, None, None, C.byref(nnz))
    assert st == -1 and "stencil" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, 0, 7, None, None, C.byref(nnz))
    assert st == -1 and "boundary" in msg
    # 32-bit pattern indices: nn·dof·npts·dof <= INT32_MAX (sizes only: nothing is allocated)
    st, msg = _status(lib.nk_grid3_pattern, 1024, 1024, 1024, 1, 0, 0, None, None, C.byref(nnz))
    assert st == -1 and "32-bit" in msg and "1024 x 1024 x 1024" in msg
    st, msg = _status(lib.nk_grid3_pattern, 100000, 100000, 100000, 1, 0, 0, None, None, C.byref(nnz))
    assert st == -1 and "32-bit" in msg
    st, msg = _status(lib.nk_grid3_pattern, 400, 400, 400, 4, 0, 0, None, None, C.byref(nnz))   # 64e6·4·7·4 > 2³¹
    assert st == -1 and "32-bit" in msg and "dof = 4" in msg
    import nonlinearsolve_jl_amd as nls
    with pytest.raises(nls.NKError, match="dof = 5"):
        nls.grid_pattern(5, 5, dof=5, nz=5)
    with pytest.raises(nls.NKError, match="nz >= 3"):
        nls.grid_pattern(5, 5, nz=2)
    with pytest.raises(ValueError, match="stencil"):
        nls.grid_pattern(5, 5, stencil="hexagon", nz=5)


def _code_object(p, jac):
    nb = C.c_int64()
    args = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params), jac)
    assert L.lib().nk_grid3_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_grid3_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_grid3_code_object(*args, small, 16, C.byref(nb)) != 0
    return buf.raw[:nb.value]


def _kernel_notes(readelf, path):
    """kernel name → (private segment, vgprs, LDS bytes) from the code object's metadata notes"""
    notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", block)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        ag = re.search(r"\.agpr_count:\s+(\d+)", block)
        ld = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        if nm and ps and not nm.group(1).endswith(".kd"):
            out[nm.group(1)] = dict(private=int(ps.group(1)), vgprs=int(vg.group(1)) if vg else -1,
                                    agprs=int(ag.group(1)) if ag else 0, lds=int(ld.group(1)) if ld else -1,
                                    spills=int(sp.group(1)) if sp else 0)
    return out


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, monkeypatch, name, direct):
    """all three kernels of every source are register programs — the 27-point neighbourhood, the 28-partial duals with their
    folded unit seeds and the slot ranks never reach scratch memory — in both forms of the fill; the staged fill's LDS is at
    most 256·28 doubles"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.access(readelf, os.X_OK):
        pytest.skip("llvm-readelf not installed")
    monkeypatch.setenv("NK_GRID_FILL_DIRECT", str(direct))
    for jac, kernels in KERNELS.items():
        co = _code_object(R.PROBLEMS[name], jac)
        assert co[:4] == b"\x7fELF"
        path = tmp_path / f"{name}_{jac}.co"
        path.write_bytes(co)
        notes = _kernel_notes(readelf, path)
        assert set(notes) == set(kernels), sorted(notes)
        for k in kernels:
            n = notes[k]
            print(f"{name}: {k} (direct = {direct}): private segment {n['private']}, VGPRs {n['vgprs']}, AGPRs {n['agprs']}, "
                  f"spilled VGPRs {n['spills']}, LDS {n['lds']} bytes")
            assert n["private"] == 0 and n["spills"] == 0, (k, notes)
            assert n["lds"] <= 256 * 28 * 8
