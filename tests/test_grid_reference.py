"""Compiled grid problems without a GPU: nk_grid_pattern against the NumPy restatement (tests/grid_core.py, tests/grid_reference.py), the restatement
against itself (analytic Jacobians against differences of its own residual), the three sources through hiprtc for gfx950, the
argument errors with their messages, and the generated kernels' resource notes (no private segment)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_core as GC
import grid_reference as R
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
SHAPES = [(3, 3), (3, 7), (37, 29), (300, 5)]
KERNELS = {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)}


def _lib_pattern(nx, ny, dof, stencil, boundary):
    import nonlinearsolve_jl_amd as nls
    return nls.grid_pattern(nx, ny, dof=dof, stencil=stencil, boundary=boundary)


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("boundary", ["dirichlet", "periodic"])
@pytest.mark.parametrize("stencil,dof", [("star", 1), ("star", 2), ("star", 4), ("box", 1), ("box", 2)])
def test_pattern_equals_the_restatement(nx, ny, stencil, dof, boundary):
    """(the box stops at dof 2: dof 4 with the box is an argument error, test_argument_errors_name_their_cause)"""
    rp, ci = _lib_pattern(nx, ny, dof, stencil, boundary)
    rp_ref, ci_ref = GC.stencil_pattern((nx, ny), dof, stencil, boundary)
    assert rp.dtype == np.int32 and ci.dtype == np.int32
    assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)
    # columns ascend strictly within every row
    inner = np.ones(ci.size, dtype=bool)
    inner[rp[:-1]] = False
    assert np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0)
    npts = len(GC.STENCILS[(2, stencil)])
    if boundary == "periodic":
        assert np.all(np.diff(rp) == npts * dof)
    else:
        interior = (min(nx, ny) >= 3) and np.diff(rp).max() == npts * dof
        assert interior and np.diff(rp).min() == (4 if stencil == "box" else 3) * dof   # a corner node


@pytest.mark.parametrize("stencil,dof", [("star", 1), ("star", 4), ("box", 2)])
def test_periodic_3x3_rows_have_distinct_columns(stencil, dof):
    rp, ci = _lib_pattern(3, 3, dof, stencil, "periodic")
    npts = len(GC.STENCILS[(2, stencil)])
    for r in range(rp.size - 1):
        row = ci[rp[r]:rp[r + 1]]
        assert row.size == npts * dof == np.unique(row).size
    if stencil == "box":   # every node of the 3 × 3 torus neighbours every node
        assert np.array_equal(ci[:9], np.arange(9))


@pytest.mark.parametrize("ns", [3, 4, 33])
def test_bratu_pattern_is_the_built_in_order(ns):
    rp, ci = _lib_pattern(ns, ns, 1, "star", "dirichlet")
    rp_b, ci_b = R.bratu_builtin_pattern(ns)
    assert np.array_equal(rp, rp_b) and np.array_equal(ci, ci_b)


def test_pattern_sizes_only():
    nnz = C.c_int64()
    assert L.lib().nk_grid_pattern(37, 29, 2, 1, 0, None, None, C.byref(nnz)) == 0
    assert nnz.value == GC.stencil_pattern((37, 29), 2, "box", "dirichlet")[1].size
    rp = np.zeros(2 * 37 * 29 + 1, dtype=np.int32)
    assert L.lib().nk_grid_pattern(37, 29, 2, 1, 0, C.c_void_p(rp.ctypes.data), None, C.byref(nnz)) == 0
    assert rp[-1] == nnz.value


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_restatement_jacobians_against_its_own_residual(name):
    """the analytic formulas the device is held against: J·v and the CSR values against central differences of the
    restatement's residual in long double, Jᵀv against the values"""
    prob, shape = R.PROBLEMS[name], (7, 5)
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
    for k in ("f", "jv", "vals"):
        assert np.all(getattr(ref, k + "_gap") <= getattr(ref, k + "_bound"))


def test_restatement_matches_the_built_in_formulas():
    """Bratu2D(n, λ): c_lap = 1 exactly and c_exp = h²λ, as nk_problem_set_params computes them"""
    c_lap, c_exp = R.bratu_params(33, 6.0)
    h = 1.0 / 34.0
    assert c_lap == 1.0 and c_exp == (h * h) * 6.0
    assert R.brusselator_params(24) == [3.4, 1.0, 10.0 / ((1.0 / 23) * (1.0 / 23))]


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    p = R.PROBLEMS[name]
    nbytes = nls.grid_compile_check(p.source, dof=p.dof, stencil=p.stencil, boundary=p.boundary, nparams=len(p.params))
    assert nbytes > 2000


def _status(fn, *args):
    st = fn(*args)
    return st, L.lib().nk_last_error().decode(errors="replace")


def test_argument_errors_name_their_cause():
    lib, nb, src = L.lib(), C.c_int64(), R.BRATU_SRC.encode()
    st, msg = _status(lib.nk_grid_compile_check, R.SYNTAX_ERROR_SRC.encode(), 1, 0, 0, 2, C.byref(nb))
    assert st == -1 and "no_such_symbol" in msg and "nk_point" in msg and "nk_nbhd" in msg   # the log and the contract
    st, msg = _status(lib.nk_grid_compile_check, src, 5, 0, 0, 2, C.byref(nb))
    assert st == -1 and "dof = 5" in msg
    st, msg = _status(lib.nk_grid_compile_check, src, 3, 1, 0, 2, C.byref(nb))
    assert st == -1 and "box" in msg and "dof = 3" in msg
    st, msg = _status(lib.nk_grid_compile_check, src, 1, 0, 0, 33, C.byref(nb))
    assert st == -1 and "nparams = 33" in msg
    nnz = C.c_int64()
    st, msg = _status(lib.nk_grid_pattern, 2, 5, 1, 0, 0, None, None, C.byref(nnz))
    assert st == -1 and "2 x 5" in msg and "nx >= 3" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 5, 0, 0, None, None, C.byref(nnz))
    assert st == -1 and "dof = 5" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 3, 1, 0, None, None, C.byref(nnz))
    assert st == -1 and "box" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, 2, 0, None, None, C.byref(nnz))
    assert st == -1 and "stencil" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, 0, 7, None, None, C.byref(nnz))
    assert st == -1 and "boundary" in msg
    import nonlinearsolve_jl_amd as nls
    with pytest.raises(nls.NKError, match="dof = 5"):
        nls.grid_pattern(5, 5, dof=5)
    with pytest.raises(ValueError, match="stencil"):
        nls.grid_pattern(5, 5, stencil="hexagon")


def _code_object(p, jac):
    nb = C.c_int64()
    args = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params), jac)
    assert L.lib().nk_grid_code_object(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_grid_code_object(*args, buf, nb.value, C.byref(nb)) == 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_grid_code_object(*args, small, 16, C.byref(nb)) != 0
    return buf.raw[:nb.value]


def _kernel_notes(readelf, path):
    """kernel name → {private segment, vgprs} from the code object's metadata notes"""
    notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", block)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        if nm and ps and not nm.group(1).endswith(".kd"):
            out[nm.group(1)] = (int(ps.group(1)), int(vg.group(1)) if vg else -1)
    return out


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, name):
    """all three kernels of every source are register programs: the neighbourhood, the duals with their folded unit seeds and
    the slot ranks never reach scratch memory"""
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
