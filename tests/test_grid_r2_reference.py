"""Compiled grid problems with a radius-2 stencil without a GPU: nk_grid_pattern / nk_grid3_pattern against the NumPy
restatement (tests/grid_core.py, tests/grid_r2_reference.py), the restatement against itself (analytic Jacobians against differences of its own
residual), the sources through hiprtc for gfx950, the argument errors with their messages, the stencil codes of the header,
Python and Julia, and the generated kernels' resource notes (no private segment, no spilled register)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_core as GC
import grid_r2_reference as R
from nonlinearsolve_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {2: [(5, 5), (6, 5), (37, 29)], 3: [(5, 5, 5), (7, 6, 5)]}
KERNELS = {2: {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)},
           3: {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}}
# in-domain stencil points of a Dirichlet corner node: the centre and, per direction, the two points on the inner side (the
# diamond adds the one diagonal that points inward) — 1 + 2·2, 1 + 2·2 + 1, 1 + 2·3
CORNER_POINTS = {(2, "star2"): 5, (2, "diamond2"): 6, (3, "star2"): 7}


LLVM = "/opt/rocm/llvm/bin"


def _status(fn, *args):
    st = fn(*args)
    return st, L.lib().nk_last_error().decode(errors="replace")


def _kernel_notes(readelf, path):
    """kernel name → private segment, VGPRs, AGPRs, LDS bytes and spilled VGPRs from the code object's metadata notes"""
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


def _lib_pattern(shape, dof, stencil, boundary):
    import nonlinearsolve_jl_amd as nls
    return nls.grid_pattern(shape[0], shape[1], dof=dof, stencil=stencil, boundary=boundary,
                            nz=shape[2] if len(shape) == 3 else None)


@pytest.mark.parametrize("boundary", ["dirichlet", "periodic"])
@pytest.mark.parametrize("dim,stencil,dof", R.PERMITTED)
def test_pattern_equals_the_restatement(dim, stencil, dof, boundary):
    npts = len(GC.STENCILS[(dim, stencil)])
    assert npts == {(2, "star2"): 9, (2, "diamond2"): 13, (3, "star2"): 13}[(dim, stencil)]
    for shape in SHAPES[dim]:
        rp, ci = _lib_pattern(shape, dof, stencil, boundary)
        rp_ref, ci_ref = GC.stencil_pattern(shape, dof, stencil, boundary)
        assert rp.dtype == np.int32 and ci.dtype == np.int32
        assert np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref), shape
        # columns ascend strictly within every row
        inner = np.ones(ci.size, dtype=bool)
        inner[rp[:-1]] = False
        assert np.all(np.diff(ci.astype(np.int64))[inner[1:]] > 0)
        if boundary == "periodic":
            assert np.all(np.diff(rp) == npts * dof)
        else:   # every shape has an interior node (two layers from every side) and a corner node
            assert np.diff(rp).max() == npts * dof and np.diff(rp).min() == CORNER_POINTS[(dim, stencil)] * dof
            assert rp[1] - rp[0] == CORNER_POINTS[(dim, stencil)] * dof            # node 0 is a corner
            centre = sum(w * 2 for w in np.cumprod((1,) + shape[:-1]))               # node (2, 2[, 2]) is interior
            assert rp[centre + 1] - rp[centre] == npts * dof


@pytest.mark.parametrize("dim,stencil,dof", R.PERMITTED)
def test_periodic_rows_of_the_smallest_torus_have_distinct_columns(dim, stencil, dof):
    rp, ci = _lib_pattern((5,) * dim, dof, stencil, "periodic")
    npts = len(GC.STENCILS[(dim, stencil)])
    for r in range(rp.size - 1):
        row = ci[rp[r]:rp[r + 1]]
        assert row.size == npts * dof == np.unique(row).size


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_restatement_jacobians_against_its_own_residual(name):
    """the analytic formulas the device is held against: J·v and the CSR values against central differences of the
    restatement's residual in long double, Jᵀv against the values"""
    prob = R.PROBLEMS[name]
    shape = (6, 5) if prob.dim == 2 else (6, 5, 5)
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


@pytest.mark.parametrize("name", ["upwind2_dirichlet", "upwind2_periodic", "upwind3_dirichlet", "upwind3_periodic"])
def test_upwind_tells_directions_signs_and_distances_apart(name):
    """what the distinct weights are for: swapping +2 with −2, ±1 with ±2, i with j (j with k) changes the restatement's
    residual far beyond its bound. Parameter t of a component is the weight of EIGHT[t] / TWELVE[t]."""
    prob = R.PROBLEMS[name]
    shape = (6, 5) if prob.dim == 2 else (6, 5, 5)
    m = 8 if prob.dim == 2 else 12
    ref = GC.reference(prob, shape)
    p = list(prob.params)
    swaps = [(2, 3), (0, 2), (0, 4), (1, 3), (6, 7)] + ([(4, 8), (10, 11)] if prob.dim == 3 else [])
    for c in (0, 1):
        for a, b in swaps:
            q = list(p)
            q[c * m + a], q[c * m + b] = p[c * m + b], p[c * m + a]
            f = GC.evaluate(prob, shape, ref.u, ref.v, params=q).f
            assert np.max(np.abs(f - ref.f)) > 1e10 * ref.f_bound.max(), (c, a, b)


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    p = R.PROBLEMS[name]
    nbytes = nls.grid_compile_check(p.source, dof=p.dof, stencil=p.stencil, boundary=p.boundary, nparams=len(p.params), dim=p.dim)
    assert nbytes > 2000


def test_outside_sources_compile():
    """(reading an offset outside the stencil's shape is a run-time NaN, not a compile error: tests/test_gpu_grid_r2_problem.py)"""
    import nonlinearsolve_jl_amd as nls
    assert nls.grid_compile_check(R.OUTSIDE_SRC["star2"], stencil="star2") > 2000
    assert nls.grid_compile_check(R.OUTSIDE_SRC["diamond2"], stencil="diamond2") > 2000
    assert nls.grid_compile_check(R.OUTSIDE_SRC["star2_3"], stencil="star2", dim=3) > 2000
    assert nls.grid_compile_check(R.OUTSIDE_SRC["star2"], stencil="diamond2") > 2000   # (1, 1) lies inside the diamond


def test_argument_errors_name_their_cause():
    import nonlinearsolve_jl_amd as nls
    lib, nb, nnz = L.lib(), C.c_int64(), C.c_int64()
    src, src3 = R.LAP4_SRC.encode(), R.LAP4_3_SRC.encode()
    st, msg = _status(lib.nk_grid_compile_check, R.SYNTAX_ERROR_SRC.encode(), 1, 16, 0, 2, C.byref(nb))
    assert st == -1 and "no_such_symbol" in msg and "nk_point" in msg and "nk_nbhd" in msg
    # a side of 4 with a radius-2 stencil, every direction, both dimensions, both stencils
    for shape in ((4, 5), (5, 4)):
        for code in (16, 17):
            st, msg = _status(lib.nk_grid_pattern, *shape, 1, code, 1, None, None, C.byref(nnz))
            assert st == -1 and "%d x %d" % shape in msg and "nx >= 5" in msg and "ny >= 5" in msg and "radius-2" in msg
    for shape in ((4, 5, 5), (5, 4, 5), (5, 5, 4), (5, 5, 2)):
        st, msg = _status(lib.nk_grid3_pattern, *shape, 1, 16, 0, None, None, C.byref(nnz))
        assert st == -1 and "%d x %d x %d" % shape in msg and "nx >= 5" in msg and "nz >= 5" in msg
    st, msg = _status(lib.nk_grid_pattern, 4, 4, 1, 0, 1, None, None, C.byref(nnz))        # radius 1 keeps its minimum of 3
    assert st == 0
    st, msg = _status(lib.nk_grid_pattern, 2, 5, 1, 0, 1, None, None, C.byref(nnz))
    assert st == -1 and "nx >= 3" in msg and "radius-1" in msg
    with pytest.raises(nls.NKError, match="nx >= 5"):
        nls.grid_pattern(4, 7, stencil="star2")
    with pytest.raises(nls.NKError, match="nz >= 5"):
        nls.grid_pattern(7, 7, stencil="star2", nz=4)
    # dof limits
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 3, 16, 0, None, None, C.byref(nnz))
    assert st == -1 and "dof = 3" in msg and "star2" in msg and "dof <= 2" in msg
    st, msg = _status(lib.nk_grid_compile_check, src, 3, 16, 0, 2, C.byref(nb))
    assert st == -1 and "dof = 3" in msg and "star2" in msg
    st, msg = _status(lib.nk_grid_pattern, 5, 5, 2, 17, 0, None, None, C.byref(nnz))
    assert st == -1 and "dof = 2" in msg and "diamond2" in msg
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 3, 16, 0, None, None, C.byref(nnz))
    assert st == -1 and "dof = 3" in msg and "star2" in msg and "28 partials" in msg
    assert lib.nk_grid3_pattern(5, 5, 5, 2, 16, 0, None, None, C.byref(nnz)) == 0
    # the diamond is not offered in 3-D
    st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, 17, 0, None, None, C.byref(nnz))
    assert st == -1 and "NK_GRID_DIAMOND2" in msg and "stencil" in msg
    st, msg = _status(lib.nk_grid3_compile_check, src3, 1, 17, 0, 2, C.byref(nb))
    assert st == -1 and "NK_GRID_DIAMOND2" in msg
    with pytest.raises(nls.NKError, match="NK_GRID_DIAMOND2"):
        nls.grid_pattern(5, 5, stencil="diamond2", nz=5)
    # codes 2 and 18 are no stencils
    for code in (2, 18, 15, 32):
        st, msg = _status(lib.nk_grid_pattern, 5, 5, 1, code, 0, None, None, C.byref(nnz))
        assert st == -1 and "stencil = %d" % code in msg
        st, msg = _status(lib.nk_grid3_pattern, 5, 5, 5, 1, code, 0, None, None, C.byref(nnz))
        assert st == -1 and "stencil = %d" % code in msg
        st, msg = _status(lib.nk_grid_compile_check, src, 1, code, 0, 2, C.byref(nb))
        assert st == -1 and "stencil" in msg
    # 32-bit pattern indices with the new point counts: nn·dof·npts·dof <= INT32_MAX. Each size would pass with the point count
    # of the radius-1 stencil of the same name (sizes only: nothing is allocated, and the refusal comes before any loop)
    st, msg = _status(lib.nk_grid_pattern, 15500, 15500, 1, 16, 0, None, None, C.byref(nnz))     # 2.40e8·9 > 2³¹ > 2.40e8·5
    assert st == -1 and "32-bit" in msg and "15500 x 15500" in msg
    st, msg = _status(lib.nk_grid_pattern, 13000, 13000, 1, 17, 0, None, None, C.byref(nnz))     # 1.69e8·13 > 2³¹ > 1.69e8·9
    assert st == -1 and "32-bit" in msg and "13000 x 13000" in msg
    st, msg = _status(lib.nk_grid_pattern, 7800, 7800, 2, 16, 0, None, None, C.byref(nnz))       # 6.08e7·2·9·2 > 2³¹
    assert st == -1 and "32-bit" in msg and "dof = 2" in msg
    st, msg = _status(lib.nk_grid3_pattern, 550, 550, 550, 1, 16, 0, None, None, C.byref(nnz))   # 1.66e8·13 > 2³¹ > 1.66e8·7
    assert st == -1 and "32-bit" in msg and "550 x 550 x 550" in msg
    with pytest.raises(ValueError, match="stencil"):
        nls.grid_pattern(5, 5, stencil="hexagon")
    with pytest.raises(ValueError, match="stencil"):
        nls.grid_compile_check(R.LAP4_SRC, stencil="hexagon")


def test_stencil_codes_agree():
    """the header's enum, _lib.GRID_STENCILS, the restatement's STENCIL_ID and Julia's GRID_STENCILS"""
    header = open(os.path.join(ROOT, "include", "mi355x_nk.h"), encoding="utf-8").read()
    enum = re.search(r"enum \{([^}]*NK_GRID_STAR2[^}]*)\}", header).group(1)
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"NK_GRID_(\w+)\s*=\s*(\d+)", enum)}
    assert codes == {"star": 0, "box": 1, "star2": 16, "diamond2": 17}
    assert L.GRID_STENCILS == codes
    assert GC.STENCIL_ID == codes
    jl = open(os.path.join(ROOT, "julia", "src", "MI355XNewtonKrylov.jl"), encoding="utf-8").read()
    line = re.search(r"const GRID_STENCILS = Dict\(([^)]*)\)", jl).group(1)
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r":(\w+)\s*=>\s*(\d+)", line)} == codes
    for name, code in codes.items():
        assert (code & 16 != 0) == name.endswith("2")   # bit 16: radius 2


def _code_object(p, jac):
    fn = L.lib().nk_grid3_code_object if p.dim == 3 else L.lib().nk_grid_code_object
    nb = C.c_int64()
    args = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params), jac)
    assert fn(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert fn(*args, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, monkeypatch, name, direct):
    """all three kernels of every radius-2 source are register programs — the 13-point neighbourhoods, the 26-partial duals with
    their folded unit seeds and the 169 slot compares never reach scratch memory, and no VGPR is spilled — in both forms of the
    fill; the staged fill's LDS is at most 256·26 doubles"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.access(readelf, os.X_OK):
        pytest.skip("llvm-readelf not installed")
    monkeypatch.setenv("NK_GRID_FILL_DIRECT", str(direct))
    p = R.PROBLEMS[name]
    npts = len(p.offsets())
    for jac, kernels in KERNELS[p.dim].items():
        co = _code_object(p, jac)
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
            assert n["lds"] <= 256 * 26 * 8
            if jac == 1:
                assert n["lds"] == (0 if direct else 256 * npts * p.dof * 8)
