"""Compiled grid problems with fields, without a GPU: the restatement (tests/grid_core.py, tests/gridf_reference.py) against itself (analytic
Jacobians against differences of its own long-double residual; its boundary rule for fields on a 5 × 5 example written out by
hand), every source through nk_grid_fields_compile_check for gfx950, the generated kernels' resource notes (no private segment;
VGPR and global-load counts printed), the argument errors with their messages, and nfields = 0 through the new entry point
against nk_grid_code_object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid3_reference as G3
import grid_core as GC
import grid_reference as G1
import gridf_reference as R
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
KERNELS = {2: {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)},
           3: {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}}


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_restatement_jacobians_against_its_own_residual(name):
    """the analytic formulas the device is held against: J·v and the CSR values against central differences of the
    restatement's residual in long double, Jᵀv against the values; 6 × 5 and 5 × 5 × 5"""
    prob = R.PROBLEMS[name]
    shape = (5, 5, 5) if prob.dim == 3 else (6, 5)
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
    # the fields matter: other data, another residual and another Jacobian
    other = GC.reference(prob, shape, shift=1.0)
    assert np.max(np.abs(other.f - ref.f)) > 1e-3 and np.max(np.abs(other.vals - ref.vals)) > 1e-3


def test_field_boundary_rule_on_a_5x5_example():
    """field value 10·j + i at node (i, j). Dirichlet: a read outside the grid returns the node's own value — at i = nx − 2 an
    offset of +2 gives the centre, not the wall; periodic: the index wraps."""
    F = np.array([[10.0 * j + i for i in range(5)] for j in range(5)])[None]
    D, P = GC.Fields(F, "dirichlet"), GC.Fields(F, "periodic")
    assert np.array_equal(D(0, 0), F[0])
    assert np.array_equal(D(1, 0), [[1, 2, 3, 4, 4], [11, 12, 13, 14, 14], [21, 22, 23, 24, 24], [31, 32, 33, 34, 34],
                                    [41, 42, 43, 44, 44]])
    assert np.array_equal(D(2, 0), [[2, 3, 4, 3, 4], [12, 13, 14, 13, 14], [22, 23, 24, 23, 24], [32, 33, 34, 33, 34],
                                    [42, 43, 44, 43, 44]])
    assert np.array_equal(D(-2, 0)[2], [20, 21, 20, 21, 22])
    assert np.array_equal(D(0, -1), [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [10, 11, 12, 13, 14], [20, 21, 22, 23, 24],
                                     [30, 31, 32, 33, 34]])
    assert np.array_equal(D(1, 1), [[11, 12, 13, 14, 4], [21, 22, 23, 24, 14], [31, 32, 33, 34, 24], [41, 42, 43, 44, 34],
                                    [40, 41, 42, 43, 44]])   # a corner read outside in either direction: the node itself
    assert np.array_equal(P(1, 0)[0], [1, 2, 3, 4, 0]) and np.array_equal(P(2, 0)[3], [32, 33, 34, 30, 31])
    assert np.array_equal(P(0, -1)[0], [40, 41, 42, 43, 44]) and np.array_equal(P(-1, 1)[4], [4, 0, 1, 2, 3])
    # u's rule beside it: 0 outside a Dirichlet boundary
    assert np.array_equal(GC.Grid(F, "dirichlet")(1, 0)[0], [1, 2, 3, 4, 0])
    # three dimensions: the clamp per node, not per direction
    F3 = np.arange(27, dtype=np.float64).reshape(1, 3, 3, 3)
    D3 = GC.Fields(F3, "dirichlet")
    assert D3(0, 0, 1)[2, 1, 1] == F3[0, 2, 1, 1] and D3(0, 0, 1)[1, 1, 1] == F3[0, 2, 1, 1]
    assert D3(0, 0, -1)[0, 2, 0] == F3[0, 0, 2, 0] and D3(-1, 0, 0)[1, 1, 0] == F3[0, 1, 1, 0]


def test_seeded_fields_are_positive_and_distinct():
    A = GC.seeded_fields(4, (37, 29))
    assert A.shape == (4, 1073) and A.min() > 0.6 and np.unique(A).size == A.size


# ------------------------------------------------------------------------------------------------ compilation
def _args(p):
    return (p.source.encode(), p.dim, p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params), p.nfields)


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_sources_compile_for_gfx950(name):
    import nonlinearsolve_jl_amd as nls
    p = R.PROBLEMS[name]
    nb = C.c_int64()
    assert L.lib().nk_grid_fields_compile_check(*_args(p), C.byref(nb)) == 0, L.lib().nk_last_error()
    assert nb.value > 2000
    assert nls.grid_compile_check(p.source, dof=p.dof, stencil=p.stencil, boundary=p.boundary, nparams=len(p.params),
                                  dim=p.dim, fields=p.nfields) == nb.value


def _status(fn, *args):
    st = fn(*args)
    return st, L.lib().nk_last_error().decode(errors="replace")


def test_argument_errors_name_their_cause():
    lib, nb = L.lib(), C.c_int64()
    src = R.PROBLEMS["bratu_f"].source.encode()
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 2, 1, 0, 0, 2, 5, C.byref(nb))
    assert st == -1 and "nfields = 5" in msg
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 2, 1, 0, 0, 2, -1, C.byref(nb))
    assert st == -1 and "nfields = -1" in msg
    st, msg = _status(lib.nk_grid_fields_code_object, src, 2, 1, 0, 0, 2, 5, 0, None, 0, C.byref(nb))
    assert st == -1 and "nfields = 5" in msg
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 4, 1, 0, 0, 2, 1, C.byref(nb))
    assert st == -1 and "dim = 4" in msg
    # a source with the contract without fields, compiled for a problem with one: the message shows the field contract
    st, msg = _status(lib.nk_grid_fields_compile_check, R.OLD_SIGNATURE_SRC.encode(), 2, 1, 0, 0, 2, 1, C.byref(nb))
    assert st == -1 and "const nk_flds &a" in msg and "a(di, dj, k)" in msg and "nk_point" in msg
    st, msg = _status(lib.nk_grid_fields_compile_check, G3.BRATU3_SRC.encode(), 3, 1, 0, 0, 2, 1, C.byref(nb))
    assert st == -1 and "const nk_flds3 &a" in msg and "a(di, dj, dk, k)" in msg
    # and the other way round: a field source compiled without fields gets the contract it has always had
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 2, 1, 0, 0, 2, 0, C.byref(nb))
    assert st == -1 and "nk_flds" not in msg.split("):")[0] and "nk_nbhd<T> &u, const nk_real *p" in msg
    # a field read outside the stencil's shape compiles (it is NaN at run time, as for u); what the geometry refuses stays refused
    st, msg = _status(lib.nk_grid_fields_compile_check, src, 2, 5, 0, 0, 2, 1, C.byref(nb))
    assert st == -1 and "dof = 5" in msg
    import nonlinearsolve_jl_amd as nls
    with pytest.raises(nls.NKError, match="nfields = 7"):
        nls.grid_compile_check(R.PROBLEMS["bratu_f"].source, nparams=2, fields=7)


def _code_object(fn, *args):
    nb = C.c_int64()
    assert fn(*args, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert fn(*args, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


@pytest.mark.parametrize("jac", [0, 1])
def test_no_fields_through_the_new_entry_point_is_the_old_program(jac):
    """nfields = 0: the bytes of nk_grid_code_object / nk_grid3_code_object on this build"""
    lib = L.lib()
    for p in (G1.PROBLEMS["bratu"], G1.PROBLEMS["box_periodic"]):
        a = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params))
        old = _code_object(lib.nk_grid_code_object, *a, jac)
        new = _code_object(lib.nk_grid_fields_code_object, a[0], 2, *a[1:], 0, jac)
        assert old == new and old[:4] == b"\x7fELF"
    p = G3.PROBLEMS["bratu3"]
    a = (p.source.encode(), p.dof, GC.STENCIL_ID[p.stencil], GC.BOUNDARY_ID[p.boundary], len(p.params))
    assert _code_object(lib.nk_grid3_code_object, *a, jac) == _code_object(lib.nk_grid_fields_code_object, a[0], 3, *a[1:], 0, jac)


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


def _global_loads(path):
    """kernel name → number of global_load instructions in its disassembly (printed for the record, not asserted on a tool
    that may be missing)"""
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.access(objdump, os.X_OK):
        return {}
    txt = subprocess.run([objdump, "-d", str(path)], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and "global_load" in line:
            out[cur] += 1
    return out


@pytest.mark.parametrize("name", sorted(R.PROBLEMS))
def test_generated_kernels_have_no_private_segment(tmp_path, name):
    """all three kernels of every field source are register programs, and the staged fill's LDS is what it is without fields:
    256·npts·dof doubles"""
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not os.access(readelf, os.X_OK):
        pytest.skip("llvm-readelf not installed")
    p = R.PROBLEMS[name]
    for jac, kernels in KERNELS[p.dim].items():
        co = _code_object(L.lib().nk_grid_fields_code_object, *_args(p), jac)
        assert co[:4] == b"\x7fELF"
        path = tmp_path / f"{name}_{jac}.co"
        path.write_bytes(co)
        notes, loads = _kernel_notes(readelf, path), _global_loads(path)
        assert set(notes) == set(kernels), sorted(notes)
        for k in kernels:
            print(f"{name}: {k}: private segment {notes[k][0]}, VGPRs {notes[k][1]}, LDS {notes[k][2]}, "
                  f"global loads {loads.get(k, '?')}")
            assert notes[k][0] == 0, (k, notes)
        if jac == 1 and not os.environ.get("NK_GRID_FILL_DIRECT"):
            assert notes[kernels[0]][2] == 256 * len(p.offsets()) * p.dof * 8


def test_a_declared_field_that_is_not_read_costs_no_load(tmp_path):
    """bratu_f4 declares four fields and reads one: its kernels have the global loads of bratu_f, one per value that reaches the
    result — the residual u at five points and the field at the centre; the JVP v at five points, u at the centre (eᵘ) and the
    field there (u's four neighbour values do not reach J·v and are dropped like an unread field)"""
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.access(objdump, os.X_OK):
        pytest.skip("llvm-objdump not installed")
    counts = {}
    for name in ("bratu_f", "bratu_f4"):
        co = _code_object(L.lib().nk_grid_fields_code_object, *_args(R.PROBLEMS[name]), 0)
        path = tmp_path / f"{name}.co"
        path.write_bytes(co)
        counts[name] = _global_loads(path)
    print(counts)
    assert counts["bratu_f"] == counts["bratu_f4"]
    assert counts["bratu_f"]["nk_grid_residual"] == 5 + 1 and counts["bratu_f"]["nk_grid_jvp"] == 5 + 1 + 1
