"""Float32 ensembles (flags & NK_BATCH_FLOAT32) compile for gfx950 without a GPU: the residual contract in nk_real, the
per-thread and per-wavefront kernels at the sizes that pick them, and the instructions that come out — no FP64 VALU work
and, while n ≤ 8, no private segment."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ensemble_f32 as F
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
F32_FLAG, JAC_FLAG = L.BATCH_FLOAT32, L.BATCH_ANALYTIC_JAC


def _code_object(src, n, npar, flags, wave):
    nb = C.c_int64()
    assert L.lib().nk_batch_code_object(src.encode(), n, npar, flags, wave, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_batch_code_object(src.encode(), n, npar, flags, wave, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


def _llvm_tools():
    tools = (os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf"))
    if not all(os.access(t, os.X_OK) for t in tools):
        pytest.skip("LLVM objdump / readelf not installed")
    return tools


@pytest.mark.parametrize("n,flags", [(1, 2), (4, 2), (8, 2), (9, 2), (33, 2), (64, 2), (3, 3)])
def test_float32_sources_compile_for_gfx950(n, flags):
    nb = C.c_int64()
    src = F.TRIG_WITH_JAC if flags & JAC_FLAG else F.DENSE_COUPLED
    assert L.lib().nk_batch_compile_check(src.encode(), n, n, flags, C.byref(nb)) == 0, L.lib().nk_last_error()
    assert nb.value > 1000
    if flags & JAC_FLAG:
        return
    for src, npar in ((F.QUADRATIC, n), (F.P2, 4)):
        if src is F.P2 and n != 4:
            continue
        assert L.lib().nk_batch_compile_check(src.encode(), n, npar, flags, C.byref(nb)) == 0, L.lib().nk_last_error()
        # the analytic-Jacobian bit with a source that has no nk_jac must fail the per-thread build, in either mode
        assert L.lib().nk_batch_compile_check(src.encode(), n, npar, flags | JAC_FLAG, C.byref(nb)) != 0


@pytest.mark.parametrize("n", [4, 9, 33, 64])
def test_nk_real_sources_also_compile_as_float64(n):
    nb = C.c_int64()
    assert L.lib().nk_batch_compile_check(F.DENSE_COUPLED.encode(), n, n, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    assert L.lib().nk_batch_compile_check(F.TRIG_WITH_JAC.encode(), 3, 3, JAC_FLAG, C.byref(nb)) == 0, L.lib().nk_last_error()


def test_float64_contract_source_fails_in_float32_mode_with_the_contract():
    nb = C.c_int64()
    assert L.lib().nk_batch_compile_check(F.DOUBLE_CONTRACT.encode(), 4, 4, 0, C.byref(nb)) == 0   # fine as Float64
    assert L.lib().nk_batch_compile_check(F.DOUBLE_CONTRACT.encode(), 4, 4, F32_FLAG, C.byref(nb)) != 0
    err = L.lib().nk_last_error().decode()
    assert "Float32" in err and "const nk_real *p" in err and "nk_f" in err, err
    assert L.lib().nk_batch_compile_check(F.DOUBLE_CONTRACT.encode(), 33, 33, F32_FLAG, C.byref(nb)) != 0
    jac64 = F.TRIG_WITH_JAC.replace("const nk_real *u, const nk_real *p, nk_real *J", "const double *u, const double *p, double *J")
    assert L.lib().nk_batch_compile_check(jac64.encode(), 3, 3, F32_FLAG | JAC_FLAG, C.byref(nb)) != 0
    assert "nk_jac" in L.lib().nk_last_error().decode()


def test_code_object_entry_point_reports_size_and_refuses_a_short_buffer():
    nb = C.c_int64()
    assert L.lib().nk_batch_code_object(F.P2.encode(), 4, 4, F32_FLAG, 0, None, 0, C.byref(nb)) == 0
    assert nb.value > 1000
    small = C.create_string_buffer(16)
    assert L.lib().nk_batch_code_object(F.P2.encode(), 4, 4, F32_FLAG, 0, small, 16, C.byref(nb)) != 0
    assert _code_object(F.P2, 4, 4, F32_FLAG, 0)[:4] == b"\x7fELF"


def _kernels(disasm):
    """kernel symbol → list of instruction mnemonics (llvm-objdump -d)"""
    out, cur = {}, None
    for line in disasm.splitlines():
        m = re.match(r"^[0-9a-f]+ <([A-Za-z0-9_]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+([a-z_][a-z0-9_]*)\b", line)
        if cur is not None and m:
            cur.append(m.group(1))
    return out


@pytest.mark.parametrize("src,n,npar,flags,wave,names", [
    (F.P2, 4, 4, F32_FLAG, 0, ("nk_batch_newton", "nk_batch_trust_region")),
    (F.QUADRATIC, 8, 8, F32_FLAG, 0, ("nk_batch_newton", "nk_batch_trust_region")),
    (F.TRIG_WITH_JAC, 3, 3, F32_FLAG | JAC_FLAG, 0, ("nk_batch_newton", "nk_batch_trust_region")),
    (F.DENSE_COUPLED, 33, 33, F32_FLAG, 1, ("nk_batch_newton_wave",)),
    (F.DENSE_COUPLED, 64, 64, F32_FLAG, 1, ("nk_batch_newton_wave",)),
])
def test_float32_kernels_have_no_fp64_valu_and_no_scratch(tmp_path, src, n, npar, flags, wave, names):
    objdump, readelf = _llvm_tools()
    co = tmp_path / "k.co"
    co.write_bytes(_code_object(src, n, npar, flags, wave))
    dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", str(co)], capture_output=True, text=True, check=True).stdout
    ks = _kernels(dis)
    for k in names:
        assert k in ks and len(ks[k]) > 50, (k, sorted(ks))
        f64 = sorted({i for i in ks[k] if i.startswith("v_") and "f64" in i})
        assert not f64, (k, f64)
    if wave:   # one 32-bit readlane per value crossing lanes: the wave kernel's Float64 form needs two
        assert sum(i == "v_readlane_b32" for i in ks["nk_batch_newton_wave"]) > 0
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    seg = dict(re.findall(r"\.name:\s+(\w+)\s[\s\S]*?\.private_segment_fixed_size:\s+(\d+)", notes))
    if not seg:   # the fields may come in another order: pair each kernel's block by its .name
        for block in notes.split("- .agpr_count")[1:]:
            nm = re.search(r"\.name:\s+(\w+)", block)
            ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if nm and ps:
                seg[nm.group(1)] = ps.group(1)
    for k in names:
        assert k in seg, (k, seg)
        if n <= 8:
            assert int(seg[k]) == 0, (k, seg[k])
