"""The Jacobian-free ensemble kernels (nk_batch_broyden, nk_batch_klement, nk_batch_dfsane) compile for gfx950 without a
GPU into a code object of their own (nk_batch_jf_code_object), in both precisions: register programs with no private
segment while n ≤ 8 (DFSane's 32-slot history included), no FP64 instruction in Float32, and the Newton code object still
holds exactly its two kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

import simple_jf_reference as R
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
F32_FLAG = L.BATCH_FLOAT32
JF = ("nk_batch_broyden", "nk_batch_klement", "nk_batch_dfsane")


def _jf_code_object(src, n, npar, flags):
    nb = C.c_int64()
    assert L.lib().nk_batch_jf_code_object(src.encode(), n, npar, flags, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_batch_jf_code_object(src.encode(), n, npar, flags, buf, nb.value, C.byref(nb)) == 0
    return buf.raw[:nb.value]


def _llvm_tools():
    tools = (os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf"))
    if not all(os.access(t, os.X_OK) for t in tools):
        pytest.skip("LLVM objdump / readelf not installed")
    return tools


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


def _private_segments(readelf, path):
    """kernel name → .private_segment_fixed_size from the code object's metadata notes"""
    notes = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, check=True).stdout
    seg = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", block)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        if nm and ps and not nm.group(1).endswith(".kd"):
            seg[nm.group(1)] = int(ps.group(1))
    return seg


def _inspect(tmp_path, co):
    objdump, readelf = _llvm_tools()
    path = tmp_path / "k.co"
    path.write_bytes(co)
    dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", str(path)], capture_output=True, text=True, check=True).stdout
    return _kernels(dis), _private_segments(readelf, path)


@pytest.mark.parametrize("flags", [0, F32_FLAG], ids=["float64", "float32"])
@pytest.mark.parametrize("src,n,npar", [(R.QUADRATIC, 1, 1), (R.QUADRATIC, 4, 4), (R.P2, 4, 4), (R.DENSE_COUPLED, 8, 8),
                                        (R.NEWTON_FAILS, 7, 7)])
def test_register_programs_at_small_n(tmp_path, src, n, npar, flags):
    """n ∈ {1, 4, 8}: all three kernels present, no private segment, and in Float32 not one v_*f64* instruction"""
    ks, seg = _inspect(tmp_path, _jf_code_object(src, n, npar, flags))
    for k in JF:
        assert k in ks and len(ks[k]) > 50, (k, sorted(ks))
        assert seg.get(k) == 0, (k, seg)
        if flags & F32_FLAG:
            f64 = sorted({i for i in ks[k] if i.startswith("v_") and "f64" in i})
            assert not f64, (k, f64)
    assert not {"nk_batch_newton", "nk_batch_trust_region", "nk_batch_newton_wave"} & set(ks)


@pytest.mark.parametrize("flags", [0, F32_FLAG], ids=["float64", "float32"])
@pytest.mark.parametrize("n", [9, 33, 64])
def test_scratch_kernels_above_eight(tmp_path, n, flags):
    """8 < n ≤ 64: the same three kernels, per thread from scratch memory, still FP64-free in Float32"""
    ks, seg = _inspect(tmp_path, _jf_code_object(R.DENSE_COUPLED, n, n, flags))
    for k in JF:
        assert k in ks and k in seg, (k, sorted(ks), seg)
        if flags & F32_FLAG:
            assert not sorted({i for i in ks[k] if i.startswith("v_") and "f64" in i}), k
    assert seg["nk_batch_broyden"] > 0   # the n×n inverse lives in scratch


def test_newton_code_object_keeps_exactly_its_kernels(tmp_path):
    for flags in (0, F32_FLAG):
        nb = C.c_int64()
        assert L.lib().nk_batch_code_object(R.P2.encode(), 4, 4, flags, 0, None, 0, C.byref(nb)) == 0
        buf = C.create_string_buffer(nb.value)
        assert L.lib().nk_batch_code_object(R.P2.encode(), 4, 4, flags, 0, buf, nb.value, C.byref(nb)) == 0
        ks, _ = _inspect(tmp_path, buf.raw[:nb.value])
        assert set(ks) == {"nk_batch_newton", "nk_batch_trust_region"}, sorted(ks)


def test_jf_code_object_arguments():
    nb = C.c_int64()
    src = R.QUADRATIC.encode()
    assert L.lib().nk_batch_jf_code_object(src, 4, 4, 0, None, 0, C.byref(nb)) == 0 and nb.value > 1000
    small = C.create_string_buffer(16)
    assert L.lib().nk_batch_jf_code_object(src, 4, 4, 0, small, 16, C.byref(nb)) != 0
    assert L.lib().nk_batch_jf_code_object(src, 65, 4, 0, None, 0, C.byref(nb)) != 0          # n outside 1..64
    assert L.lib().nk_batch_jf_code_object(src, 4, 4, 0, None, 0, None) != 0
    assert L.lib().nk_batch_jf_code_object(b"this is not C++", 4, 4, 0, None, 0, C.byref(nb)) != 0
    assert _jf_code_object(R.QUADRATIC, 4, 4, F32_FLAG)[:4] == b"\x7fELF"
