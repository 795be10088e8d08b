"""The per-wavefront SimpleTrustRegion kernel (nk_batch_trust_region_wave) compiles for gfx950 without a GPU into a code
object of its own (nk_batch_code_object, wave = 2), in both precisions: it holds that kernel and no other, runs without FP64
instructions in Float32, moves values between lanes with v_readlane, and leaves scratch memory — none where the Newton
wavefront kernel leaves room in the register file, below a tenth of the per-thread kernel's everywhere else. The two older
kernel sets keep exactly their kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

import wave_tr_cases as W
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
F32_FLAG = L.BATCH_FLOAT32
SRC = W.DENSE_COUPLED
WAVE_TR = "nk_batch_trust_region_wave"
# the sizes at which the Newton wavefront kernel needs at most 400 of the 512 registers: the extra state fits
NO_SCRATCH = {0: 24, F32_FLAG: 48}


def _code_object(src, n, npar, flags, wave):
    """one call into a buffer that is large enough (a size query first would compile twice: 14 s each at n = 64 in Float64)"""
    nb, cap = C.c_int64(), 1 << 22
    buf = C.create_string_buffer(cap)
    assert L.lib().nk_batch_code_object(src.encode(), n, npar, flags, wave, buf, cap, C.byref(nb)) == 0, L.lib().nk_last_error()
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
@pytest.mark.parametrize("n", [9, 16, 24, 33, 48, 64])
def test_wave_tr_code_object(tmp_path, n, flags):
    ks, seg = _inspect(tmp_path, _code_object(SRC, n, n, flags, 2))
    assert set(ks) == {WAVE_TR}, sorted(ks)
    assert len(ks[WAVE_TR]) > 200
    if flags & F32_FLAG:
        f64 = sorted({i for i in ks[WAVE_TR] if i.startswith("v_") and "f64" in i})
        assert not f64, f64
        assert "v_readlane_b32" in ks[WAVE_TR]
    if n <= NO_SCRATCH[flags]:
        assert seg[WAVE_TR] == 0, seg
    else:
        _, per_thread = _inspect(tmp_path, _code_object(SRC, n, n, flags, 0))
        print(f"n = {n}: private segment {seg[WAVE_TR]} B per lane, nk_batch_trust_region {per_thread['nk_batch_trust_region']} B")
        assert 10 * seg[WAVE_TR] < per_thread["nk_batch_trust_region"], (seg, per_thread)


@pytest.mark.parametrize("flags", [0, F32_FLAG], ids=["float64", "float32"])
def test_older_kernel_sets_keep_exactly_their_kernels(tmp_path, flags):
    ks, _ = _inspect(tmp_path, _code_object(SRC, 9, 9, flags, 0))
    assert set(ks) == {"nk_batch_newton", "nk_batch_trust_region"}, sorted(ks)
    ks, _ = _inspect(tmp_path, _code_object(SRC, 9, 9, flags, 1))
    assert set(ks) == {"nk_batch_newton_wave"}, sorted(ks)


def test_code_object_arguments():
    nb = C.c_int64()
    src = SRC.encode()
    assert L.lib().nk_batch_code_object(src, 9, 9, 0, 2, None, 0, C.byref(nb)) == 0 and nb.value > 1000
    assert L.lib().nk_batch_code_object(src, 9, 9, 0, 3, None, 0, C.byref(nb)) != 0              # wave > 2
    assert b"wave = 3" in L.lib().nk_last_error()
    assert L.lib().nk_batch_code_object(src, 65, 9, 0, 2, None, 0, C.byref(nb)) != 0             # n outside 1..64
    assert L.lib().nk_batch_code_object(b"this is not C++", 9, 9, 0, 2, None, 0, C.byref(nb)) != 0
    small = C.create_string_buffer(16)
    assert L.lib().nk_batch_code_object(src, 9, 9, 0, 2, small, 16, C.byref(nb)) != 0            # buffer too small
    assert _code_object(SRC, 9, 9, F32_FLAG, 2)[:4] == b"\x7fELF"


def test_compile_check_accepts_per_thread():
    """with NK_BATCH_PER_THREAD the check compiles the per-thread set alone: fewer code bytes than with the wavefront kernel"""
    assert L.BATCH_PER_THREAD == 4
    both, alone = C.c_int64(), C.c_int64()
    assert L.lib().nk_batch_compile_check(SRC.encode(), 9, 9, 0, C.byref(both)) == 0, L.lib().nk_last_error()
    assert L.lib().nk_batch_compile_check(SRC.encode(), 9, 9, L.BATCH_PER_THREAD, C.byref(alone)) == 0, L.lib().nk_last_error()
    assert 0 < alone.value < both.value
    assert L.lib().nk_batch_compile_check(SRC.encode(), 9, 9, L.BATCH_PER_THREAD | F32_FLAG, C.byref(alone)) == 0


def test_last_kernel_of_a_null_object():
    assert L.lib().nk_batch_last_kernel(None) is None
