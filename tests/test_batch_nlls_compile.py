"""The least-squares ensemble kernels (nk_batch_gauss_newton, nk_batch_trust_region_nlls) compile for gfx950 without a GPU
into a code object of their own (nk_batch_nlls_code_object), in both precisions: register programs with no private segment
while n ≤ 8 and m·(n + 2) ≤ 80 (Float64) or 128 (Float32), scratch above, no FP64 instruction in Float32, and the contract
in nk_last_error when m < n."""
import ctypes as C
import os
import re
import subprocess

import pytest

import simple_nlls_reference as R
from nonlinearsolve_jl_amd import _lib as L

LLVM = "/opt/rocm/llvm/bin"
F32_FLAG, JAC_FLAG = L.BATCH_FLOAT32, L.BATCH_ANALYTIC_JAC
NLLS = ("nk_batch_gauss_newton", "nk_batch_trust_region_nlls")
PRECISIONS = pytest.mark.parametrize("flags", [0, F32_FLAG], ids=["float64", "float32"])

# a residual of any shape, every unknown used: the probe the register-resident boundary was found with
PROBE = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) f[i] = u[i % NK_N] * u[(i + 3) % NK_N] / (nk_real(1) + u[(i + 1) % NK_N] * p[i]) - p[i];
}
"""


def _code_object(src, n, m, npar, flags):
    nb = C.c_int64()
    assert L.lib().nk_batch_nlls_code_object(src.encode(), n, m, npar, flags, None, 0, C.byref(nb)) == 0, L.lib().nk_last_error()
    buf = C.create_string_buffer(nb.value)
    assert L.lib().nk_batch_nlls_code_object(src.encode(), n, m, npar, flags, buf, nb.value, C.byref(nb)) == 0
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


def _assert_register_program(ks, seg, flags):
    assert set(ks) == set(NLLS), sorted(ks)       # exactly the new kernels
    for k in NLLS:
        assert len(ks[k]) > 50 and seg.get(k) == 0, (k, seg)
        if flags & F32_FLAG:
            f64 = sorted({i for i in ks[k] if i.startswith("v_") and "f64" in i})
            assert not f64, (k, f64)


@PRECISIONS
@pytest.mark.parametrize("src,n,m,npar,jac", [(R.EXPCOS, 4, 5, 5, 0), (R.RATIONAL, 3, 8, 16, 0), (R.MICHAELIS_MENTEN, 2, 16, 32, 0),
                                              (R.POLY_SQUARED, 3, 6, 12, JAC_FLAG), (R.SQUARES_AND_PRODUCTS, 4, 8, 8, 0)])
def test_register_programs_at_small_shapes(tmp_path, src, n, m, npar, jac, flags):
    """the reference shape (m = 5, n = 4), (8, 3) and the other test shapes: exactly the two kernels, no private segment,
    and in Float32 not one v_*f64* instruction (exp and cos included)"""
    ks, seg = _inspect(tmp_path, _code_object(src, n, m, npar, flags | jac))
    _assert_register_program(ks, seg, flags)


@pytest.mark.parametrize("n,m,flags", [(1, 26, 0), (3, 16, 0), (5, 11, 0), (8, 8, 0), (2, 32, F32_FLAG), (4, 21, F32_FLAG),
                                       (7, 14, F32_FLAG), (8, 12, F32_FLAG)])
def test_register_resident_boundary(tmp_path, n, m, flags):
    """the largest m of several n under m·(n + 2) ≤ 80 (Float64) / 128 (Float32): still no private segment in either kernel"""
    assert m * (n + 2) <= (128 if flags else 80) < (m + 1) * (n + 2)
    ks, seg = _inspect(tmp_path, _code_object(PROBE, n, m, m, flags))
    _assert_register_program(ks, seg, flags)


@PRECISIONS
@pytest.mark.parametrize("src,n,m,npar", [(R.MICHAELIS_MENTEN, 2, 64, 128), (R.SQUARES_AND_PRODUCTS, 12, 24, 24), (PROBE, 8, 64, 64)])
def test_scratch_kernels_above_the_boundary(tmp_path, src, n, m, npar, flags):
    """beyond the boundary, and with n > 8: the same two kernels from scratch memory, still FP64-free in Float32"""
    ks, seg = _inspect(tmp_path, _code_object(src, n, m, npar, flags))
    assert set(ks) == set(NLLS), sorted(ks)
    for k in NLLS:
        assert seg[k] > 0, seg
        if flags & F32_FLAG:
            assert not sorted({i for i in ks[k] if i.startswith("v_") and "f64" in i}), k


def test_a_source_for_n_outputs_builds_with_more_residuals_and_fewer_are_refused():
    nb = C.c_int64()
    lib = L.lib()
    src = R.N_OUTPUTS_ONLY.encode()
    for flags in (0, F32_FLAG):
        assert lib.nk_batch_nlls_compile_check(src, 3, 5, 3, flags, C.byref(nb)) == 0, lib.nk_last_error()
        assert nb.value > 1000
        assert lib.nk_batch_nlls_compile_check(src, 3, 3, 3, flags, C.byref(nb)) == 0          # m == n is accepted
        assert lib.nk_batch_nlls_compile_check(src, 3, 2, 3, flags, C.byref(nb)) == -1         # m < n: NK_E_INVALID
        err = lib.nk_last_error()
        assert b"nk_f(const T *u, const nk_real *p, T *f)" in err and b"n <= m <= 64" in err, err
    assert lib.nk_batch_nlls_compile_check(src, 3, 65, 3, 0, C.byref(nb)) == -1
    assert lib.nk_batch_nlls_compile_check(b"this is not C++", 2, 4, 2, 0, C.byref(nb)) != 0


def test_code_object_arguments():
    nb = C.c_int64()
    lib = L.lib()
    src = R.MICHAELIS_MENTEN.encode()
    assert lib.nk_batch_nlls_code_object(src, 2, 8, 16, 0, None, 0, C.byref(nb)) == 0 and nb.value > 1000
    small = C.create_string_buffer(16)
    assert lib.nk_batch_nlls_code_object(src, 2, 8, 16, 0, small, 16, C.byref(nb)) != 0
    assert lib.nk_batch_nlls_code_object(src, 2, 8, 16, 0, None, 0, None) != 0
    assert lib.nk_batch_nlls_code_object(src, 2, 1, 16, 0, None, 0, C.byref(nb)) == -1
    assert _code_object(R.MICHAELIS_MENTEN, 2, 8, 16, F32_FLAG)[:4] == b"\x7fELF"
