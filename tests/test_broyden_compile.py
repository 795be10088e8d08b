"""csrc/nk_qn.hip cross-compiles for gfx950 without a GPU, and none of the kernels of Broyden and Klement — the two passes over
the dense inverse Jacobian first of all, with their 32 row accumulators per lane — has a private segment or spills vector
registers. Read from the compiler's resource remarks, as tests/test_lbroyden_compile.py reads them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinearsolve.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ["k_qn_update", "k_qn_reduce", "k_bd_fill", "k_bd_pass_a", "k_bd_fold", "k_bd_pass_b", "k_bd_diag_update", "k_kl_step"]


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("qn") / "nk_qn.o"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "nk_qn.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:.*?(Function Name|ScratchSize \[bytes/lane\]|VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return rows


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_private_segment_and_no_spill(remarks, kernel):
    hits = {n: r for n, r in remarks.items() if n.startswith("_Z%d%s" % (len(kernel), kernel))}   # (the length prefix makes the name exact)
    assert len(hits) == 1, sorted(remarks)
    (name, r), = hits.items()
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
    assert r["Occupancy [waves/SIMD]"] >= 1
