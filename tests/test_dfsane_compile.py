"""The two DFSane kernels of csrc/nk_qn.hip — the trial point and the one-pass reduction over f_t and f — cross-compile for
gfx950 without a GPU, with no private segment and no spills. Read from the compiler's resource remarks, as
tests/test_lbroyden_compile.py reads them for the other kernels of that object."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinearsolve.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("sane") / "nk_qn.o"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "nk_qn.hip"), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:.*?(Function Name|ScratchSize \[bytes/lane\]|VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return rows


@pytest.mark.parametrize("kernel", ["k_sane_trial", "k_sane_reduce"])
def test_no_private_segment_and_no_spills(remarks, kernel):
    hits = {n: r for n, r in remarks.items() if n.startswith("_Z%d%s" % (len(kernel), kernel))}   # (the length makes it exact)
    assert len(hits) == 1, sorted(remarks)
    (name, r), = hits.items()
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (name, r)
    assert r["Occupancy [waves/SIMD]"] >= 4      # streaming kernels: nothing in them needs a large register file
