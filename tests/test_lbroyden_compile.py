"""csrc/nk_qn.hip cross-compiles for gfx950 without a GPU, and neither of its two streaming kernels — the reduce pass and the
combine pass over U and V — has a private segment or spills, at threshold 10 (the default) and 32 (the widest instance: 64
accumulators, or 64 column values, per lane). Read from the compiler's resource remarks, as tests/test_kernel_resources.py reads
the build's."""
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


@pytest.mark.parametrize("kernel", ["k_lb_reduce", "k_lb_combine"])
@pytest.mark.parametrize("threshold", [10, 32])
def test_no_private_segment(remarks, kernel, threshold):
    hits = {n: r for n, r in remarks.items() if re.search(r"\d+%sILi%dEE" % (kernel, threshold), n)}
    assert len(hits) == 1, sorted(remarks)
    (name, r), = hits.items()
    print(name, r)
    assert r["ScratchSize [bytes/lane]"] == 0 and r.get("VGPRs Spill", 0) == 0, (name, r)
    if threshold == 10:   # (the widest instances keep some of their 64 column addresses in spare vector lanes; the default does not)
        assert r.get("SGPRs Spill", 0) == 0, (name, r)
    assert r["Occupancy [waves/SIMD]"] >= 1


def test_every_column_count_is_instantiated(remarks):
    for kernel in ("k_lb_reduce", "k_lb_combine"):
        got = sorted(int(m.group(1)) for n in remarks for m in [re.search(r"\d+%sILi(\d+)EE" % kernel, n)] if m)
        assert got == list(range(0, 33)), (kernel, got)
    assert all(r["ScratchSize [bytes/lane]"] == 0 for r in remarks.values())
