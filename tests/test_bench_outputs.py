"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy — whole when small, a fixed seeded sample when
large, the same from run to run (CPU); and on the device, two runs with the same arguments write the same arrays (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as b
    return b


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(bench, tmp_path):
    rng = np.random.default_rng(3)
    outs = {"u": rng.standard_normal(1000), "fu": rng.standard_normal(1000), "fnorm_inf": 0.25}
    bench.dump_outputs(str(tmp_path), outs, 1, 0, None)
    got = _load(tmp_path)
    assert sorted(got) == ["fnorm_inf", "fu", "u"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["u"], outs["u"]) and np.array_equal(got["fu"], outs["fu"]) and got["fnorm_inf"][0] == 0.25


def test_large_outputs_are_a_fixed_sample_within_the_budget(bench, tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    u, fu = np.arange(n, dtype=np.float64), -np.arange(n, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"u": u, "fu": fu, "fnorm_inf": 1.0}, 1, 0, None)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["fnorm_inf", "fu", "sample_index", "u"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["u"], u[idx]) and np.array_equal(a["fu"], fu[idx])
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 64 << 20


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(nls, tmp_path):
    lines = {}
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", "128", "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300)
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and out, r.stdout[-2000:] + r.stderr[-2000:]
        lines[d] = json.loads(out[-1])
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["fnorm_inf", "fu", "u"] and a["u"].shape == (128 * 128,) and a["fu"].shape == (128 * 128,)
    assert all(np.array_equal(a[k], b[k]) for k in a)   # fixed inputs, fixed work: bit for bit
    assert a["fnorm_inf"][0] == lines["a"]["check"]["fnorm_inf_after_timed_steps"]
    assert lines["a"]["steps"] == 3 and lines["a"]["ms_per_step"] > 0 and lines["a"]["roofline"] is None
