"""Ensemble SimpleTrustRegion for 8 < n <= 64 on one MI355X: one system per thread (nk_batch_trust_region, the kernel there was
before the per-wavefront one) against one system per wavefront (nk_batch_trust_region_wave), with SimpleNewtonRaphson on its
wavefront kernel for scale. Float64 and Float32; the dense coupled residual of the tests from their rough starts; batches
sized by the rule of tools/ensemble_sizes.py (2^20 / (n/4) systems: the chip several times over); device tensors in and out;
maxiters = 300; HIP events around the solve call; one warm-up of every case, then the minimum of 5, the three cases taking
turns inside every repetition. The threshold NK_BATCH_TR_WAVE_MIN_N of nk_batch.hip follows from the table this prints.

    python tools/ensemble_wave_tr_bench.py [--out profiles/ensemble_wave_tr.json] [--sizes 9,12,16,24,32,48,64] [--commit HASH]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

import nonlinearsolve_jl_amd as nls   # noqa: E402
from ensemble_f32 import DENSE_COUPLED   # noqa: E402  (the nk_real contract: one source for both precisions)

MAXITERS, REPS = 300, 5


def _commit(given):
    if given:
        return given
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def _rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        return "unknown"


def _timed(prob, alg, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    # device tensors in and out; the call ends by reading the retcodes and step counts (two int32 per system) back to the host
    sol = nls.vectorized_solve(prob, alg, maxiters=MAXITERS, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, sol


def measure(n, f32):
    nb = (1 << 20) // max(1, n // 4)
    rng = np.random.default_rng(n)
    P = rng.uniform(1.0, 4.0, (nb, n))
    u0 = rng.uniform(0.5, 2.0, (nb, n)) + 1.5 * rng.standard_normal((nb, n))
    tdt = torch.float32 if f32 else torch.float64
    prob = nls.ImmutableNonlinearProblem(DENSE_COUPLED, torch.tensor(u0, dtype=tdt, device="cuda"),
                                         torch.tensor(P, dtype=tdt, device="cuda"), eltype=np.float32 if f32 else None)
    cases = {"tr_per_thread": (nls.SimpleTrustRegion(), {"per_wavefront": False}),
             "tr_per_wavefront": (nls.SimpleTrustRegion(), {"per_wavefront": True}),
             "newton_per_wavefront": (nls.SimpleNewtonRaphson(), {"per_wavefront": True})}
    best, last = {}, {}
    for rep in range(REPS + 1):                        # repetition 0 compiles, loads and warms up
        for name, (alg, kw) in cases.items():
            dt, sol = _timed(prob, alg, **kw)
            if rep:
                best[name] = min(best.get(name, dt), dt)
            last[name] = sol
    row = {"n": n, "precision": "float32" if f32 else "float64", "systems": nb}
    for name, sol in last.items():
        row[name] = {"kernel": sol.kernel, "seconds": best[name], "systems_per_s": nb / best[name],
                     "mean_steps": float(sol.iters.mean()), "success_share": float((sol.retcode_raw == 1).mean())}
    a, b = row["tr_per_thread"], row["tr_per_wavefront"]
    row["wavefront_over_thread"] = b["systems_per_s"] / a["systems_per_s"]
    same = (last["tr_per_thread"].retcode_raw == last["tr_per_wavefront"].retcode_raw)
    row["retcodes_equal_share"] = float(same.mean())
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_wave_tr.json"))
    ap.add_argument("--sizes", default="9,12,16,24,32,48,64")
    ap.add_argument("--commit", default=None, help="the commit measured, where the tree is not a git checkout")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this measurement needs the GPU: nothing is timed without one")
    result = {"what": "ensemble SimpleTrustRegion, one system per thread vs one per wavefront; min of %d after a warm-up" % REPS,
              "device": torch.cuda.get_device_name(0), "commit": _commit(args.commit), "rocm": _rocm_version(),
              "hip": torch.version.hip, "maxiters": MAXITERS, "rows": []}
    for f32 in (False, True):
        for n in (int(s) for s in args.sizes.split(",")):
            row = measure(n, f32)
            result["rows"].append(row)
            a, b, c = row["tr_per_thread"], row["tr_per_wavefront"], row["newton_per_wavefront"]
            print(f"{row['precision']} n={n:2d} {row['systems']:7d} systems | per thread {a['systems_per_s']:.3e}/s "
                  f"({a['mean_steps']:.1f} steps, ok {a['success_share']:.3f}) | per wavefront {b['systems_per_s']:.3e}/s "
                  f"({b['mean_steps']:.1f} steps, ok {b['success_share']:.3f}) = x{row['wavefront_over_thread']:.2f} | "
                  f"Newton per wavefront {c['systems_per_s']:.3e}/s ({c['mean_steps']:.1f} steps, ok {c['success_share']:.3f})",
                  flush=True)
            with open(args.out, "w") as fh:            # after every row: a partial table survives a time limit
                json.dump(result, fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
