"""Ensemble throughput in Float32 against Float64: the same systems, inputs already on the device, HIP events around the
C-ABI call (nk_batch_solve / nk_batch_solve_f32), the two precisions alternating call by call. For each case: systems/s in
each precision, their ratio, and the share of systems on which both precisions report the same retcode and step count.

    python tools/ensemble_precision_bench.py [--nbatch 1048576] [--reps 20] [--dtype both|float32|float64]

Quadratic parameters lie in [1, 4]: the Float32 default abstol (2.9e-6) is reachable there (u*u - p cannot go below
ulp(p)), so that both precisions do the same Newton work."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

import ensemble_f32 as F
import nonlinearsolve_jl_amd as nls
from nonlinearsolve_jl_amd import _lib as L
from nonlinearsolve_jl_amd.core import _BatchKernel

ap = argparse.ArgumentParser()
ap.add_argument("--nbatch", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--dtype", choices=("both", "float32", "float64"), default="both")
a = ap.parse_args()
nb = a.nbatch
dtypes = ("float64", "float32") if a.dtype == "both" else (a.dtype,)
ctx = nls.default_context()
rng = np.random.default_rng(0)
ptr = lambda x: C.c_void_p(x.data_ptr())
cases = [("quadratic n=4", F.QUADRATIC, 4, np.ones(4), rng.uniform(1.0, 4.0, (nb, 4)), 1000),
         ("quadratic n=8", F.QUADRATIC, 8, np.ones(8), rng.uniform(1.0, 4.0, (nb, 8)), 1000),
         ("tutorial p2_f n=4, maxiters 100", F.P2, 4, np.array([1.0, 2.0, 3.0, 4.0]), rng.random((nb, 4)) + 0.05, 100)]
cases += [(f"dense coupled n={n} (wave kernel)", F.DENSE_COUPLED, n, np.ones(n), rng.uniform(1.0, 4.0, (nb, n)), 100)
          for n in (16, 32, 64)]
print(f"# {nb} systems per call, {a.reps} timed calls per precision (alternating), min over calls; "
      f"device: {torch.cuda.get_device_name(0)}", flush=True)
for name, src, n, u0, P, maxit in cases:
    runs = {}
    for dt in dtypes:
        tdt = torch.float32 if dt == "float32" else torch.float64
        P32 = P.astype(np.float32)          # both precisions solve the float32-rounded parameters
        h = _BatchKernel.get(ctx, src, n, P.shape[1], L.BATCH_FLOAT32 if dt == "float32" else 0)
        fn = L.lib().nk_batch_solve_f32 if dt == "float32" else L.lib().nk_batch_solve
        bufs = dict(u0=torch.tensor(u0, dtype=tdt, device="cuda"), p=torch.tensor(P32, device="cuda").to(tdt).contiguous(),
                    u=torch.empty((nb, n), dtype=tdt, device="cuda"), r=torch.empty((nb, n), dtype=tdt, device="cuda"),
                    rc=torch.empty(nb, dtype=torch.int32, device="cuda"), it=torch.empty(nb, dtype=torch.int32, device="cuda"))
        runs[dt] = dict(h=h, fn=fn, b=bufs, ts=[])
    del P
    call = lambda R: R["fn"](R["h"], nb, ptr(R["b"]["u0"]), 0, ptr(R["b"]["p"]), L.DEVICE, 0.0, maxit, ptr(R["b"]["u"]),
                             ptr(R["b"]["r"]), ptr(R["b"]["rc"]), ptr(R["b"]["it"]))
    for R in runs.values():                 # warm-up
        assert call(R) == 0, L.lib().nk_last_error()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for R in runs.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = call(R)
            e1.record()
            torch.cuda.synchronize()
            assert st == 0, L.lib().nk_last_error()
            R["ts"].append(e0.elapsed_time(e1) * 1e-3)
    line = [f"{name}:"]
    for dt, R in runs.items():
        t = min(R["ts"])
        it = R["b"]["it"].cpu().numpy().astype(np.int64)
        ok = (R["b"]["rc"].cpu().numpy() == 1).mean() * 100
        R["sps"] = nb / t
        line.append(f"{dt} {nb / t / 1e6:.1f} M systems/s ({t * 1e3:.3f} ms, median {np.median(R['ts']) * 1e3:.3f}; "
                    f"mean {it.mean():.2f} steps, {ok:.1f} % Success);")
    if len(runs) == 2:
        r32, r64 = runs["float32"], runs["float64"]
        same = ((r32["b"]["rc"] == r64["b"]["rc"]) & (r32["b"]["it"] == r64["b"]["it"])).float().mean().item() * 100
        line.append(f"float32/float64 = {r32['sps'] / r64['sps']:.2f}x; same (retcode, steps) on {same:.2f} % of the systems")
    print(" ".join(line), flush=True)
    del runs
    torch.cuda.empty_cache()
