"""Ensemble throughput of the Jacobian-free methods (SimpleBroyden, SimpleKlement, SimpleDFSane) against SimpleNewtonRaphson on
the same systems: inputs already on the device, HIP events around the C-ABI call, the four methods alternating call by call,
min over the timed calls. For each case and precision: systems/s, mean iterations and the share of systems that end in
Success, each precision at its own default abstol. Then the kernels' VGPR counts and private-segment sizes from the
code-object notes (nk_batch_jf_code_object / nk_batch_code_object + llvm-readelf).

    python tools/ensemble_jf_bench.py [--nbatch 1048576] [--reps 10] [--dtype both|float32|float64]

Quadratic parameters lie in [1, 4], where the Float32 default abstol (2.9e-6) is reachable."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch

import nonlinearsolve_jl_amd as nls
import simple_jf_reference as R
from nonlinearsolve_jl_amd import _lib as L
from nonlinearsolve_jl_amd.core import _BatchKernel

ap = argparse.ArgumentParser()
ap.add_argument("--nbatch", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--dtype", choices=("both", "float32", "float64"), default="both")
a = ap.parse_args()
nb = a.nbatch
dtypes = ("float64", "float32") if a.dtype == "both" else (a.dtype,)
METHODS = ("SimpleNewtonRaphson", "SimpleBroyden", "SimpleKlement", "SimpleDFSane")
ctx = nls.default_context()
lib = L.lib()
rng = np.random.default_rng(0)
ptr = lambda x: C.c_void_p(x.data_ptr())
cases = [("quadratic n=4", R.QUADRATIC, 4, np.ones(4), rng.uniform(1.0, 4.0, (nb, 4)), 1000),
         ("quadratic n=8", R.QUADRATIC, 8, np.ones(8), rng.uniform(1.0, 4.0, (nb, 8)), 1000),
         ("tutorial p2_f n=4, maxiters 100", R.P2, 4, np.array([1.0, 2.0, 3.0, 4.0]), rng.random((nb, 4)) + 0.05, 100)]
cases += [(f"dense coupled n={n}, maxiters 100", R.DENSE_COUPLED, n, np.ones(n), rng.uniform(1.0, 4.0, (nb, n)), 100)
          for n in (16, 32)]


def call(method, f32, h, b, maxit):
    sfx = "_f32" if f32 else ""
    head = (h, nb, ptr(b["u0"]), 0, ptr(b["p"]), L.DEVICE, 0.0, maxit)
    outs = (ptr(b["u"]), ptr(b["r"]), ptr(b["rc"]), ptr(b["it"]))
    if method == "SimpleNewtonRaphson":
        return getattr(lib, "nk_batch_solve" + sfx)(*head, *outs)
    if method == "SimpleBroyden":
        return getattr(lib, "nk_batch_solve_broyden" + sfx)(*head, -1.0, *outs)
    if method == "SimpleKlement":
        return getattr(lib, "nk_batch_solve_klement" + sfx)(*head, *outs)
    return getattr(lib, "nk_batch_solve_dfsane" + sfx)(*head, -1.0, -1.0, -1.0, 0, -1.0, -1.0, -1.0, 0, *outs)


print(f"# {nb} systems per call, {a.reps} timed calls per method (alternating), min over calls; "
      f"device: {torch.cuda.get_device_name(0)}", flush=True)
for name, src, n, u0, P, maxit in cases:
    for dt in dtypes:
        f32 = dt == "float32"
        tdt = torch.float32 if f32 else torch.float64
        h = _BatchKernel.get(ctx, src, n, P.shape[1], L.BATCH_FLOAT32 if f32 else 0)
        u0d = torch.tensor(u0, dtype=tdt, device="cuda")
        pd = torch.tensor(P.astype(np.float32), device="cuda").to(tdt).contiguous()
        runs = {m: dict(b=dict(u0=u0d, p=pd, u=torch.empty((nb, n), dtype=tdt, device="cuda"),
                               r=torch.empty((nb, n), dtype=tdt, device="cuda"),
                               rc=torch.empty(nb, dtype=torch.int32, device="cuda"),
                               it=torch.empty(nb, dtype=torch.int32, device="cuda")), ts=[]) for m in METHODS}
        for m, Rn in runs.items():         # warm-up (compiles the Jacobian-free module on the first call)
            assert call(m, f32, h, Rn["b"], maxit) == 0, lib.nk_last_error()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m, Rn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st = call(m, f32, h, Rn["b"], maxit)
                e1.record()
                torch.cuda.synchronize()
                assert st == 0, lib.nk_last_error()
                Rn["ts"].append(e0.elapsed_time(e1) * 1e-3)
        parts = []
        for m, Rn in runs.items():
            t = min(Rn["ts"])
            it = Rn["b"]["it"].cpu().numpy().astype(np.int64)
            ok = (Rn["b"]["rc"].cpu().numpy() == 1).mean() * 100
            parts.append(f"{m[6:]} {nb / t / 1e6:.1f} M/s ({t * 1e3:.3f} ms; {it.mean():.2f} it, {ok:.1f} % ok)")
        print(f"{name} {dt}: " + "; ".join(parts), flush=True)
        del runs, u0d, pd
        torch.cuda.empty_cache()

# ---- kernel resources from the code-object notes
readelf = "/opt/rocm/llvm/bin/llvm-readelf"
if not os.access(readelf, os.X_OK):
    print("# kernel resources: llvm-readelf not available")
    sys.exit(0)
print("# kernel resources (code-object notes): vgpr / private segment bytes")
for name, src, n, _u0, P, _m in cases:
    for dt in dtypes:
        flags = L.BATCH_FLOAT32 if dt == "float32" else 0
        blobs = []
        for jf in (False, True):
            nbytes = C.c_int64()
            f = (lambda buf, cap: lib.nk_batch_jf_code_object(src.encode(), n, P.shape[1], flags, buf, cap, C.byref(nbytes))) \
                if jf else (lambda buf, cap: lib.nk_batch_code_object(src.encode(), n, P.shape[1], flags, 0, buf, cap,
                                                                      C.byref(nbytes)))
            assert f(None, 0) == 0, lib.nk_last_error()
            buf = C.create_string_buffer(nbytes.value)
            assert f(buf, nbytes.value) == 0
            blobs.append(buf.raw[:nbytes.value])
        row = []
        for blob in blobs:
            with tempfile.NamedTemporaryFile(suffix=".co") as co:
                co.write(blob)
                co.flush()
                notes = subprocess.run([readelf, "--notes", co.name], capture_output=True, text=True, check=True).stdout
            for block in re.split(r"\n\s*- \.", notes)[1:]:
                nm = re.search(r"\.name:\s+(\w+)", block)
                if not nm or nm.group(1).endswith(".kd") or nm.group(1) == "nk_batch_trust_region":
                    continue
                g = lambda key: (re.search(r"\.%s:\s+(\d+)" % key, block) or [None, "?"])[1]
                row.append(f"{nm.group(1)[9:]} {g('vgpr_count')}/{g('private_segment_fixed_size')}")
        print(f"#   {name} {dt}: " + ", ".join(row))
