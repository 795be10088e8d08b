"""Ensemble throughput of the least-squares kernels (SimpleGaussNewton, SimpleTrustRegion on m residuals and n unknowns, one
fit per GPU thread) for a few (m, n) in both precisions: inputs already on the device, HIP events around the C-ABI call, the
methods alternating call by call, min over the timed calls. For each case: fits/s, mean iterations and the share of fits
that end in Success, each precision at its own default abstol. As a comparison line the same fits run through the existing
square Newton kernel (nk_batch_solve) on the hand-formed normal equations Jᵀf = 0 — what a user had to do before, with
the condition number squared and max|Jᵀf| ≤ abstol as the stopping test, so its iteration counts are not the same quantity.
Then the kernels' VGPR counts and private-segment sizes from the code-object notes.

    python tools/ensemble_nlls_bench.py [--nbatch 1048576] [--reps 10] [--dtype both|float32|float64]

The fits have zero residual at the optimum (data generated from the model), so that Success is reachable."""
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
import simple_nlls_reference as R
from nonlinearsolve_jl_amd import _lib as L
from nonlinearsolve_jl_amd.core import _BatchKernel

# the normal equations g(u) = J(u)ᵀ f(u) of the two algebraic models, n equations in n unknowns; p as in the fits
MM_NORMAL = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *g) {
  T g0 = T(nk_real(0)), g1 = T(nk_real(0));
#pragma unroll
  for (int i = 0; i < NK_NP / 2; ++i) {
    const nk_real x = p[2 * i];
    const T d = nk_real(1) / (u[1] + x);
    const T f = u[0] * x * d - p[2 * i + 1];
    g0 = g0 + f * (x * d);
    g1 = g1 - f * (u[0] * x * d * d);
  }
  g[0] = g0; g[1] = g1;
}
"""
RATIONAL_NORMAL = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *g) {
  T g0 = T(nk_real(0)), g1 = T(nk_real(0)), g2 = T(nk_real(0));
#pragma unroll
  for (int i = 0; i < NK_NP / 2; ++i) {
    const nk_real x = p[2 * i];
    const T d = nk_real(1) / (nk_real(1) + u[2] * x);
    const T q = (u[0] + u[1] * x) * d;
    const T f = q - p[2 * i + 1];
    g0 = g0 + f * d;
    g1 = g1 + f * (x * d);
    g2 = g2 - f * (q * x * d);
  }
  g[0] = g0; g[1] = g1; g[2] = g2;
}
"""

ap = argparse.ArgumentParser()
ap.add_argument("--nbatch", type=int, default=1 << 20)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--dtype", choices=("both", "float32", "float64"), default="both")
a = ap.parse_args()
nb = a.nbatch
dtypes = ("float64", "float32") if a.dtype == "both" else (a.dtype,)
ctx = nls.default_context()
lib = L.lib()
ptr = lambda x: C.c_void_p(x.data_ptr())


def tiled(fam):
    """the family's committed problems repeated up to nbatch"""
    reps = -(-nb // fam.p.shape[0])
    return np.tile(fam.u0, (reps, 1))[:nb], np.tile(fam.p, (reps, 1))[:nb]


cases = [("exp·cos m=5 n=4", R.expcos_family(), None), ("rational m=8 n=3", R.rational_family(), RATIONAL_NORMAL),
         ("Michaelis-Menten m=8 n=2", R.michaelis_menten_family(8), MM_NORMAL),
         ("Michaelis-Menten m=16 n=2", R.michaelis_menten_family(16), MM_NORMAL),
         ("Michaelis-Menten m=64 n=2", R.michaelis_menten_family(64, nb=200), MM_NORMAL)]
TR = (-1.0, -1.0, -1.0, -1.0, -1.0, -1)


def call(method, f32, h, b):
    sfx = "_f32" if f32 else ""
    head = (h, nb, ptr(b["u0"]), 1, ptr(b["p"]), L.DEVICE, 0.0, 1000)
    outs = (ptr(b["u"]), ptr(b["r"]), ptr(b["rc"]), ptr(b["it"]))
    if method == "GaussNewton":
        return getattr(lib, "nk_batch_solve_gauss_newton" + sfx)(*head, *outs)
    if method == "TrustRegion":
        return getattr(lib, "nk_batch_solve_trust_region_nlls" + sfx)(*head, *TR, *outs)
    return getattr(lib, "nk_batch_solve" + sfx)(*head, *outs)      # Newton on the normal equations


print(f"# {nb} fits per call, {a.reps} timed calls per method (alternating), min over calls; "
      f"device: {torch.cuda.get_device_name(0)}", flush=True)
for name, fam, normal in cases:
    u0, P = tiled(fam)
    for dt in dtypes:
        f32 = dt == "float32"
        tdt = torch.float32 if f32 else torch.float64
        flags = L.BATCH_FLOAT32 if f32 else 0
        u0d = torch.tensor(u0, device="cuda").to(tdt).contiguous()
        pd = torch.tensor(P, device="cuda").to(tdt).contiguous()
        hs = {"GaussNewton": (_BatchKernel.get(ctx, fam.source, fam.n, fam.nparams, flags, fam.m), fam.m),
              "TrustRegion": (_BatchKernel.get(ctx, fam.source, fam.n, fam.nparams, flags, fam.m), fam.m)}
        if normal is not None:
            hs["Newton on JᵀF=0"] = (_BatchKernel.get(ctx, normal, fam.n, fam.nparams, flags), fam.n)
        runs = {m: dict(h=h, b=dict(u0=u0d, p=pd, u=torch.empty((nb, fam.n), dtype=tdt, device="cuda"),
                                    r=torch.empty((nb, nr), dtype=tdt, device="cuda"),
                                    rc=torch.empty(nb, dtype=torch.int32, device="cuda"),
                                    it=torch.empty(nb, dtype=torch.int32, device="cuda")), ts=[]) for m, (h, nr) in hs.items()}
        for m, Rn in runs.items():         # warm-up
            assert call(m, f32, Rn["h"], Rn["b"]) == 0, lib.nk_last_error()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for m, Rn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st = call(m, f32, Rn["h"], Rn["b"])
                e1.record()
                torch.cuda.synchronize()
                assert st == 0, lib.nk_last_error()
                Rn["ts"].append(e0.elapsed_time(e1) * 1e-3)
        parts = []
        for m, Rn in runs.items():
            t = min(Rn["ts"])
            it = Rn["b"]["it"].cpu().numpy().astype(np.int64)
            ok = (Rn["b"]["rc"].cpu().numpy() == 1).mean() * 100
            parts.append(f"{m} {nb / t / 1e6:.1f} M fits/s ({t * 1e3:.3f} ms; {it.mean():.2f} it, {ok:.1f} % ok)")
        print(f"{name} {dt}: " + "; ".join(parts), flush=True)
        del runs, u0d, pd
        torch.cuda.empty_cache()

# ---- kernel resources from the code-object notes
readelf = "/opt/rocm/llvm/bin/llvm-readelf"
if not os.access(readelf, os.X_OK):
    print("# kernel resources: llvm-readelf not available")
    sys.exit(0)
print("# kernel resources (code-object notes): vgpr / private segment bytes")
for name, fam, _normal in cases:
    for dt in dtypes:
        flags = L.BATCH_FLOAT32 if dt == "float32" else 0
        nbytes = C.c_int64()
        f = lambda buf, cap: lib.nk_batch_nlls_code_object(fam.source.encode(), fam.n, fam.m, fam.nparams, flags, buf, cap,
                                                           C.byref(nbytes))
        assert f(None, 0) == 0, lib.nk_last_error()
        buf = C.create_string_buffer(nbytes.value)
        assert f(buf, nbytes.value) == 0
        with tempfile.NamedTemporaryFile(suffix=".co") as co:
            co.write(buf.raw[:nbytes.value])
            co.flush()
            notes = subprocess.run([readelf, "--notes", co.name], capture_output=True, text=True, check=True).stdout
        row = []
        for block in re.split(r"\n\s*- \.", notes)[1:]:
            nm = re.search(r"\.name:\s+(\w+)", block)
            if not nm or nm.group(1).endswith(".kd"):
                continue
            g = lambda key: (re.search(r"\.%s:\s+(\d+)" % key, block) or [None, "?"])[1]
            row.append(f"{nm.group(1)[9:]} {g('vgpr_count')}/{g('private_segment_fixed_size')}")
        print(f"#   {name} {dt}: " + ", ".join(row))
