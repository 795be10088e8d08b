"""Step time of DFSane (csrc/nk_qn.hip, nk_solver.hip: sane_step) on Quadratic at n = 2²⁴ with every step accepted at its first
trial: sigma_1 = 0.4 from u0 = 1.3 converges in five such steps, and with AbsNormTerminationMode at abstol 1e-300 the solve
never terminates (u² − 2 is never exactly 0 in Float64), so every later step does the full work — the trial pass, the residual,
the reduce pass, one fetch of three scalars — whatever the numbers are. The tool checks that the timed steps made one trial each.

Reported: wall-clock ms per fused step (host side included), the device time of the two new passes (the library's per-kernel
event timing, a run of its own) with TB/s on their 40·n algorithmic bytes, the residual kernel's share, and the same step
composed literally from the exported BLAS-1 entry points: scale (d = −σ f), axpy (u += α d), the residual, two norms (‖f‖₂,
‖f‖∞), two differences (δu, δf), two dots, two copies into the caches; the scalars go through the host as those entry points
return them. Fused and composed runs alternate, three times each after a warm-up of each; the minimum is reported.

    python tools/dfsane_bench.py [--out profiles/dfsane_bench.txt] [--log2n 24] [--steps 50]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import nonlinearsolve_jl_amd as nls
from nonlinearsolve_jl_amd import _lib as L

SETTLE = 8


def fused(n, steps, profile):
    prob = nls.NonlinearProblem(nls.Quadratic(n, 2.0), torch.full((n,), 1.3, dtype=torch.float64, device="cuda"))
    cache = nls.init(prob, nls.DFSane(sigma_1=0.4), abstol=1e-300, maxiters=10 ** 6,
                     termination_condition=nls.AbsNormTerminationMode())
    for _ in range(SETTLE):
        nls.step_(cache)
    t_before = cache.dfsane_state["total_trials"]
    assert t_before == SETTLE and not cache.force_stop, (t_before, cache.retcode)
    if profile:
        prob.ctx.profile_enable(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        nls.step_(cache)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    assert cache.nsteps == SETTLE + steps and not cache.force_stop, (cache.nsteps, cache.retcode)
    assert cache.dfsane_state["total_trials"] == t_before + steps, "a timed step needed more than one trial"
    rep = prob.ctx.profile_report() if profile else None
    if profile:
        prob.ctx.profile_enable(False)
    cache.close()
    return ms, rep


def composed(n, steps):
    """the literal step (lib/NonlinearSolveSpectralMethods/src/solve.jl:201-259, α = 1 accepted) from the exported BLAS-1 calls"""
    P = nls.Quadratic(n, 2.0)
    ctx, lib = P.ctx, L.lib()
    dev = dict(dtype=torch.float64, device="cuda")
    u, fu, d, u_cache, fu_cache = (torch.zeros(n, **dev) for _ in range(5))
    u.fill_(1.3)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    axpby = lambda a, x, b, yy: L.check(lib.nk_vec_axpby(ctx._h, n, float(a), ptr(x), float(b), ptr(yy)))
    L.check(lib.nk_residual(P._h, ptr(u), ptr(fu), L.DEVICE))
    axpby(1.0, u, 0.0, u_cache)
    axpby(1.0, fu, 0.0, fu_cache)
    state = dict(sigma=0.4, f1=ctx.nrm2(fu) ** 2)

    def step():
        axpby(-state["sigma"], fu, 0.0, d)                  # d = −σ f
        ctx.axpy(1.0, d, u)                                 # u += α d
        L.check(lib.nk_residual(P._h, ptr(u), ptr(fu), L.DEVICE))
        fn = ctx.nrm2(fu) ** 2                              # the merit (the acceptance test reads it)
        ctx.norm_inf(fu)                                    # the termination check
        axpby(1.0, u, -1.0, u_cache)                        # δu = u − u_cache
        axpby(1.0, fu, -1.0, fu_cache)                      # δf = fu − fu_cache
        sxx, sxf = ctx.dot(u_cache, u_cache), ctx.dot(u_cache, fu_cache)
        s = sxx / sxf if sxf != 0.0 else float("nan")
        if not (1e-10 <= abs(s) <= 1e10):
            s = min(max(1.0 / max(fn, 1e-300) ** 0.5, 1.0), 1e5)
        state["sigma"] = s
        axpby(1.0, u, 0.0, u_cache)                         # the caches
        axpby(1.0, fu, 0.0, fu_cache)

    for _ in range(SETTLE):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    P.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "dfsane_bench.txt"))
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    n = 2 ** args.log2n
    fused(n, 5, False)
    composed(n, 5)
    fs, cs = [], []
    for _ in range(3):
        fs.append(fused(n, args.steps, False)[0])
        cs.append(composed(n, args.steps))
    ms, base = min(fs), min(cs)
    _ms, rep = fused(n, args.steps, True)
    zero = dict(launches=0, avg_us=float("nan"))
    tri, red, res = rep.get("newton_update", zero), rep.get("multidot", zero), rep.get("residual", zero)
    by = 40.0 * n
    both = tri["avg_us"] + red["avg_us"]
    lines = [f"DFSane step, every step accepted at its first trial: Quadratic, n = 2^{args.log2n} = {n}, {args.steps} steps after "
             f"{SETTLE}, {torch.cuda.get_device_name(0)}",
             "launches per fused step: 4 (trial point, residual, reduce pass, publish of three scalars); timed by the library: "
             f"{tri['launches']} trial, {red['launches']} reduce, {res['launches']} residual launches in {args.steps} steps", "",
             f"  fused step            {ms:9.3f} ms/step (wall clock, min of 3 runs: {', '.join('%.3f' % x for x in fs)})",
             f"  trial pass            {tri['avg_us']:9.1f} us  {24.0 * n / (tri['avg_us'] * 1e-6) / 1e12:8.2f} TB/s on {24.0 * n / 1e6:.1f} MB",
             f"  reduce pass           {red['avg_us']:9.1f} us  {16.0 * n / (red['avg_us'] * 1e-6) / 1e12:8.2f} TB/s on {16.0 * n / 1e6:.1f} MB",
             f"  both passes           {both:9.1f} us  {by / (both * 1e-6) / 1e12:8.2f} TB/s on {by / 1e6:.1f} MB (40 n)",
             f"  residual kernel       {res['avg_us']:9.1f} us  ({100.0 * res['avg_us'] / (1e3 * ms):.0f} % of the fused step)",
             f"  composed from BLAS-1  {base:9.3f} ms/step (min of 3 runs: {', '.join('%.3f' % x for x in cs)})",
             f"  fused / composed      {ms / base:9.3f}   (composed / fused {base / ms:.2f}x)", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
