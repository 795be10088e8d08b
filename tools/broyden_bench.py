"""Step time of good Broyden's dense inverse Jacobian (csrc/nk_qn.hip, nk_solver.hip: qn_step) on Quadratic at n = 4096, 8192 and
16384. With AbsNormTerminationMode at abstol 1e-300 and max_resets out of reach the solve never terminates, so every timed step does
the full work whatever the numbers are: the vector launch, the residual, the reduce launch, one fetch of six scalars, pass A (one
read of J⁻¹), the fold of the partial column sums, pass B (one read and one write).

Reported per size: the device time of each pass (the library's per-kernel event timing: each launch carries its own begin/end
timestamps), as the MEDIAN over the timed steps, one profile window per step; TB/s on the bytes the design says the pass moves
(8n² + 8n²/32, 8n²/32, 16n²) and the fraction of the 6.29 TB/s achievable HBM rate; the wall-clock time per step; and the
launch count per step.

    python tools/broyden_bench.py [--out profiles/broyden_bench.txt] [--sizes 4096 8192 16384] [--steps 24]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import nonlinearsolve_jl_amd as nls

SETTLE = 4
ACHIEVABLE = 6.29e12
PASSES = [("pass A (read)", "multidot", lambda n: 8.0 * n * n * (1.0 + 1.0 / 32)), ("fold of z", "reduce_small", lambda n: 8.0 * n * n / 32),
          ("pass B (read+write)", "multiaxpy", lambda n: 16.0 * n * n)]
VECTORS = [("vector launch", "newton_update"), ("reduce launch", "other"), ("residual", "residual")]


def measure(n, steps):
    u0 = torch.linspace(1.0, 2.375, n, dtype=torch.float64, device="cuda")
    prob = nls.NonlinearProblem(nls.Quadratic(n, 2.0), u0)
    cache = nls.init(prob, nls.Broyden(max_resets=10 ** 9), abstol=1e-300, maxiters=10 ** 6,
                     termination_condition=nls.AbsNormTerminationMode())
    for _ in range(SETTLE):
        nls.step_(cache)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        nls.step_(cache)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0) / steps
    per, launches = {}, []
    for _ in range(steps):
        prob.ctx.profile_enable(True)
        nls.step_(cache)
        torch.cuda.synchronize()
        rep = prob.ctx.profile_report()
        prob.ctx.profile_enable(False)
        launches.append(sum(r["launches"] for r in rep.values()))
        for k, r in rep.items():
            per.setdefault(k, []).append(r["avg_us"] * r["launches"])
    assert not cache.force_stop and cache.nsteps == SETTLE + 2 * steps, (cache.retcode, cache.nsteps)
    resets = cache.qn_state["nresets"]
    cache.close()
    return wall, {k: statistics.median(v) for k, v in per.items()}, statistics.median(launches), resets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "broyden_bench.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192, 16384])
    ap.add_argument("--steps", type=int, default=24)
    args = ap.parse_args()
    assert args.steps >= 20
    lines = [f"good Broyden, dense J⁻¹: Quadratic, median of {args.steps} steps after {SETTLE}, {torch.cuda.get_device_name(0)}", ""]
    for n in args.sizes:
        wall, med, launches, resets = measure(n, args.steps)
        lines.append(f"n = {n}: J⁻¹ {8.0 * n * n / 2 ** 20:.0f} MiB, {launches:.0f} launches per step, {wall:.3f} ms/step wall clock"
                     f" ({resets} resets in the run: a reset step replaces the vector launch's source by one write-only fill)")
        tot_us, tot_b = 0.0, 0.0
        for label, key, by in PASSES:
            us = med.get(key, float("nan"))
            tot_us, tot_b = tot_us + us, tot_b + by(n)
            rate = by(n) / (us * 1e-6)
            lines.append(f"  {label:22s}{us:10.1f} us  {rate / 1e12:6.2f} TB/s on {by(n) / 1e6:9.1f} MB  {rate / ACHIEVABLE:5.2f} of achievable")
        rate = tot_b / (tot_us * 1e-6)
        lines.append(f"  {'the three passes':22s}{tot_us:10.1f} us  {rate / 1e12:6.2f} TB/s on {tot_b / 1e6:9.1f} MB  {rate / ACHIEVABLE:5.2f} of achievable")
        for label, key in VECTORS:
            lines.append(f"  {label:22s}{med.get(key, float('nan')):10.1f} us")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
