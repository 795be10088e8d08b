"""The geometric multigrid `precs` of compiled grid problems (csrc/nk_gridmg.hip) measured: Bratu as a compiled source and the
variable-coefficient channel problem (tests/gridmg_reference.py, cases (a) and (b)) at `--grid`² (1024²), one GPU.

Per problem:
  * the time of NewtonRaphson + GMRES(30) to ‖h²F‖∞ <= 1e-8 with MultigridPrecs(2, coarse_max) for every coarse_max of `--sweep`
    (0 = the library's default), the median of `--reps` solves after one warm-up solve — every solve builds its hierarchy —
    and the same solve repeated on one cache (reinit_ + solve_), where the hierarchy exists and is only updated;
  * the same solve with the aggregation AMG `precs` object on the concrete Jacobian, same commit, same process;
  * set-up (first nk_gmres_set_multigrid_preconditioner: hierarchy + update) and update (every later call) on their own;
  * µs per V-cycle — (a solve of exactly 30 Arnoldi steps with the V-cycle − the same without preconditioner) / 31 applications —
    and per smoothing step on all levels — (V-cycle with ν = 3 − V-cycle with ν = 2) / 2 — against the algorithmic bytes of
    csrc/nk_gridmg.hip's header (a smoothing step: 12 nnz + 52 n per level).
The ceiling is the built-in Bratu2D problem with its own V-cycle (stencil kernels, no matrix), same λ, same tolerance.
No ratio is fixed in advance; nothing here asserts a time. The two sources, their fields and their spacings are the test tree's
(tests/gridmg_reference.py, put on sys.path below): the tool measures exactly the problems the tests check.

    python tools/grid_mg_bench.py [--grid 1024] [--reps 5] [--sweep 0,4,8,16,31] [--out profiles/grid_mg_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gridmg_reference as GM
import nonlinearsolve_jl_amd as nls

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def make(prob, n, params):
    P = nls.CompiledGridProblem(prob.source, n, n, dof=prob.dof, stencil=prob.stencil, boundary=prob.boundary, params=params,
                                fields=prob.nfields)
    if prob.nfields:
        f = prob.fields((n, n))
        for k in range(prob.nfields):
            P.set_field(k, np.ascontiguousarray(f[k * n * n:(k + 1) * n * n]))
    return P


def newton_time(P, precs, abstol, reps, concrete=False):
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(gmres_restart=30, maxiters=300, precs=precs), concrete_jac=concrete)
    ts, sol = [], None
    for rep in range(reps + 1):
        prob = nls.NonlinearProblem(P, u0=P.initial_guess(device=True))
        dt, sol = timed(lambda: nls.solve(prob, alg, abstol=abstol, maxiters=50))
        if rep:
            ts.append(dt)
    return statistics.median(ts), sol


def resolve_time(P, precs, abstol, reps):
    """the same solve again on one cache (reinit_ + solve_): the hierarchy exists, every new Jacobian only updates it — what a
    step of an implicit time integration pays"""
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(gmres_restart=30, maxiters=300, precs=precs))
    u0 = P.initial_guess(device=True)
    cache = nls.init(nls.NonlinearProblem(P, u0=u0.clone()), alg, abstol=abstol, maxiters=50)
    nls.solve_(cache)
    ts = []
    for _ in range(reps):
        nls.reinit_(cache, u0=u0.clone())
        ts.append(timed(lambda: nls.solve_(cache))[0])
    cache.close()
    return statistics.median(ts)


def cycle_times(P, n_unknowns, u, cm):
    """(set-up s, update s, µs per V-cycle at ν = 2, µs per smoothing step on all levels, levels)"""
    op = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), u)
    b = torch.randn(n_unknowns, dtype=torch.float64, device=u.device)

    def solve30(G):
        G.solve(b, fixed_iters=30)                                   # warm-up
        return statistics.median(timed(lambda: G.solve(b, fixed_iters=30))[0] for _ in range(5))
    G0 = nls.GMRES(n_unknowns, restart=30).set_operator(op)
    plain = solve30(G0)
    G0.close()
    out = {}
    for nu in (2, 3):
        G = nls.GMRES(n_unknowns, restart=30).set_operator(op)
        setup, _ = timed(lambda: G.set_multigrid_preconditioner(P, u, nu=nu, coarse_max=cm))
        update = statistics.median(timed(lambda: G.set_multigrid_preconditioner(P, u, nu=nu, coarse_max=cm))[0] for _ in range(5))
        out[nu] = (setup, update, (solve30(G) - plain) / 31.0, G.multigrid_levels())
        G.close()
    return out[2][0], out[2][1], 1e6 * out[2][2], 1e6 * (out[3][2] - out[2][2]) / 2.0, out[2][3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="0,4,8,16,31", help="coarse_max values; 0 = the library's default")
    ap.add_argument("--lam", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.grid
    sweep = [int(x) for x in args.sweep.split(",")]
    say(f"Multigrid precs of compiled grid problems at {n}^2 on {torch.cuda.get_device_name(0)}")
    for name, params in (("bratu", [args.lam]), ("channel", None)):
        prob = GM.PROBLEMS[name]
        params = prob.params if params is None else params
        P = make(prob, n, params)
        h = min(GM.spacing((n, n), prob.boundary))
        abstol = 1e-8 / (h * h)
        say(f"\n== {name}: {prob.__doc__.split(':')[0].strip()}; tolerance ‖F‖∞ <= 1e-8/h² = {abstol:.3e}")
        for cm in sweep:
            t, sol = newton_time(P, nls.MultigridPrecs(2, cm), abstol, args.reps)
            say(f"  MultigridPrecs(2, {cm:2d}): {1e3 * t:8.2f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} "
                f"Krylov iterations")
        say(f"  MultigridPrecs(2,  0) on an existing cache (reinit_ + solve_): {1e3 * resolve_time(P, nls.MultigridPrecs(2, 0), abstol, args.reps):8.2f} ms")
        t, sol = newton_time(P, nls.ObjectPrecs("amg", "right"), abstol, args.reps, concrete=True)
        say(f"  AMG precs object      : {1e3 * t:8.2f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} Krylov "
            f"iterations")
        u = sol.u if torch.is_tensor(sol.u) else torch.as_tensor(np.asarray(sol.u), device="cuda:0")
        for cm in (0, 31):
            setup, update, vc, sm, lv = cycle_times(P, prob.dof * n * n, u, cm)
            nnz_all, n_all = sum(x["nnz"] for x in lv[:-1]), sum(x["n"] for x in lv[:-1])
            sm_bytes = 12.0 * nnz_all + 52.0 * n_all
            # ν = 2: per smoothed level 3 steps with a row product, one without (32 n), one residual (12 nnz + 28 n), plus the
            # transfers (≈ 8 n_f + 8 n_c each way, x read and written once more by the prolongation)
            vc_bytes = 3.0 * sm_bytes + 32.0 * n_all + (12.0 * nnz_all + 28.0 * n_all) + 36.0 * n_all
            say(f"  coarse_max {cm:2d}: {len(lv)} levels, coarsest {lv[-1]['sides']}; set-up {1e3 * setup:.2f} ms, update "
                f"{1e3 * update:.2f} ms; V-cycle {vc:.0f} µs for {vc_bytes / 1e6:.1f} MB ({vc_bytes / vc / 1e3:.0f} GB/s); smoothing "
                f"step on all levels {sm:.0f} µs for {sm_bytes / 1e6:.1f} MB ({sm_bytes / sm / 1e3:.0f} GB/s)")
        P.close()
    B = nls.Bratu2D(n, args.lam)
    for cm in (0, 31):
        t, sol = newton_time(B, nls.MultigridPrecs(2, cm), 1e-8, args.reps)
        say(f"\n== built-in Bratu2D, MultigridPrecs(2, {cm}): {1e3 * t:8.2f} ms  {sol.retcode}, {sol.stats.nsteps} steps, "
            f"{sol.stats.gmres_iters} Krylov iterations (the ceiling)")
        say(f"   on an existing cache (reinit_ + solve_): {1e3 * resolve_time(B, nls.MultigridPrecs(2, cm), 1e-8, args.reps):8.2f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
