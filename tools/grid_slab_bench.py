"""What the slab programs of a compiled grid problem on several ranks cost (csrc/nk_grid.hip, "several ranks"): two processes
share one GPU (callback transport over gloo, as in tests/test_gpu_multirank.py); each builds the Bratu source of
tests/grid_reference.py on the 2-rank context at `--grid`² (1024²: slabs of 1024 × 512) and the bratu3 source of
tests/grid3_reference.py at `--grid3`³ (128³: slabs of 128 × 128 × 64), and beside each, on a communicator-free Context in the
same process, the one-rank program on a grid of the slab's own size. Rank 0 reports.

Kernel times only: the kernels' own begin → end device timestamps from the context profile (the generated launches join it), one
launch per sample, the slab problem and its one-rank twin alternating, the median of `--reps` samples after a warm-up. Both
ranks run the same loop and meet at a barrier before every timed call — a slab call is collective, so the two ranks' slab
kernels always run at the same time; the barrier makes the one-rank twins do so too, and the GPU is shared alike in both halves
of a pair. The exchange is not in these figures, and its time on a shared GPU says nothing about xGMI: it is not reported.

    python tools/grid_slab_bench.py [--out profiles/grid_slab_bench.txt] [--grid 1024] [--grid3 128] [--reps 200]
"""
import argparse
import os
import socket
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _worker(rank, world, port, q, args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import grid3_reference as R3
        import grid_reference as R
        import nonlinearsolve_jl_amd as nls
        torch.cuda.set_device(0)
        ctx = nls.Context(device=0)
        nls.set_default_context(ctx)
        nls.dist.init_comm(ctx, "torch")
        one = nls.Context(device=0)
        gen = torch.Generator(device="cuda").manual_seed(1 + rank)
        g, g3 = args.grid, args.grid3
        cases = [(f"bratu {g}^2", R.BRATU_SRC, (g, g, None), R.bratu_params(g, 6.0)),
                 (f"bratu3 {g3}^3", R3.BRATU3_SRC, (g3, g3, g3), R3.bratu3_params(g3, 3.0))]
        lines = [f"Slab programs of compiled grid problems on 2 ranks sharing one {torch.cuda.get_device_name(0)}, rank 0's kernels",
                 f"kernel begin -> end device timestamps, one launch per sample, slab and one-rank twin alternating, {args.reps} "
                 "samples after 20; the one-rank twin is the one-rank program on a grid of the slab's own size", "",
                 f"  {'kernel':44s} {'slab median us':>15s} {'p10':>8s} {'p90':>8s} {'one-rank median us':>19s} {'p10':>8s} {'p90':>8s} "
                 f"{'ratio':>7s}  spread of one-rank (p90 - p10) / median"]
        for label, src, (nx, ny, nz), par in cases:
            Pm = nls.CompiledGridProblem(src, nx, ny, params=par, nz=nz, ctx=ctx)
            l0, l1 = Pm.lines
            shape1 = (nx, l1 - l0, None) if nz is None else (nx, ny, l1 - l0)
            P1 = nls.CompiledGridProblem(src, shape1[0], shape1[1], params=par, nz=shape1[2], ctx=one)
            n = Pm.n_local
            assert P1.n_local == n
            u = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 1.0
            v = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 1.0
            Jm, J1 = Pm.jac_csr(), P1.jac_csr()
            kinds = [("residual", "residual", lambda P, J: P.residual(u)), ("JVP", "jvp", lambda P, J: P.jvp(v, u)),
                     ("fill (LDS-staged rows)", "jacfill", lambda P, J: P.jac_values(u, J))]
            for what, family, call in kinds:
                samples = {"slab": [], "one": []}
                for i in range(20 + args.reps):
                    for key, c, P, J in (("slab", ctx, Pm, Jm), ("one", one, P1, J1)):
                        torch.cuda.synchronize()
                        dist.barrier()             # both halves start in step on both ranks: the GPU is shared alike
                        c.profile_enable(True)
                        call(P, J)
                        t = 1e3 * c.profile_report()[family]["total_ms"]
                        if i >= 20:
                            samples[key].append(t)
                ctx.profile_enable(False)
                one.profile_enable(False)
                s, o = sorted(samples["slab"]), sorted(samples["one"])
                ms, mo = statistics.median(s), statistics.median(o)
                p = lambda t, f: t[(f * len(t)) // 10]
                lines.append(f"  {what + ' ' + label + f' (n_local {n})':44s} {ms:15.2f} {p(s, 1):8.2f} {p(s, 9):8.2f} {mo:19.2f} "
                             f"{p(o, 1):8.2f} {p(o, 9):8.2f} {ms / mo:7.3f}  {(p(o, 9) - p(o, 1)) / mo:.3f}")
            Pm.close()
            P1.close()
        q.put((rank, "ok", "\n".join(lines) + "\n"))
    except Exception:
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), ""))
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/grid_slab_bench.txt")
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--grid3", type=int, default=128)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, 2, port, q, args)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=550) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res
    print(res[0][2])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(res[0][2])
    return 0


if __name__ == "__main__":
    sys.exit(main())
