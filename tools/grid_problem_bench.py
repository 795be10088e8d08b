"""The generated kernels of a compiled grid problem (csrc/nk_grid.hip) against the hand-written Bratu kernels, in one process:
the Bratu source of tests/grid_reference.py compiled at 1024² next to Bratu2D(1024).

Kernel times are the kernels' own begin → end device timestamps (the library's per-kernel event timing, which the generated
launches join): one launch per sample, the two problems alternating, the median of `--reps` samples after a warm-up; GB/s on
the algorithmic bytes — residual 16 n, JVP 24 n (the built-in JVP reads a precomputed diagonal where the generated one reads u:
the same 24 n), fill 8 nnz + 8 n. The fill is timed in both of its forms: rows put together in LDS and stored as whole lines
(the default), and every thread storing its own partials (NK_GRID_FILL_DIRECT=1).

Then bench.py's protocol — NewtonRaphson, exactly 30 Arnoldi steps of GMRES(30) per Newton step, nothing terminates — matrix-free
and on the concrete Jacobian, on both problems: `--steps` timed steps after `--warmup`, three runs each, alternating.

    python tools/grid_problem_bench.py [--out profiles/grid_problem_bench.txt] [--grid 1024] [--reps 200] [--steps 300]

`--dim 3` measures the 3-D generated kernels instead (nk_grid3_residual, nk_grid3_jvp, nk_grid3_jac in both forms of the fill):
the bratu3 source of tests/grid3_reference.py at `--grid3`³ (256³ = 16.8 M unknowns), the 27-point box3 source at `--box3`³,
and as the yardstick the 2-D Bratu source at `--grid2`² (4096², the same unknown count) — same process, same protocol, the
problems alternating. Fill bytes are 8 nnz + (8 dof + 4) n: the values, u and the row pointer.

    python tools/grid_problem_bench.py --dim 3 [--out profiles/grid3_problem_bench.txt] [--grid3 256] [--box3 160] [--grid2 4096]

`--radius 2` measures the radius-2 generated kernels beside their radius-1 twins at equal unknowns: the fourth-order Bratu
source lap4 of tests/grid_r2_reference.py (9-point star2) beside the radius-1 compiled Bratu source at `--grid`² (1024²), and
lap4_3 (13-point star2) beside bratu3 at `--grid3`³ (256³) — same process, same protocol, the problems alternating. Residual
and JVP move the same algorithmic bytes in both (16 n, 24 n): a time ratio above 1 is load-path cost. The fill grows with
8 nnz / n and is compared in GB/s.

    python tools/grid_problem_bench.py --radius 2 [--out profiles/grid_r2_problem_bench.txt] [--grid 1024] [--grid3 256]

`--fields` measures what a read-only field costs (nk_problem_create_grid_fields), at `--grid`² (1024²) and at `--grid2`² (4096²,
which does not fit the Infinity Cache): (a) the Bratu source without fields as the yardstick, (b) bratu_f of
tests/gridf_reference.py, one field read at the centre, (c) a source reading one field at all five points, (d) source (b)
compiled with four fields declared — same process, same protocol, the problems alternating. Algorithmic bytes grow by 8 n per
field read (dof = 1). Expected, and nothing is tuned to it: (b)/(a) near the byte ratio (24/16 residual, 32/24 JVP), (c) within
the p10–p90 spread of (b) since the extra reads are cache hits, (d) indistinguishable from (b).

    python tools/grid_problem_bench.py --fields [--out profiles/gridf_problem_bench.txt] [--grid 1024] [--grid2 4096]

`--sides` measures what a boundary kind per side costs (NK_GRID_SIDES), at `--grid`² (1024²): the Bratu source with (a) the
Dirichlet-0 boundary as the yardstick, (b) mirror-node on all four sides, (c) x periodic and y mirror-face — same process, same
protocol, the problems alternating, the fill in both forms. Expected, and nothing is tuned to it: residual and JVP move the
bytes of (a) and cost the same; the fill of (b) and (c) stores slightly fewer or more values than (a) (a mirrored ghost is a
column where the Dirichlet ghost is none, unless it lands on a column the row already has) and adds the merge's integer
compares. The ratios to (a) are printed.

    python tools/grid_problem_bench.py --sides [--out profiles/grid_sides_bench.txt] [--grid 1024]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import grid_reference as R
import nonlinearsolve_jl_amd as nls


def kernel_samples(ctx, calls, reps, warm=20):
    """calls: {label: (callable, profile family)}; per label the sorted per-launch device times in µs"""
    out = {k: [] for k in calls}
    for i in range(warm + reps):
        for label, (fn, family) in calls.items():
            ctx.profile_enable(True)       # (also resets the accumulators)
            fn()
            r = ctx.profile_report()[family]
            if i >= warm:
                out[label].append(1e3 * r["total_ms"])   # (every launch of the family the call made: one)
    ctx.profile_enable(False)
    return {k: sorted(v) for k, v in out.items()}


def steps_per_second(make_problem, u0, concrete, steps, warmup):
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(gmres_restart=30, maxiters=30, fixed_iters=30), concrete_jac=concrete)
    cache = nls.init(nls.NonlinearProblem(make_problem(), u0.clone()), alg, abstol=1e-300, maxiters=10 ** 9)
    for _ in range(warmup):
        cache.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        cache.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fn = cache.fnorm_inf
    cache.close()
    return steps / dt, fn


def main3(args):
    """the 3-D kernels beside the 2-D generated kernels at equal unknowns"""
    import grid3_reference as R3
    g3, b3, g2 = args.grid3, args.box3, args.grid2
    cases = [   # label, source, (nx, ny, nz), stencil, parameters
        (f"2-D bratu {g2}^2", R.BRATU_SRC, (g2, g2, None), "star", R.bratu_params(g2, 6.0)),
        (f"bratu3 {g3}^3", R3.BRATU3_SRC, (g3, g3, g3), "star", R3.bratu3_params(g3, 3.0)),
        (f"box3 {b3}^3", R3.BOX3_SRC, (b3, b3, b3), "box", R3.BOX3_PARAMS),
    ]
    generated_kernels(args, "Compiled grid problems in 3-D beside the 2-D generated kernels at equal unknowns", cases)


def main_radius2(args):
    """the radius-2 kernels beside the radius-1 generated kernels at equal unknowns, in 2-D and in 3-D"""
    import grid3_reference as R3
    import grid_r2_reference as R2
    g, g3 = args.grid, args.grid3
    cases = [
        (f"bratu {g}^2 (5-point)", R.BRATU_SRC, (g, g, None), "star", R.bratu_params(g, 6.0)),
        (f"lap4 {g}^2 (9-point star2)", R2.LAP4_SRC, (g, g, None), "star2", R2.lap4_params(g, 3.0)),
        (f"bratu3 {g3}^3 (7-point)", R3.BRATU3_SRC, (g3, g3, g3), "star", R3.bratu3_params(g3, 3.0)),
        (f"lap4_3 {g3}^3 (13-point star2)", R2.LAP4_3_SRC, (g3, g3, g3), "star2", R2.lap4_params(g3, 3.0)),
    ]
    generated_kernels(args, "Compiled grid problems with a radius-2 stencil beside their radius-1 twins at equal unknowns", cases)


# one field at all five points: Bratu with the source strength averaged over the star
BRATU_F5_SRC = """
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, nk_site s, T *f) {
  const T c = u(0, 0);
  const nk_real w = 0.2 * (a(0, 0) + a(-1, 0) + a(1, 0) + a(0, -1) + a(0, 1));
  f[0] = p[0] * (4.0 * c - u(-1, 0) - u(1, 0) - u(0, -1) - u(0, 1)) - (p[1] * w) * exp(c);
}
"""


def main_fields(args):
    """what a field costs: no field, one read at the centre, one read at five points, four declared and one read"""
    import gridf_reference as RF
    cases = []
    for g in (args.grid, args.grid2):
        par = R.bratu_params(g, 6.0)
        cases += [   # label, source, shape, stencil, parameters, fields declared, fields read
            (f"(a) bratu {g}^2, no field", R.BRATU_SRC, (g, g, None), "star", par, 0, 0),
            (f"(b) bratu_f {g}^2, 1 field at the centre", RF.BRATU_F_SRC, (g, g, None), "star", par, 1, 1),
            (f"(c) bratu_f5 {g}^2, 1 field at 5 points", BRATU_F5_SRC, (g, g, None), "star", par, 1, 1),
            (f"(d) bratu_f {g}^2, 4 declared, 1 read", RF.BRATU_F_SRC, (g, g, None), "star", par, 4, 1),
        ]
    generated_kernels(args, "Compiled grid problems with read-only fields beside the same problem without", cases, direct=False)


def main_sides(args):
    """what a kind per side costs: Dirichlet-0, mirror-node all round, x periodic with y mirror-face"""
    g = args.grid
    par = R.bratu_params(g, 6.0)
    cases = [(f"(a) bratu {g}^2, Dirichlet-0", R.BRATU_SRC, (g, g, None), "star", par),
             (f"(b) bratu {g}^2, mirror-node all round", R.BRATU_SRC, (g, g, None), "star", par),
             (f"(c) bratu {g}^2, x periodic, y mirror-face", R.BRATU_SRC, (g, g, None), "star", par)]
    boundaries = {cases[0][0]: "dirichlet", cases[1][0]: ("mirror_node",) * 4,
                  cases[2][0]: {"x": "periodic", "y": "mirror_face"}}
    generated_kernels(args, "Compiled grid problems with a boundary kind per side beside the Dirichlet-0 form", cases,
                      boundaries=boundaries)


def generated_kernels(args, title, cases, direct=True, boundaries=None):
    """the three generated kernels of every case, the fill in both forms (direct = False: the default form only), ordered by
    kernel so that the cases alternate. A case may end with (fields declared, fields read): the fields hold seeded positive
    data, and every kernel's algorithmic bytes grow by 8 n per field read. boundaries: label → boundary= of the case (the
    default: "dirichlet"); with it the time ratios of the cases (b), (c) to (a) are printed."""
    ctx = nls.default_context()
    gen = torch.Generator(device="cuda").manual_seed(1)
    calls, meta, problems, sizes = {}, {}, [], []   # meta: label → (kind rank, algorithmic bytes, unknowns)
    for label, src, (nx, ny, nz), stencil, par, *fld in cases:
        nf, nread = fld if fld else (0, 0)

        def create():
            P = nls.CompiledGridProblem(src, nx, ny, stencil=stencil, params=par, nz=nz, fields=nf,
                                        boundary=(boundaries or {}).get(label, "dirichlet"))
            for k in range(nf):
                P.set_field(k, 0.5 + torch.rand(P.nn, dtype=torch.float64, device="cuda", generator=gen))
            return P
        P = create()
        Pd = P
        if direct:
            os.environ["NK_GRID_FILL_DIRECT"] = "1"
            Pd = create()
            del os.environ["NK_GRID_FILL_DIRECT"]
        n = P.n_local
        u = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 1.0
        v = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 1.0
        J, Jd = P.jac_csr(), Pd.jac_csr()
        nnz = J.info()["nnz"]
        # the fill agrees with the dual JVP, and its two forms with each other, before anything is timed
        P.jac_values(u, J)
        Pd.jac_values(u, Jd)
        jv = P.jvp(v, u)
        assert float((J.matvec(v) - jv).abs().max()) <= 1e-10 * max(1.0, float(jv.abs().max()))
        assert torch.equal(J.matvec(v), Jd.matvec(v))
        sizes.append(f"{label}: n = {n}, nnz = {nnz} ({nnz / n:.2f} per row)")
        print("built and checked " + sizes[-1], flush=True)
        fb = 8.0 * nread * (n // P.dof)   # a field read once per node
        kinds = [("residual", lambda P=P, u=u: P.residual(u), "residual", 16.0 * n + fb),
                 ("JVP", lambda P=P, u=u, v=v: P.jvp(v, u), "jvp", 24.0 * n + fb),
                 ("fill (LDS-staged rows)", lambda P=P, u=u, J=J: P.jac_values(u, J), "jacfill", 8.0 * nnz + 12.0 * n + fb),
                 ("fill (direct stores)", lambda Pd=Pd, u=u, Jd=Jd: Pd.jac_values(u, Jd), "jacfill", 8.0 * nnz + 12.0 * n + fb)]
        if not direct:
            kinds.pop()
        for what, fn, fam, b in kinds:
            calls[f"{what:24s} {label}"] = (fn, fam)
            meta[f"{what:24s} {label}"] = (("res", "JVP", "fill (L", "fill (d").index(what[:7] if what[:4] == "fill" else what[:3]), b, n)
        problems += [P, Pd] if direct else [P]
    # (ordered by kernel, so that the 2-D yardstick and the 3-D kernels of one kind alternate)
    order = sorted(calls, key=lambda k: meta[k][0])
    ts = kernel_samples(ctx, {k: calls[k] for k in order}, args.reps)
    lines = [f"{title}, {torch.cuda.get_device_name(0)}"] + sizes + [
             f"kernel begin -> end device timestamps, one launch per sample, problems alternating, {args.reps} samples after 20;",
             "GB/s on algorithmic bytes: residual 16 n, JVP 24 n, fill 8 nnz + 12 n (dof = 1)" +
             (", each + 8 n per field read" if any(len(c) > 5 for c in cases) else ""), "",
             f"  {'kernel':56s} {'median us':>10s} {'p10':>9s} {'p90':>9s} {'GB/s (median)':>14s}  {'ns/unknown':>10s}  algorithmic MB"]
    for label in order:
        t = ts[label]
        med = statistics.median(t)
        _rank, b, n = meta[label]
        lines.append(f"  {label:56s} {med:10.2f} {t[len(t) // 10]:9.2f} {t[(9 * len(t)) // 10]:9.2f} "
                     f"{b / med / 1e3:14.1f}  {1e3 * med / n:10.4f}  {b / 1e6:.1f}")
    if any(len(c) > 5 for c in cases):   # the fields protocol: time ratios between the cases (a) … (d) of one size
        lines += ["", "time ratios of the medians (expected: (b)/(a) near the byte ratio 24/16 residual, 32/24 JVP; (c)/(b) and (d)/(b) near 1)"]
        med = {k: statistics.median(ts[k]) for k in order}
        for what in ("residual", "JVP", "fill (LDS-staged rows)"):
            for size in sorted({c[2][0] for c in cases}):
                m = {c[0][:3]: med[f"{what:24s} {c[0]}"] for c in cases if c[2][0] == size}
                lines.append(f"  {what:24s} {size}^2: (b)/(a) {m['(b)'] / m['(a)']:.3f}   (c)/(b) {m['(c)'] / m['(b)']:.3f}   "
                             f"(d)/(b) {m['(d)'] / m['(b)']:.3f}")
    if boundaries:   # the sides protocol: time ratios of (b) and (c) to the Dirichlet-0 form (a), with (a)'s own spread
        lines += ["", "time ratios of the medians to (a), and (a)'s own spread (p90 - p10) / median (expected: residual and JVP near 1; "
                  "the fill near its byte ratio)"]
        med = {k: statistics.median(ts[k]) for k in order}
        for what in ("residual", "JVP", "fill (LDS-staged rows)", "fill (direct stores)"):
            m = {c[0][:3]: f"{what:24s} {c[0]}" for c in cases}
            ta = ts[m["(a)"]]
            lines.append(f"  {what:24s} (b)/(a) {med[m['(b)']] / med[m['(a)']]:.3f}   (c)/(a) {med[m['(c)']] / med[m['(a)']]:.3f}   "
                         f"spread of (a) {(ta[(9 * len(ta)) // 10] - ta[len(ta) // 10]) / med[m['(a)']]:.3f}   "
                         f"bytes (b)/(a) {meta[m['(b)']][1] / meta[m['(a)']][1]:.3f}   (c)/(a) {meta[m['(c)']][1] / meta[m['(a)']][1]:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for PP in problems:
        PP.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dim", type=int, default=2, choices=(2, 3))
    ap.add_argument("--radius", type=int, default=1, choices=(1, 2))
    ap.add_argument("--fields", action="store_true")
    ap.add_argument("--sides", action="store_true")
    ap.add_argument("--grid3", type=int, default=256)
    ap.add_argument("--box3", type=int, default=160)
    ap.add_argument("--grid2", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if args.out is None:
        name = "grid_r2_problem_bench.txt" if args.radius == 2 else ("grid3_problem_bench.txt" if args.dim == 3 else "grid_problem_bench.txt")
        name = "gridf_problem_bench.txt" if args.fields else ("grid_sides_bench.txt" if args.sides else name)
        args.out = os.path.join(ROOT, "profiles", name)
    if args.sides:
        return main_sides(args)
    if args.fields:
        return main_fields(args)
    if args.radius == 2:
        return main_radius2(args)
    if args.dim == 3:
        return main3(args)
    ns = args.grid
    n, nnz = ns * ns, 5 * ns * ns - 4 * ns
    ctx = nls.default_context()
    par = R.bratu_params(ns, 6.0)
    B = nls.Bratu2D(ns, 6.0)
    P = nls.CompiledGridProblem(R.BRATU_SRC, ns, ns, params=par)
    os.environ["NK_GRID_FILL_DIRECT"] = "1"
    Pd = nls.CompiledGridProblem(R.BRATU_SRC, ns, ns, params=par)
    del os.environ["NK_GRID_FILL_DIRECT"]
    g = torch.Generator(device="cuda").manual_seed(1)
    u = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 1.0
    v = 2.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 1.0
    JB, JP, JPd = B.jac_csr(), P.jac_csr(), Pd.jac_csr()
    # the two problems compute the same numbers before anything is timed
    assert float((P.residual(u) - B.residual(u)).abs().max()) <= 1e-12
    assert float((P.jvp(v, u) - B.jvp(v, u)).abs().max()) <= 1e-12
    for PP, JJ in ((B, JB), (P, JP), (Pd, JPd)):
        PP.jac_values(u, JJ)
    assert float((JP.matvec(v) - JB.matvec(v)).abs().max()) <= 1e-12 and torch.equal(JP.matvec(v), JPd.matvec(v))
    calls = {
        "residual built-in  k_bratu_residual": (lambda: B.residual(u), "residual"),
        "residual generated nk_grid_residual": (lambda: P.residual(u), "residual"),
        "JVP      built-in  k_bratu_jvp_tile": (lambda: B.jvp(v, u), "jvp"),
        "JVP      generated nk_grid_jvp": (lambda: P.jvp(v, u), "jvp"),
        "fill     built-in  k_bratu_jac": (lambda: B.jac_values(u, JB), "jacfill"),
        "fill     generated nk_grid_jac (LDS-staged rows)": (lambda: P.jac_values(u, JP), "jacfill"),
        "fill     generated nk_grid_jac (direct stores)": (lambda: Pd.jac_values(u, JPd), "jacfill"),
    }
    bytes_of = {"residual": 16.0 * n, "jvp": 24.0 * n, "jacfill": 8.0 * nnz + 8.0 * n}
    ts = kernel_samples(ctx, calls, args.reps)
    lines = [f"Compiled grid problem against the built-in Bratu kernels: {ns} x {ns}, n = {n}, nnz = {nnz}, "
             f"{torch.cuda.get_device_name(0)}",
             f"kernel begin -> end device timestamps, one launch per sample, problems alternating, {args.reps} samples after 20", "",
             f"  {'kernel':52s} {'median us':>10s} {'p10':>8s} {'p90':>8s} {'GB/s (median)':>14s}  algorithmic MB"]
    for label, (_fn, fam) in calls.items():
        t = ts[label]
        med = statistics.median(t)
        lines.append(f"  {label:52s} {med:10.2f} {t[len(t) // 10]:8.2f} {t[(9 * len(t)) // 10]:8.2f} "
                     f"{bytes_of[fam] / med / 1e3:14.1f}  {bytes_of[fam] / 1e6:.1f}")
    lines += ["", f"Newton steps/s, bench.py's fixed-work protocol (30 Arnoldi steps of GMRES(30) per step), {args.steps} steps after "
              f"{args.warmup}, three runs each, alternating:"]
    u0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    for concrete, what in ((False, "matrix-free (JVP operator)"), (True, "concrete Jacobian (fill + CSR SpMV)")):
        rb, rp = [], []
        for _ in range(3):
            sb, fb = steps_per_second(lambda: B, u0, concrete, args.steps, args.warmup)
            sp, fp = steps_per_second(lambda: P, u0, concrete, args.steps, args.warmup)
            rb.append(sb)
            rp.append(sp)
        lines += [f"  {what}",
                  f"    built-in Bratu2D      median {statistics.median(rb):9.1f} steps/s  (runs: {', '.join('%.1f' % x for x in rb)}; |f|inf after {fb:.3e})",
                  f"    compiled Bratu source median {statistics.median(rp):9.1f} steps/s  (runs: {', '.join('%.1f' % x for x in rp)}; |f|inf after {fp:.3e})",
                  f"    compiled / built-in   {statistics.median(rp) / statistics.median(rb):9.3f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for PP in (B, P, Pd):
        PP.close()


if __name__ == "__main__":
    main()
