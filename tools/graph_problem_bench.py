"""The generated kernels of a compiled graph problem (csrc/nk_graph.hip) beside the compiled GRID problem, in one process, on
three inputs of `--grid`² nodes (1024²):

    (a) the 5-point Bratu problem written as a graph (every node's edges are its grid neighbours, no data),
    (b) a triangulated mesh — the grid's 4 neighbours plus one random diagonal per cell — in natural order, with the `sink`
        source of tests/graph_reference.py (one edge datum, two node data),
    (c) the same mesh and data with the nodes renumbered by a random permutation,

each against CompiledGridProblem with the Bratu source of tests/grid_reference.py at the same size.

Kernel times are the kernels' own begin → end device timestamps (the library's per-kernel event timing, which the generated
launches join): one launch per sample, the problems alternating, the median of `--reps` samples after a warm-up; GB/s on the
algorithmic bytes — per node 16·dof + 4 + deg·(4 + 8·r_e) + 8·r_n for the residual (r_e, r_n the data arrays the source reads),
8·dof more for the JVP, and for the fill the residual's reads plus 4 (slot → node) + 8·dof² per slot. The fill is timed in both
of its forms: one slot per thread (the default) and one node per thread with an inner slot loop (NK_GRAPH_FILL_NODE=1).

Then the time to ‖F‖∞ <= 1e-8 from u = 0 — NewtonRaphson on the concrete Jacobian, GMRES with the aggregation AMG `precs` on the
right — for the three graph problems and the grid problem: the median wall time of `--solves` solves after one warm-up solve.

    python tools/graph_problem_bench.py [--out profiles/graph_problem_bench.txt] [--grid 1024] [--reps 100] [--solves 3]
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

import graph_reference as GR
import grid_reference as R
import nonlinearsolve_jl_amd as nls
from grid_problem_bench import kernel_samples

BRATU_GRAPH_SRC = """
template <typename T>
__device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f) {
  const T c = u.self();
  T acc = T(0.0);
  for (int e = 0; e < u.deg(); ++e) acc = acc + u.nbr(e);
  f[0] = p[0] * (4.0 * c - acc) - p[1] * exp(c);
}
"""


def mesh(nx, ny, diagonals, perm=None, seed=1):
    """CSR adjacency (rowptr, colind int32) of the nx × ny grid's 4 neighbours, plus one random diagonal per cell"""
    idx = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    a = [idx[:, :-1].ravel(), idx[:-1, :].ravel()]
    b = [idx[:, 1:].ravel(), idx[1:, :].ravel()]
    if diagonals:
        main = np.random.default_rng(seed).integers(2, size=(ny - 1, nx - 1)).astype(bool)
        a.append(np.where(main, idx[:-1, :-1], idx[:-1, 1:]).ravel())
        b.append(np.where(main, idx[1:, 1:], idx[1:, :-1]).ravel())
    a, b = np.concatenate(a), np.concatenate(b)
    if perm is not None:
        a, b = perm[a], perm[b]
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((dst, src))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nx * ny))])
    return rowptr.astype(np.int32), dst[order].astype(np.int32), src[order]


def solve_time(make_problem, n, solves):
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True)
    times, sol = [], None
    for k in range(solves + 1):
        u0 = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = nls.solve(nls.NonlinearProblem(make_problem(), u0), alg, abstol=1e-8, maxiters=60)
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), sol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_problem_bench.txt"))
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--solves", type=int, default=3)
    args = ap.parse_args()
    ns = args.grid
    nn = ns * ns
    ctx = nls.default_context()
    par = R.bratu_params(ns, 6.0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    v = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    rng = np.random.default_rng(2)
    perm = rng.permutation(nn)
    sink = GR.PROBLEMS["sink"]

    def graph_problem(src, rp, ci, params, data=None):
        made = []
        for node_form in (False, True):
            if node_form:
                os.environ["NK_GRAPH_FILL_NODE"] = "1"
            P = nls.CompiledGraphProblem(src, rp, ci, params=params, edge_data=1 if data else 0, node_data=2 if data else 0)
            os.environ.pop("NK_GRAPH_FILL_NODE", None)
            if data:
                P.set_edge_data(0, data[0])
                P.set_node_data(0, data[1])
                P.set_node_data(1, data[2])
            made.append(P)
        return made

    G = nls.CompiledGridProblem(R.BRATU_SRC, ns, ns, params=par)
    cases = {}   # label → (slot-form problem, node-form problem, u, v, ne, r_e, r_n)
    rp, ci, _ = mesh(ns, ns, False)
    cases["(a) bratu as a graph"] = (*graph_problem(BRATU_GRAPH_SRC, rp, ci, par), u, v, ci.size, 0, 0)
    rp, ci, src = mesh(ns, ns, True)
    w_pair = rng.uniform(0.5, 1.5, nn)   # w of edge (i, j) from the two nodes: the same in both directions
    kappa, mass = rng.uniform(0.05, 0.15, nn), rng.uniform(0.5, 1.0, nn)
    cases["(b) triangulation, natural"] = (*graph_problem(sink.source, rp, ci, sink.params, (0.5 * (w_pair[src] + w_pair[ci]), kappa, mass)),
                                           u, v, ci.size, 1, 2)
    rp, ci, src = mesh(ns, ns, True, perm)
    inv = np.argsort(perm)   # node perm[m] of (c) is node m of (b): the same mesh, data and vectors, renumbered
    dev_inv = torch.as_tensor(inv, device="cuda")
    kc, mc = np.empty(nn), np.empty(nn)
    kc[perm], mc[perm] = kappa, mass
    cases["(c) triangulation, permuted"] = (*graph_problem(sink.source, rp, ci, sink.params,
                                                           (0.5 * (w_pair[inv[src]] + w_pair[inv[ci]]), kc, mc)),
                                            u[dev_inv], v[dev_inv], ci.size, 1, 2)
    # the numbers before anything is timed: (a) is the grid problem; (c) is (b) renumbered; the two fills agree bit for bit
    Pa = cases["(a) bratu as a graph"][0]
    assert float((Pa.residual(u) - G.residual(u)).abs().max()) <= 1e-12 and float((Pa.jvp(v, u) - G.jvp(v, u)).abs().max()) <= 1e-12
    fb = cases["(b) triangulation, natural"][0].residual(u)
    fc = cases["(c) triangulation, permuted"][0].residual(u[dev_inv])
    assert float((fc - fb[dev_inv]).abs().max()) <= 1e-12
    calls, meta, sizes = {}, {}, []
    JG = G.jac_csr()
    grid_nnz = JG.info()["nnz"]
    calls["residual grid  nk_grid_residual"] = (lambda: G.residual(u), "residual")
    calls["JVP      grid  nk_grid_jvp"] = (lambda: G.jvp(v, u), "jvp")
    calls["fill     grid  nk_grid_jac"] = (lambda: G.jac_values(u, JG), "jacfill")
    meta["residual grid  nk_grid_residual"], meta["JVP      grid  nk_grid_jvp"] = 16.0 * nn, 24.0 * nn
    meta["fill     grid  nk_grid_jac"] = 8.0 * grid_nnz + 12.0 * nn
    for label, (P, Pn, uu, vv, ne, r_e, r_n) in cases.items():
        J, Jn = P.jac_csr(), Pn.jac_csr()
        P.jac_values(uu, J)
        Pn.jac_values(uu, Jn)
        jv = P.jvp(vv, uu)
        assert float((J.matvec(vv) - jv).abs().max()) <= 1e-10 * max(1.0, float(jv.abs().max()))
        assert torch.equal(J.matvec(vv), Jn.matvec(vv))
        res = 20.0 * nn + ne * (4.0 + 8.0 * r_e) + 8.0 * r_n * nn
        sizes.append(f"{label}: nn = {nn}, ne = {ne} (mean degree {ne / nn:.2f}), nnz = {ne + nn}; residual {res / nn:.1f} B per node")
        print("built and checked " + sizes[-1], flush=True)
        for what, fn, fam, b in (("residual", lambda P=P, uu=uu: P.residual(uu), "residual", res),
                                 ("JVP     ", lambda P=P, uu=uu, vv=vv: P.jvp(vv, uu), "jvp", res + 8.0 * nn),
                                 ("fill     slot per thread", lambda P=P, uu=uu, J=J: P.jac_values(uu, J), "jacfill", res + 12.0 * (ne + nn)),
                                 ("fill     node per thread", lambda Pn=Pn, uu=uu, Jn=Jn: Pn.jac_values(uu, Jn), "jacfill", res + 12.0 * (ne + nn))):
            calls[f"{what} {label}"] = (fn, fam)
            meta[f"{what} {label}"] = b
    order = sorted(calls, key=lambda k: ("res", "JVP", "fil").index(k[:3]))
    ts = kernel_samples(ctx, {k: calls[k] for k in order}, args.reps)
    med = {k: statistics.median(ts[k]) for k in order}
    lines = [f"Compiled graph problems beside the compiled grid problem (Bratu {ns} x {ns}), {torch.cuda.get_device_name(0)}"] + sizes + [
             f"kernel begin -> end device timestamps, one launch per sample, problems alternating, {args.reps} samples after 20;",
             "GB/s on algorithmic bytes (grid: residual 16 n, JVP 24 n, fill 8 nnz + 12 n; graph: see above, fill + 12 per slot)", "",
             f"  {'kernel':56s} {'median us':>10s} {'p10':>9s} {'p90':>9s} {'GB/s (median)':>14s}  {'x grid':>7s}  algorithmic MB"]
    grid_of = {"res": med["residual grid  nk_grid_residual"], "JVP": med["JVP      grid  nk_grid_jvp"], "fil": med["fill     grid  nk_grid_jac"]}
    for k in order:
        t = ts[k]
        lines.append(f"  {k:56s} {med[k]:10.2f} {t[len(t) // 10]:9.2f} {t[(9 * len(t)) // 10]:9.2f} {meta[k] / med[k] / 1e3:14.1f}  "
                     f"{med[k] / grid_of[k[:3]]:7.2f}  {meta[k] / 1e6:.1f}")
    lines += ["", f"time to |F|inf <= 1e-8 from u = 0: NewtonRaphson, concrete J, GMRES with the AMG precs on the right; median wall time of "
              f"{args.solves} solves after one warm-up solve"]
    t, sol = solve_time(lambda: G, nn, args.solves)
    lines.append(f"  {'grid  bratu (CompiledGridProblem)':40s} {1e3 * t:9.1f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} GMRES iterations")
    for label, (P, _Pn, _u, _v, _ne, _re, _rn) in cases.items():
        t, sol = solve_time(lambda P=P: P, nn, args.solves)
        lines.append(f"  {label:40s} {1e3 * t:9.1f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} GMRES iterations")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for P, Pn, *_ in cases.values():
        P.close()
        Pn.close()
    G.close()


if __name__ == "__main__":
    main()
