"""The kernels of a compiled element problem (csrc/nk_elem.hip) on the triangulation tools/graph_problem_bench.py builds —
`--grid`² nodes (1024²), a random diagonal per cell — in natural order and with the nodes randomly permuted: P1 Bratu with the
exponential lumped at the nodes (node data x, y), beside the compiled GRAPH problem's `sink` kernels on the same mesh, in the
same process.

Every callback of an element problem is two launches: the generated kernel (one element, for the fill one (element, local node)
pair, per thread) and k_elem_gather. Both carry the library's per-kernel event timing — the generated kernel in its family
(residual, jvp, jacfill), the gather in the family elem_gather — so the table has each launch and their sum: one call per sample,
the problems alternating, the median of `--reps` samples after a warm-up. GB/s on the byte model, per pass (ne elements, nn
nodes, npe = 3, dof = 1, L = npe·dof = 3, r_n = 2 node data arrays, S = the pattern's entries):

    element residual   conn 4·npe·ne + u 8·nn + node data 8·r_n·nn + B written 8·L·ne              (JVP: + v 8·nn)
    gather F / J·v     list pointers 4·nn + lists 4·npe·ne + B read 8·L·ne + mask 4·nn + out 8·nn
    element matrices   conn 4·npe·ne + u 8·nn + node data 8·r_n·nn + M written 8·L²·ne
    gather J           list pointers 4·S + lists 4·npe²·ne + M read 8·L²·ne + slot → node 4·S + row pointers, spos, mask 12·nn
                       + out 8·S

u and the node data are counted once per node (the gathers through conn are expected from cache; that holds for the natural
order and not for the permuted one). The graph kind's model is graph_problem_bench's.

Then the time to ‖F‖∞ <= 1e-8 from the initial guess — NewtonRaphson on the concrete Jacobian, GMRES with the aggregation AMG
`precs` on the right, the boundary nodes fixed at 0 — the median wall time of `--solves` solves after one warm-up solve.

    python tools/elem_problem_bench.py [--out profiles/elem_problem_bench.txt] [--grid 1024] [--reps 50] [--solves 2]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import graph_reference as GR
import nonlinearsolve_jl_amd as nls
from graph_problem_bench import mesh

# P1 Bratu, −Δu = p0·exp(u), the exponential lumped; p1 scales the equation (1/h², so that the residual is O(1) like the grid's)
BRATU_ELEM_SRC = """
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real x1 = u.x(1, 0) - u.x(0, 0), y1 = u.x(1, 1) - u.x(0, 1), x2 = u.x(2, 0) - u.x(0, 0), y2 = u.x(2, 1) - u.x(0, 1);
  const nk_real det = x1 * y2 - x2 * y1, area = p[1] * (0.5 * fabs(det)), id = 1.0 / det, third = area * (1.0 / 3.0);
  const nk_real bx[3] = {(y1 - y2) * id, y2 * id, (-y1) * id}, by[3] = {(x2 - x1) * id, (-x2) * id, x1 * id};
  const T u0 = u.at(0), u1 = u.at(1), u2 = u.at(2);
  const T gx = bx[0] * u0 + bx[1] * u1 + bx[2] * u2, gy = by[0] * u0 + by[1] * u1 + by[2] * u2;
#pragma unroll
  for (int a = 0; a < 3; ++a) f[a] = area * (gx * bx[a] + gy * by[a]) - (p[0] * third) * exp(u.at(a));
}
"""


def triangles(nx, ny, perm=None, seed=1):
    """conn [ne, 3] int32 of the triangulation graph_problem_bench.mesh(nx, ny, True, perm, seed) is the node graph of"""
    idx = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    main = np.random.default_rng(seed).integers(2, size=(ny - 1, nx - 1)).astype(bool).ravel()
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    t1 = np.where(main[:, None], np.stack([a, b, c], 1), np.stack([a, b, d], 1))
    t2 = np.where(main[:, None], np.stack([a, c, d], 1), np.stack([b, c, d], 1))
    conn = np.stack([t1, t2], 1).reshape(-1, 3)
    if perm is not None:
        conn = perm[conn]
    return np.ascontiguousarray(conn, dtype=np.int32)


def samples(ctx, calls, reps, warm=10):
    """calls: {label: (callable, family)}; per label the per-call device times in µs of the family's launch, of the gather
    (0 for a graph problem: one launch) and of both"""
    out = {k: ([], [], []) for k in calls}
    for i in range(warm + reps):
        for label, (fn, family) in calls.items():
            ctx.profile_enable(True)       # (also resets the accumulators)
            fn()
            r = ctx.profile_report()
            if i >= warm:
                a, g = 1e3 * r[family]["total_ms"], 1e3 * r.get("elem_gather", {"total_ms": 0.0})["total_ms"]
                for lst, x in zip(out[label], (a, g, a + g)):
                    lst.append(x)
    ctx.profile_enable(False)
    return {k: tuple(statistics.median(x) for x in v) for k, v in out.items()}


def solve_time(P, u0, solves):
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(precs=nls.ObjectPrecs("amg", "right")), concrete_jac=True)
    times, sol = [], None
    for k in range(solves + 1):
        start = u0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sol = nls.solve(nls.NonlinearProblem(P, start), alg, abstol=1e-8, maxiters=60)
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), sol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elem_problem_bench.txt"))
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--solves", type=int, default=2)
    args = ap.parse_args()
    ns = args.grid
    nn = ns * ns
    ctx = nls.default_context()
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    v = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    rng = np.random.default_rng(2)
    perm = rng.permutation(nn)
    inv = np.argsort(perm)
    dev_inv = torch.as_tensor(inv, device="cuda")
    jj, ii = np.divmod(np.arange(nn), ns)
    x, y = ii / (ns - 1.0), jj / (ns - 1.0)
    edge = (ii == 0) | (ii == ns - 1) | (jj == 0) | (jj == ns - 1)
    par = [6.0, float((ns - 1) ** 2)]
    sink = GR.PROBLEMS["sink"]
    w_pair, kappa, mass = rng.uniform(0.5, 1.5, nn), rng.uniform(0.05, 0.15, nn), rng.uniform(0.5, 1.0, nn)

    def to_perm(z):
        out = np.empty_like(z)
        out[perm] = z
        return out

    cases = {}   # label → (element problem, graph problem, u, v, ne, graph edges, boundary mask)
    for label, pm in (("natural", None), ("permuted", perm)):
        conn = triangles(ns, ns, pm)
        E = nls.CompiledElementProblem(BRATU_ELEM_SRC, conn, nn, params=par, node_data=2)
        E.set_node_data(0, x if pm is None else to_perm(x))
        E.set_node_data(1, y if pm is None else to_perm(y))
        rp, ci, src = mesh(ns, ns, True, pm)
        assert np.array_equal(rp, nls.elem_adjacency(conn, nn)[0])   # the same mesh
        G = nls.CompiledGraphProblem(sink.source, rp, ci, params=sink.params, edge_data=1, node_data=2)
        s, d = (src, ci) if pm is None else (inv[src], inv[ci])
        G.set_edge_data(0, 0.5 * (w_pair[s] + w_pair[d]))
        G.set_node_data(0, kappa if pm is None else to_perm(kappa))
        G.set_node_data(1, mass if pm is None else to_perm(mass))
        uu, vv = (u, v) if pm is None else (u[dev_inv], v[dev_inv])
        cases[label] = (E, G, uu, vv, conn.shape[0], ci.size, edge if pm is None else to_perm(edge))
        print(f"built {label}: nn = {nn}, ne = {conn.shape[0]}, node pairs = {ci.size}", flush=True)
    # the numbers before anything is timed: permuted is natural renumbered; fill·v is the JVP, free and with the boundary fixed
    fn_, fp_ = cases["natural"][0].residual(u), cases["permuted"][0].residual(u[dev_inv])
    assert float((fp_ - fn_[dev_inv]).abs().max()) <= 1e-9 * max(1.0, float(fn_.abs().max()))
    calls, model, sizes = {}, {}, []
    for label, (E, G, uu, vv, ne, nedges, bd) in cases.items():
        S = nedges + nn
        for fixed in (False, True):
            E.set_fixed(bd if fixed else np.zeros(nn, dtype=np.int32))
            J = E.jac_csr()
            E.jac_values(uu, J)
            jv = E.jvp(vv, uu)
            assert float((J.matvec(vv) - jv).abs().max()) <= 1e-10 * max(1.0, float(jv.abs().max()))
        JG = G.jac_csr()
        common = 12.0 * ne + 8.0 * nn + 16.0 * nn
        res = (common + 24.0 * ne, 4.0 * nn + 12.0 * ne + 24.0 * ne + 4.0 * nn + 8.0 * nn)
        jvp = (res[0] + 8.0 * nn, res[1])
        fill = (common + 72.0 * ne, 4.0 * S + 36.0 * ne + 72.0 * ne + 4.0 * S + 12.0 * nn + 8.0 * S)
        gres = 20.0 * nn + nedges * 12.0 + 16.0 * nn
        sizes.append(f"{label}: nn = {nn}, ne = {ne}, S = {S}; element residual {sum(res) / nn:.1f} B per node (graph sink {gres / nn:.1f}), "
                     f"fill {sum(fill) / nn:.1f} (graph {(gres + 12.0 * S) / nn:.1f})")
        for what, fe, fg, fam, me, mg in (
                ("residual", lambda E=E, uu=uu: E.residual(uu), lambda G=G, uu=uu: G.residual(uu), "residual", res, gres),
                ("JVP     ", lambda E=E, uu=uu, vv=vv: E.jvp(vv, uu), lambda G=G, uu=uu, vv=vv: G.jvp(vv, uu), "jvp", jvp, gres + 8.0 * nn),
                ("fill    ", lambda E=E, uu=uu, J=J: E.jac_values(uu, J), lambda G=G, uu=uu, JG=JG: G.jac_values(uu, JG), "jacfill", fill,
                 gres + 12.0 * S)):
            calls[f"{what} {label:9s} elements"], model[f"{what} {label:9s} elements"] = (fe, fam), me
            calls[f"{what} {label:9s} graph sink"], model[f"{what} {label:9s} graph sink"] = (fg, fam), (mg, 0.0)
    med = samples(ctx, calls, args.reps)
    lines = [f"Compiled element problems: P1 Bratu on a triangulation of {ns} x {ns} nodes, {torch.cuda.get_device_name(0)}"] + sizes + [
             f"kernel begin -> end device timestamps, one call per sample, problems alternating, {args.reps} samples after 10; medians;",
             "GB/s on the byte model of the tool's header (element kernel | gather | both); x graph = both launches / the graph kernel", "",
             f"  {'call':38s} {'kernel us':>10s} {'gather us':>10s} {'sum us':>10s} {'GB/s kernel':>12s} {'GB/s gather':>12s} {'GB/s sum':>9s} {'x graph':>8s}"]
    for k in calls:
        a, g, t = med[k]
        ma, mg = model[k]
        base = med[k.replace("elements", "graph sink")][2]
        gg = f"{mg / g / 1e3:12.1f}" if g > 0 else f"{'-':>12s}"
        lines.append(f"  {k:38s} {a:10.2f} {g:10.2f} {t:10.2f} {ma / a / 1e3:12.1f} {gg} {(ma + mg) / t / 1e3:9.1f} {t / base:8.2f}")
    lines += ["", f"time to |F|inf <= 1e-8: NewtonRaphson, concrete J, GMRES with the AMG precs on the right; median wall time of {args.solves} "
              "solves after one warm-up solve (elements: boundary fixed at 0, from the initial guess; graph sink: from u = 0)"]
    for label, (E, G, uu, vv, ne, nedges, bd) in cases.items():
        E.set_fixed(bd)
        t, sol = solve_time(E, E.initial_guess(device=True), args.solves)
        lines.append(f"  {'elements   ' + label:28s} {1e3 * t:9.1f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} GMRES iterations")
        t, sol = solve_time(G, torch.zeros(nn, dtype=torch.float64, device="cuda"), args.solves)
        lines.append(f"  {'graph sink ' + label:28s} {1e3 * t:9.1f} ms  {sol.retcode}, {sol.stats.nsteps} steps, {sol.stats.gmres_iters} GMRES iterations")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for E, G, *_ in cases.values():
        E.close()
        G.close()


if __name__ == "__main__":
    main()
