"""What element blocks cost (csrc/nk_elem.hip, "Blocks"), measured against the one-block problem on the same nodes in the same
process, on the triangulation tools/elem_problem_bench.py builds — `--grid`² nodes (1024²), natural order:

    one block      P1 Bratu on all triangles                                        (the plain layout: the parent's programs)
    + Robin bars   the same triangles plus the 4·(grid − 1) boundary bars as a second block with the radiation term
                   p2·len·(u⁴ − w⁴), the ambient value w an element datum
    quads + tris   the left half of the cells as Q1 Bratu quads (2 × 2 Gauss points), the right half as the P1 triangles

A callback of a problem of several blocks is one generated launch per block and ONE k_elem_gather. Both carry the library's
per-kernel event timing — the generated kernels in the callback's family (residual, jvp, jacfill; the blocks' launches are summed),
the gather in the family elem_gather: one call per sample, the problems alternating, the median of `--reps` samples after 10.
GB/s on DESIGN §6h's byte model with TB = Σ npe_k·ne_k and TM = Σ npe_k²·ne_k (dof = 1, r_n = 2 node data arrays, S = the
pattern's entries, n_k the nodes block k touches):

    element kernels   Σ_k [conn 4·npe_k·ne_k + (u 8 + node data 8·r_n)·n_k + element data 8·nelem_k·ne_k] + B written 8·TB
                      (JVP: + v 8·n_k; the fill writes M, 8·TM, instead of B)
    gather F / J·v    list pointers 4·nn + lists 4·TB + B read 8·TB + mask 4·nn + out 8·nn
    gather J          list pointers 4·S + lists 4·TM + M read 8·TM + slot → node 4·S + row pointers, spos, mask 12·nn + out 8·S

    python tools/elem_blocks_bench.py [--out profiles/elem_blocks_bench.txt] [--grid 1024] [--reps 50]
"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import nonlinearsolve_jl_amd as nls
from elem_problem_bench import BRATU_ELEM_SRC, samples

ROBIN_SRC = """
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real dx = u.x(1, 0) - u.x(0, 0), dy = u.x(1, 1) - u.x(0, 1), len = sqrt(dx * dx + dy * dy);
  const nk_real w2 = u.w(0) * u.w(0), w4 = w2 * w2, k = (p[1] * p[2] * len) * (1.0 / 6.0);
  const T a2 = u.at(0) * u.at(0), b2 = u.at(1) * u.at(1);
  const T q0 = a2 * a2 - w4, q1 = b2 * b2 - w4;
  f[0] = k * (2.0 * q0 + q1);
  f[1] = k * (q0 + 2.0 * q1);
}
"""

# Q1 Bratu on a quadrilateral, 2 × 2 Gauss points, the exponential at the nodes weighted by the shape functions
QUAD_BRATU_SRC = """
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real XI[4] = {-1.0, 1.0, 1.0, -1.0}, ETA[4] = {-1.0, -1.0, 1.0, 1.0}, G = 0.5773502691896257;
  T ex[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { f[a] = T(0.0); ex[a] = exp(u.at(a)); }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const nk_real xi = G * XI[g], eta = G * ETA[g];
    nk_real N[4], dxi[4], deta[4], j00 = 0.0, j01 = 0.0, j10 = 0.0, j11 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      N[a] = 0.25 * ((1.0 + XI[a] * xi) * (1.0 + ETA[a] * eta));
      dxi[a] = 0.25 * (XI[a] * (1.0 + ETA[a] * eta));
      deta[a] = 0.25 * (ETA[a] * (1.0 + XI[a] * xi));
      j00 = j00 + dxi[a] * u.x(a, 0);
      j01 = j01 + dxi[a] * u.x(a, 1);
      j10 = j10 + deta[a] * u.x(a, 0);
      j11 = j11 + deta[a] * u.x(a, 1);
    }
    const nk_real det = j00 * j11 - j01 * j10, id = 1.0 / det, wd = p[1] * fabs(det);
    nk_real nx[4], ny[4];
    T gx = T(0.0), gy = T(0.0);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      nx[a] = (j11 * dxi[a] - j01 * deta[a]) * id;
      ny[a] = (j00 * deta[a] - j10 * dxi[a]) * id;
      gx = gx + nx[a] * u.at(a);
      gy = gy + ny[a] * u.at(a);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = f[a] + (wd * (gx * nx[a] + gy * ny[a]) - ((p[0] * wd) * N[a]) * ex[a]);
  }
}
"""


def cells(ns, seed=1):
    """the (ns − 1)² cells' corners a, b, c, d (counter-clockwise) and the diagonal elem_problem_bench.triangles picks"""
    idx = np.arange(ns * ns, dtype=np.int64).reshape(ns, ns)
    main = np.random.default_rng(seed).integers(2, size=(ns - 1, ns - 1)).astype(bool).ravel()
    return idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel(), main


def tris_of(a, b, c, d, main):
    t1 = np.where(main[:, None], np.stack([a, b, c], 1), np.stack([a, b, d], 1))
    t2 = np.where(main[:, None], np.stack([a, c, d], 1), np.stack([b, c, d], 1))
    return np.ascontiguousarray(np.stack([t1, t2], 1).reshape(-1, 3), dtype=np.int32)


def boundary_bars(ns):
    """the 4·(ns − 1) boundary edges, counter-clockwise"""
    r = np.arange(ns - 1)
    top = (ns - 1) * ns
    bars = np.concatenate([np.stack([r, r + 1], 1), np.stack([(r + 1) * ns - 1, (r + 2) * ns - 1], 1),
                           np.stack([top + r + 1, top + r], 1), np.stack([(r + 1) * ns, r * ns], 1)])
    return np.ascontiguousarray(bars, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elem_blocks_bench.txt"))
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    ns = args.grid
    nn = ns * ns
    ctx = nls.default_context()
    gen = torch.Generator(device="cuda").manual_seed(1)
    u = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    v = 2.0 * torch.rand(nn, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    jj, ii = np.divmod(np.arange(nn), ns)
    x, y = ii / (ns - 1.0), jj / (ns - 1.0)
    par = [6.0, float((ns - 1) ** 2), 1.0 / (ns - 1.0)]   # p2 scales the boundary term to the equation's 1/h² (a length, not an area)
    a, b, c, d, diag = cells(ns)
    tri = tris_of(a, b, c, d, diag)
    bars = boundary_bars(ns)
    left = (np.arange((ns - 1) ** 2) % (ns - 1)) < (ns - 1) // 2
    quads = np.ascontiguousarray(np.stack([a, b, c, d], 1)[left], dtype=np.int32)
    tri_right = tris_of(a[~left], b[~left], c[~left], d[~left], diag[~left])
    Block = nls.ElementBlock
    kw = dict(params=par, node_data=2)
    # label → (problem, the connectivities of its blocks)
    built = {
        "one block": (nls.CompiledElementProblem(BRATU_ELEM_SRC, tri, nn, **kw), [tri]),
        "+ Robin bars": (nls.CompiledElementProblem(BRATU_ELEM_SRC, tri, nn, blocks=[Block(ROBIN_SRC, bars, elem_data=1)], **kw), [tri, bars]),
        "quads + tris": (nls.CompiledElementProblem(QUAD_BRATU_SRC, quads, nn, blocks=[Block(BRATU_ELEM_SRC, tri_right)], **kw),
                         [quads, tri_right]),
    }
    built["+ Robin bars"][0].set_elem_data(0, np.random.default_rng(3).uniform(0.5, 1.5, bars.shape[0]), block=1)
    sizes, calls, model = [], {}, {}
    for label, (P, conns) in built.items():
        P.set_node_data(0, x)
        P.set_node_data(1, y)
        J = P.jac_csr()
        P.jac_values(u, J)
        jv = P.jvp(v, u)
        assert float((J.matvec(v) - jv).abs().max()) <= 1e-10 * max(1.0, float(jv.abs().max())), label   # fill·v is the JVP
        S = J.info()["nnz"]
        tb = sum(cn.size for cn in conns)
        tm = sum(cn.size * cn.shape[1] for cn in conns)
        touched = [np.unique(cn).size for cn in conns]
        read = sum(4.0 * cn.size + 8.0 * nel * cn.shape[0] for cn, (_, _, nel) in zip(conns, P.blocks))
        res = (read + 24.0 * sum(touched) + 8.0 * tb, 4.0 * nn + 12.0 * tb + 12.0 * nn)
        jvp = (res[0] + 8.0 * sum(touched), res[1])
        fill = (read + 24.0 * sum(touched) + 8.0 * tm, 8.0 * S + 12.0 * tm + 12.0 * nn + 8.0 * S)
        sizes.append(f"{label}: blocks (ne, npe, element data) = {P.blocks}, TB = {tb}, TM = {tm}, S = {S}; model residual "
                     f"{sum(res) / nn:.1f} B per node, fill {sum(fill) / nn:.1f}")
        for what, fn, fam, m in (("residual", lambda P=P: P.residual(u), "residual", res), ("JVP     ", lambda P=P: P.jvp(v, u), "jvp", jvp),
                                 ("fill    ", lambda P=P, J=J: P.jac_values(u, J), "jacfill", fill)):
            calls[f"{what} {label}"], model[f"{what} {label}"] = (fn, fam), m
    # the boundary block changes the boundary rows and nothing else
    f1, f2 = built["one block"][0].residual(u), built["+ Robin bars"][0].residual(u)
    on_edge = torch.as_tensor((ii == 0) | (ii == ns - 1) | (jj == 0) | (jj == ns - 1), device="cuda")
    assert bool((f1 == f2)[~on_edge].all()) and bool((f1 != f2)[on_edge].any())
    med = samples(ctx, calls, args.reps)
    lines = [f"Element blocks: P1 Bratu on a triangulation of {ns} x {ns} nodes, {torch.cuda.get_device_name(0)}"] + sizes + [
             f"kernel begin -> end device timestamps, one call per sample, problems alternating, {args.reps} samples after 10; medians;",
             "kernels us: the generated launches of all blocks summed; GB/s on the byte model of the tool's header; x one block = sum / the "
             "one-block problem's sum", "",
             f"  {'call':24s} {'kernels us':>10s} {'gather us':>10s} {'sum us':>10s} {'GB/s kernels':>13s} {'GB/s gather':>12s} {'GB/s sum':>9s} {'x one block':>12s}"]
    for k in calls:
        ker, g, t = med[k]
        mk, mg = model[k]
        base = med[k[:9] + "one block"][2]
        lines.append(f"  {k:24s} {ker:10.2f} {g:10.2f} {t:10.2f} {mk / ker / 1e3:13.1f} {mg / g / 1e3:12.1f} {(mk + mg) / t / 1e3:9.1f} {t / base:12.3f}")
    lines += ["", "difference to the one-block problem, us (kernels | gather | sum):"]
    for k in calls:
        if not k.endswith("one block"):
            o = med[k[:9] + "one block"]
            lines.append(f"  {k:24s} {med[k][0] - o[0]:+10.2f} {med[k][1] - o[1]:+10.2f} {med[k][2] - o[2]:+10.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for P, _ in built.values():
        P.close()


if __name__ == "__main__":
    main()
