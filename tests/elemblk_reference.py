"""The table of the element-block tests: block meshes, and every case as the HIP sources of its blocks beside the same formulas
in NumPy (tests/elemblk_core.py evaluates them; the one-block table tests/elem_reference.py supplies most sources).

Cases — the smallest shapes at which something can go wrong
    split-*      tri257p with its 452 elements cut into two blocks of the same source, after element 1 and after element 256
                 (the second cut puts a workgroup boundary of the first block's kernel at its very end); bratu and react2. The
                 summation order is that of the one-block problem, so the device results must be the one-block problem's bits
    quadtri      an 8 × 5-node rectangle: the left 3 columns of cells as quads (Q1 p-Laplacian diffusion), the right 4 as
                 triangle pairs (P1 diffusion), sharing the interface nodes
    robin        tri30 (P1 Bratu) plus the 18 bars on its boundary edges — the edges in exactly one triangle — with the radiation
                 term p1·len·(u⁴ − w⁴), consistent weights (2, 1; 1, 2)/6, the ambient value w an element datum of the bars: the
                 entries (i, j) of boundary edges get contributions from both blocks
    springs      tri30 with react2 (dof 2) plus 5 truss bars between nodes that share no triangle: their pattern entries come
                 from the bar block alone
    points       the strip with its orphans (P1 Bratu) plus an npe = 1 block on nodes 0, 5 and 8 — node 5 is in no other
                 element — a cubic nodal spring whose stiffness is an element datum
    indexed      integer-valued sources on tri30's triangles, its boundary bars and 7 points: combinations of u.node(a), s.e,
                 s.ne, NK_BLOCK, u.w(k) and u.at that are exact in float64 — bit for bit
    three        tri30: Bratu (no element data), the Robin bars (1 datum) and 6 bars with 4 data
    eight        tri2's 4 nodes, eight tiny blocks of the indexed source with npe 3, 2, 1, 3, 2, 1, 2, 1 — bit for bit"""
import numpy as np

import elem_core as EC
import elem_reference as R
import elemblk_core as BC
from elem_core import Problem, gsqrt
from elemblk_core import BlockMesh, BlockProblem

# ------------------------------------------------------------------------------------------------ sources
ROBIN_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real dx = u.x(1, 0) - u.x(0, 0), dy = u.x(1, 1) - u.x(0, 1), len = sqrt(dx * dx + dy * dy);
  const nk_real w2 = u.w(0) * u.w(0), w4 = w2 * w2, k = (p[1] * len) * (1.0 / 6.0);
  const T a2 = u.at(0) * u.at(0), b2 = u.at(1) * u.at(1);
  const T q0 = a2 * a2 - w4, q1 = b2 * b2 - w4;
  f[0] = k * (2.0 * q0 + q1);
  f[1] = k * (q0 + 2.0 * q1);
}
"""


def _robin(u, p, s):
    dx, dy = u.x(1, 0) - u.x(0, 0), u.x(1, 1) - u.x(0, 1)
    ln = gsqrt(dx * dx + dy * dy)
    w2 = u.w(0) * u.w(0)
    w4, k = w2 * w2, (p[1] * ln) * (1.0 / 6.0)
    a2, b2 = u.at(0) * u.at(0), u.at(1) * u.at(1)
    q0, q1 = a2 * a2 - w4, b2 * b2 - w4
    return [k * (2.0 * q0 + q1), k * (q0 + 2.0 * q1)]


POINT_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const T x = u.at(0);
  f[0] = u.w(0) * (x + p[0] * (x * (x * x)));
}
"""


def _point(u, p, s):
    x = u.at(0)
    return [u.w(0) * (x + p[0] * (x * (x * x)))]


FOUR_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const T a = u.at(0), b = u.at(1);
  f[0] = u.w(0) * a + u.w(1) * (b * b);
  f[1] = u.w(2) * b + u.w(3) * (a * b);
}
"""


def _four(u, p, s):
    a, b = u.at(0), u.at(1)
    return [u.w(0) * a + u.w(1) * (b * b), u.w(2) * b + u.w(3) * (a * b)]


BLOCK_INDEXED_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
#pragma unroll
  for (int a = 0; a < NK_NPE; ++a) {
    const int b = (a + 1) % NK_NPE;
    const nk_real c = (nk_real)(1 + (u.node(a) + s.e + 3 * NK_BLOCK) % 7) + u.x(a, 0) * u.w(0);
    f[a] = c * (u.at(a) * u.at(b)) + ((nk_real)(u.node(b) % 5 + NK_BLOCK) * u.at(a) - (nk_real)((s.e + s.ne + s.nn) % 3));
  }
}
"""


def _block_indexed(u, p, s):
    out = []
    for a in range(u.npe):
        b = (a + 1) % u.npe
        c = u.real(1 + (u.node(a) + s.e + 3 * u.block) % 7) + u.x(a, 0) * u.w(0)
        out.append(c * (u.at(a) * u.at(b)) + (u.real(u.node(b) % 5 + u.block) * u.at(a) - u.real((s.e + s.ne + s.nn) % 3)))
    return out


def _indexed(npe):
    return Problem(f"bindexed{npe}", BLOCK_INDEXED_SRC, npe, 1, [], _block_indexed, [], [("int", -2, 2)])


AMBIENT, STIFF = (0.5, 1.5), (0.5, 2.0)
ROBIN = Problem("robin", ROBIN_SRC, 2, 1, [], _robin, [], [AMBIENT])
POINT = Problem("point", POINT_SRC, 1, 1, [], _point, [], [STIFF])
FOUR = Problem("four", FOUR_SRC, 2, 1, [], _four, [], [(-1.0, 1.0)] * 4)


# ------------------------------------------------------------------------------------------------ meshes
def boundary_edges(M):
    """the edges of a triangulation that lie in exactly one triangle, in the order they are first met, oriented as met"""
    seen = {}
    for el in M.conn:
        for a in range(3):
            i, j = int(el[a]), int(el[(a + 1) % 3])
            seen.setdefault((min(i, j), max(i, j)), []).append((i, j))
    return [v[0] for v in seen.values() if len(v) == 1]


def _split(M, cut):
    return BlockMesh(f"{M.name}/{cut}", M.nn, [M.conn[:cut], M.conn[cut:]], M.X, M.boundary)


def _quadtri():
    nx, ny, cut = 8, 5, 3
    at = lambda i, j: j * nx + i   # noqa: E731
    rng = np.random.default_rng(77)
    quads, tris = [], []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            if i < cut:
                quads.append([a, b, c, d])
            else:
                tris += [[a, b, d], [b, c, d]] if rng.integers(2) else [[a, b, c], [a, c, d]]
    xs, ys = np.meshgrid(np.arange(nx) / (nx - 1.0), 0.8 * np.arange(ny) / (ny - 1.0))
    X = np.stack([xs.ravel() + 0.1 * ys.ravel(), ys.ravel() + 0.04 * xs.ravel() ** 2])
    bd = [at(i, j) for j in range(ny) for i in range(nx) if i in (0, nx - 1) or j in (0, ny - 1)]
    return BlockMesh("quadtri8x5", nx * ny, [quads, tris], X, bd)


_T30, _T257, _STRIP, _T2 = R.MESHES["tri30"], R.MESHES["tri257p"], R.MESHES["strip"], R.MESHES["tri2"]
_EDGES30 = boundary_edges(_T30)
SPRINGS = [(0, 2), (1, 3), (6, 20), (12, 29), (5, 24)]
POINT_NODES = [[0], [5], [8]]
SIX_BARS = [(0, 7), (7, 14), (14, 21), (3, 28), (9, 10), (2, 27)]

MESHES = {m.name: m for m in (
    _split(_T257, 1), _split(_T257, 256), _quadtri(),
    BlockMesh("tri30+edges", _T30.nn, [_T30.conn, _EDGES30], _T30.X, _T30.boundary),
    BlockMesh("tri30+springs", _T30.nn, [_T30.conn, SPRINGS], _T30.X, _T30.boundary),
    BlockMesh("strip+points", _STRIP.nn, [_STRIP.conn, POINT_NODES], _STRIP.X, _STRIP.boundary),
    BlockMesh("tri30+edges+points", _T30.nn, [_T30.conn, _EDGES30, [[0], [7], [7], [14], [29], [3], [16]]], _T30.X, _T30.boundary),
    BlockMesh("tri30+edges+six", _T30.nn, [_T30.conn, _EDGES30, SIX_BARS], _T30.X, _T30.boundary),
    BlockMesh("tri2x8", _T2.nn, [[[0, 1, 2], [1, 3, 2]], [[0, 3], [1, 2]], [[3], [0], [3]], [[2, 1, 3]], [[3, 0]], [[1]], [[2, 0], [0, 1]],
                                 [[2], [2]]], _T2.X, _T2.boundary))}

# ------------------------------------------------------------------------------------------------ the table
_P = R.PROBLEMS
XY = ["x", "y"]
PROBLEMS = {
    "split-bratu": BlockProblem("split-bratu", [_P["bratu"], _P["bratu"]], _P["bratu"].params, XY),
    "split-react2": BlockProblem("split-react2", [_P["react2"], _P["react2"]], _P["react2"].params, XY),
    "quadtri": BlockProblem("quadtri", [_P["plap"], _P["diffusion"]], _P["plap"].params, ["x", "y", R.SOURCE]),
    "robin": BlockProblem("robin", [_P["bratu"], ROBIN], [1.0, 0.5], XY),
    "springs": BlockProblem("springs", [_P["react2"], _P["truss"]], _P["react2"].params, XY),
    "points": BlockProblem("points", [_P["bratu"], POINT], [1.0], XY),
    "indexed": BlockProblem("indexed", [_indexed(3), _indexed(2), _indexed(1)], [], [("int", -3, 3)]),
    "three": BlockProblem("three", [_P["bratu"], ROBIN, FOUR], [1.0, 0.5], XY),
    "eight": BlockProblem("eight", [_indexed(n) for n in (3, 2, 1, 3, 2, 1, 2, 1)], [], [("int", -3, 3)]),
}
EXACT = ("indexed", "eight")
SPLITS = [("split-bratu", "tri257p/1", "bratu"), ("split-bratu", "tri257p/256", "bratu"),
          ("split-react2", "tri257p/1", "react2"), ("split-react2", "tri257p/256", "react2")]
PAIRS = [(p, m) for p, m, _ in SPLITS] + [("quadtri", "quadtri8x5"), ("robin", "tri30+edges"), ("springs", "tri30+springs"),
                                           ("points", "strip+points"), ("indexed", "tri30+edges+points"), ("three", "tri30+edges+six"),
                                           ("eight", "tri2x8")]
CASES = [(p, m, masked) for p, m in PAIRS for masked in (False, True)]
for _p, _m in PAIRS:
    assert [q.npe for q in PROBLEMS[_p].parts] == [b.npe for b in MESHES[_m].blocks], (_p, _m)

assert BC and EC
