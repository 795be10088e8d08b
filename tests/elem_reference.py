"""The table of the compiled element problems' tests: the meshes, and every problem as HIP source beside the same formula in
NumPy (tests/elem_core.py runs the formula on arrays with the device's dual-number rules, and element by element on scalars).
Every source has its loops over the local nodes unrolled (compile-time bounds), so the generated kernels keep f[] in registers.

Meshes — the smallest at which something can go wrong
    tri1, tri2      one triangle; two triangles sharing an edge
    tri30           a 6 × 5-node rectangle, a random diagonal per cell, natural order: 40 elements
    tri255p         17 × 15 nodes, 448 elements          } nodes and elements randomly renumbered, every element's local order
    tri256p         16 × 16 nodes, 450 elements          } cyclically rotated; node counts one short of a workgroup, exactly
    tri257p         16 × 16 nodes + a cell centre: 452   } one, and one past it
                    A planar triangulation of n nodes has at most 2n − 5 triangles, so with these node counts the element counts
                    lie on both sides of 256 (40 | 448, 450, 452) and cannot reach 512; the (element, local node) pairs of the
                    fill — one thread each — lie on both sides of 256 and 512 (120 | 1344, 1350, 1356), and the entry lists on
                    both sides of 512 as well.
    fan300          a closed fan: node 150 in 300 triangles — a gather list longer than a workgroup, one diagonal entry summed
                    from 300 terms
    strip           10 triangles on 12 of 14 nodes: nodes 5 and 13 (the last) are in no element; the mask fixes node 13
    quad7x5         7 × 5 quadrilaterals          tet3x3x2   3 × 3 × 2 cubes cut into six tetrahedra each (108)
    hex3x2x2        12 hexahedra                   truss      15 bars (npe = 2) on 9 nodes with degrees 1 to 6

Problems
    diffusion   P1, −∇·((1 + ū²)∇u) = g on triangles; node data x, y, g; no elementary function
    bratu       P1, −Δu = p0·exp(u), the exponential lumped at the nodes; node data x, y
    plap        Q1 p-Laplacian, 2 × 2 Gauss points, k = pow(p1 + |∇u|², p0); node data x, y, g
    tetdiff     P1 on tetrahedra, −∇·(κ_e (1 + p0 ū²) ∇u) = g; node data x, y, z, g; element datum κ
    react2      dof 2 on triangles: diffusion of both components, reactions u0·u1² − p0 and p2·u1 − u0·u1²; checks the dof blocks
    truss       dof 2, npe 2: bars with engineering strain, l = sqrt(·), N = (k/l0)(l − l0), a body load p per reference length;
                node data x, y; element datum k
    quad4       dof 4 on quads, npe·dof = 16: deviation from the element mean times the next component's mean
    hex8        npe 8: cubic spring to the element mean; element datum κ; node datum g
    indexed2/3/4/8   an integer-valued polynomial of s.e, u.node(a), u.x and u.w (integer data): bit for bit"""
import elem_core as EC
from elem_core import Problem, gdiv, gexp, gpow, gsqrt

# ------------------------------------------------------------------------------------------------ meshes
MESHES = {m.name: m for m in (EC.one_triangle(), EC.two_triangles(), EC.rectangle(6, 5, 1), EC.renumbered(EC.rectangle(17, 15, 1), 1),
                              EC.renumbered(EC.rectangle(16, 16, 1), 2), EC.renumbered(EC.rectangle(16, 16, 2, extra_centre=True), 3),
                              EC.fan(300, 150), EC.strip_with_orphans(), EC.quads(7, 5), EC.tets(3, 3, 2), EC.hexes(3, 2, 2),
                              EC.truss())}
TRIANGLES = ("tri1", "tri2", "tri30", "tri255p", "tri256p", "tri257p", "fan300", "strip")

# ------------------------------------------------------------------------------------------------ P1 triangles
_TRI_GEOMETRY = r"""
  const nk_real x1 = u.x(1, 0) - u.x(0, 0), y1 = u.x(1, 1) - u.x(0, 1), x2 = u.x(2, 0) - u.x(0, 0), y2 = u.x(2, 1) - u.x(0, 1);
  const nk_real det = x1 * y2 - x2 * y1, area = 0.5 * fabs(det), id = 1.0 / det, third = area * (1.0 / 3.0);
  const nk_real bx[3] = {(y1 - y2) * id, y2 * id, (-y1) * id}, by[3] = {(x2 - x1) * id, (-x2) * id, x1 * id};
"""


def _tri_geometry(u):
    x1, y1, x2, y2 = u.x(1, 0) - u.x(0, 0), u.x(1, 1) - u.x(0, 1), u.x(2, 0) - u.x(0, 0), u.x(2, 1) - u.x(0, 1)
    det = x1 * y2 - x2 * y1
    area, idet = 0.5 * abs(det), 1.0 / det
    third = area * (1.0 / 3.0)
    return area, third, [(y1 - y2) * idet, y2 * idet, (-y1) * idet], [(x2 - x1) * idet, (-x2) * idet, x1 * idet]


DIFFUSION_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {""" + _TRI_GEOMETRY + r"""
  const T u0 = u.at(0), u1 = u.at(1), u2 = u.at(2);
  const T gx = bx[0] * u0 + bx[1] * u1 + bx[2] * u2, gy = by[0] * u0 + by[1] * u1 + by[2] * u2;
  const T ub = (u0 + u1 + u2) * (1.0 / 3.0);
  const T k = (1.0 + ub * ub) * area;
#pragma unroll
  for (int a = 0; a < 3; ++a) f[a] = k * (gx * bx[a] + gy * by[a]) - third * u.x(a, 2);
}
"""


def _diffusion(u, p, s):
    area, third, bx, by = _tri_geometry(u)
    u0, u1, u2 = u.at(0), u.at(1), u.at(2)
    gx, gy = bx[0] * u0 + bx[1] * u1 + bx[2] * u2, by[0] * u0 + by[1] * u1 + by[2] * u2
    ub = (u0 + u1 + u2) * (1.0 / 3.0)
    k = (1.0 + ub * ub) * area
    return [k * (gx * bx[a] + gy * by[a]) - third * u.x(a, 2) for a in range(3)]


BRATU_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {""" + _TRI_GEOMETRY + r"""
  const T u0 = u.at(0), u1 = u.at(1), u2 = u.at(2);
  const T gx = bx[0] * u0 + bx[1] * u1 + bx[2] * u2, gy = by[0] * u0 + by[1] * u1 + by[2] * u2;
#pragma unroll
  for (int a = 0; a < 3; ++a) f[a] = area * (gx * bx[a] + gy * by[a]) - (p[0] * third) * exp(u.at(a));
}
"""


def _bratu(u, p, s):
    area, third, bx, by = _tri_geometry(u)
    u0, u1, u2 = u.at(0), u.at(1), u.at(2)
    gx, gy = bx[0] * u0 + bx[1] * u1 + bx[2] * u2, by[0] * u0 + by[1] * u1 + by[2] * u2
    return [area * (gx * bx[a] + gy * by[a]) - (p[0] * third) * gexp(u.at(a)) for a in range(3)]


REACT2_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {""" + _TRI_GEOMETRY + r"""
  const T gx0 = bx[0] * u.at(0, 0) + bx[1] * u.at(1, 0) + bx[2] * u.at(2, 0), gy0 = by[0] * u.at(0, 0) + by[1] * u.at(1, 0) + by[2] * u.at(2, 0);
  const T gx1 = bx[0] * u.at(0, 1) + bx[1] * u.at(1, 1) + bx[2] * u.at(2, 1), gy1 = by[0] * u.at(0, 1) + by[1] * u.at(1, 1) + by[2] * u.at(2, 1);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T a0 = u.at(a, 0), a1 = u.at(a, 1), r = a0 * (a1 * a1);
    f[2 * a] = area * (gx0 * bx[a] + gy0 * by[a]) + third * (r - p[0]);
    f[2 * a + 1] = (p[1] * area) * (gx1 * bx[a] + gy1 * by[a]) + third * (p[2] * a1 - r);
  }
}
"""


def _react2(u, p, s):
    area, third, bx, by = _tri_geometry(u)
    gx0 = bx[0] * u.at(0, 0) + bx[1] * u.at(1, 0) + bx[2] * u.at(2, 0)
    gy0 = by[0] * u.at(0, 0) + by[1] * u.at(1, 0) + by[2] * u.at(2, 0)
    gx1 = bx[0] * u.at(0, 1) + bx[1] * u.at(1, 1) + bx[2] * u.at(2, 1)
    gy1 = by[0] * u.at(0, 1) + by[1] * u.at(1, 1) + by[2] * u.at(2, 1)
    out = []
    for a in range(3):
        a0, a1 = u.at(a, 0), u.at(a, 1)
        r = a0 * (a1 * a1)
        out.append(area * (gx0 * bx[a] + gy0 * by[a]) + third * (r - p[0]))
        out.append((p[1] * area) * (gx1 * bx[a] + gy1 * by[a]) + third * (p[2] * a1 - r))
    return out


# ------------------------------------------------------------------------------------------------ Q1 p-Laplacian
PLAP_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real XI[4] = {-1.0, 1.0, 1.0, -1.0}, ETA[4] = {-1.0, -1.0, 1.0, 1.0}, G = 0.5773502691896257;
#pragma unroll
  for (int a = 0; a < 4; ++a) f[a] = T(0.0);
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
    const nk_real det = j00 * j11 - j01 * j10, id = 1.0 / det, wd = fabs(det);
    nk_real nx[4], ny[4];
    T gx = T(0.0), gy = T(0.0);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      nx[a] = (j11 * dxi[a] - j01 * deta[a]) * id;
      ny[a] = (j00 * deta[a] - j10 * dxi[a]) * id;
      gx = gx + nx[a] * u.at(a);
      gy = gy + ny[a] * u.at(a);
    }
    const T k = pow(p[1] + (gx * gx + gy * gy), p[0]) * wd;
#pragma unroll
    for (int a = 0; a < 4; ++a) f[a] = f[a] + (k * (gx * nx[a] + gy * ny[a]) - (wd * N[a]) * u.x(a, 2));
  }
}
"""


def _plap(u, p, s):
    XI, ETA, G = [-1.0, 1.0, 1.0, -1.0], [-1.0, -1.0, 1.0, 1.0], 0.5773502691896257
    f = [u.zero() for _ in range(4)]
    for g in range(4):
        xi, eta = G * XI[g], G * ETA[g]
        N = [0.25 * ((1.0 + XI[a] * xi) * (1.0 + ETA[a] * eta)) for a in range(4)]
        dxi = [0.25 * (XI[a] * (1.0 + ETA[a] * eta)) for a in range(4)]
        deta = [0.25 * (ETA[a] * (1.0 + XI[a] * xi)) for a in range(4)]
        j00 = j01 = j10 = j11 = u.real(0.0)
        for a in range(4):
            j00 = j00 + dxi[a] * u.x(a, 0)
            j01 = j01 + dxi[a] * u.x(a, 1)
            j10 = j10 + deta[a] * u.x(a, 0)
            j11 = j11 + deta[a] * u.x(a, 1)
        det = j00 * j11 - j01 * j10
        idet, wd = 1.0 / det, abs(det)
        nx = [(j11 * dxi[a] - j01 * deta[a]) * idet for a in range(4)]
        ny = [(j00 * deta[a] - j10 * dxi[a]) * idet for a in range(4)]
        gx, gy = u.zero(), u.zero()
        for a in range(4):
            gx = gx + nx[a] * u.at(a)
            gy = gy + ny[a] * u.at(a)
        k = gpow(p[1] + (gx * gx + gy * gy), p[0]) * wd
        for a in range(4):
            f[a] = f[a] + (k * (gx * nx[a] + gy * ny[a]) - (wd * N[a]) * u.x(a, 2))
    return f


# ------------------------------------------------------------------------------------------------ P1 tetrahedra
TETDIFF_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  nk_real d[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d[a][k] = u.x(a + 1, k) - u.x(0, k);
  }
  nk_real gN[4][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    gN[a + 1][0] = d[b][1] * d[c][2] - d[b][2] * d[c][1];
    gN[a + 1][1] = d[b][2] * d[c][0] - d[b][0] * d[c][2];
    gN[a + 1][2] = d[b][0] * d[c][1] - d[b][1] * d[c][0];
  }
  const nk_real det = (d[0][0] * gN[1][0] + d[0][1] * gN[1][1]) + d[0][2] * gN[1][2], id = 1.0 / det, vol = fabs(det) * (1.0 / 6.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int a = 1; a < 4; ++a) gN[a][k] = gN[a][k] * id;
    gN[0][k] = -((gN[1][k] + gN[2][k]) + gN[3][k]);
  }
  T g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = ((gN[0][k] * u.at(0) + gN[1][k] * u.at(1)) + gN[2][k] * u.at(2)) + gN[3][k] * u.at(3);
  const T ub = (((u.at(0) + u.at(1)) + u.at(2)) + u.at(3)) * 0.25;
  const T kk = (1.0 + p[0] * (ub * ub)) * (u.w(0) * vol);
#pragma unroll
  for (int a = 0; a < 4; ++a) f[a] = kk * ((g[0] * gN[a][0] + g[1] * gN[a][1]) + g[2] * gN[a][2]) - (0.25 * vol) * u.x(a, 3);
}
"""


def _tetdiff(u, p, s):
    d = [[u.x(a + 1, k) - u.x(0, k) for k in range(3)] for a in range(3)]
    gN = [None] * 4
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        gN[a + 1] = [d[b][1] * d[c][2] - d[b][2] * d[c][1], d[b][2] * d[c][0] - d[b][0] * d[c][2], d[b][0] * d[c][1] - d[b][1] * d[c][0]]
    det = (d[0][0] * gN[1][0] + d[0][1] * gN[1][1]) + d[0][2] * gN[1][2]
    idet, vol = 1.0 / det, abs(det) * (1.0 / 6.0)
    gN[0] = [None] * 3
    for k in range(3):
        for a in range(1, 4):
            gN[a][k] = gN[a][k] * idet
        gN[0][k] = -((gN[1][k] + gN[2][k]) + gN[3][k])
    g = [((gN[0][k] * u.at(0) + gN[1][k] * u.at(1)) + gN[2][k] * u.at(2)) + gN[3][k] * u.at(3) for k in range(3)]
    ub = (((u.at(0) + u.at(1)) + u.at(2)) + u.at(3)) * 0.25
    kk = (1.0 + p[0] * (ub * ub)) * (u.w(0) * vol)
    return [kk * ((g[0] * gN[a][0] + g[1] * gN[a][1]) + g[2] * gN[a][2]) - (0.25 * vol) * u.x(a, 3) for a in range(4)]


# ------------------------------------------------------------------------------------------------ truss
TRUSS_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  const nk_real X = u.x(1, 0) - u.x(0, 0), Y = u.x(1, 1) - u.x(0, 1), l0 = sqrt(X * X + Y * Y), h = 0.5 * l0;
  const T dx = (u.at(1, 0) - u.at(0, 0)) + X, dy = (u.at(1, 1) - u.at(0, 1)) + Y;
  const T l = sqrt(dx * dx + dy * dy);
  const T n = ((u.w(0) * (1.0 / l0)) * (l - l0)) / l;
  const T fx = n * dx, fy = n * dy;
  f[0] = (-fx) - h * p[0];
  f[1] = (-fy) - h * p[1];
  f[2] = fx - h * p[0];
  f[3] = fy - h * p[1];
}
"""


def _truss(u, p, s):
    X, Y = u.x(1, 0) - u.x(0, 0), u.x(1, 1) - u.x(0, 1)
    l0 = gsqrt(X * X + Y * Y)
    h = 0.5 * l0
    dx, dy = (u.at(1, 0) - u.at(0, 0)) + X, (u.at(1, 1) - u.at(0, 1)) + Y
    ln = gsqrt(dx * dx + dy * dy)
    n = gdiv((u.w(0) * (1.0 / l0)) * (ln - l0), ln)
    fx, fy = n * dx, n * dy
    return [(-fx) - h * p[0], (-fy) - h * p[1], fx - h * p[0], fy - h * p[1]]


# ------------------------------------------------------------------------------------------------ quad4 and hex8
QUAD4_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  T m[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) m[c] = (((u.at(0, c) + u.at(1, c)) + u.at(2, c)) + u.at(3, c)) * 0.25;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int n = (c + 1) % 4;
      const T uc = u.at(a, c);
      f[4 * a + c] = u.w(0) * ((uc - m[c]) * m[n]) + 0.25 * ((uc * u.at(a, n) + p[0] * uc) - 1.0);
    }
  }
}
"""


def _quad4(u, p, s):
    m = [(((u.at(0, c) + u.at(1, c)) + u.at(2, c)) + u.at(3, c)) * 0.25 for c in range(4)]
    out = []
    for a in range(4):
        for c in range(4):
            n = (c + 1) % 4
            uc = u.at(a, c)
            out.append(u.w(0) * ((uc - m[c]) * m[n]) + 0.25 * ((uc * u.at(a, n) + p[0] * uc) - 1.0))
    return out


HEX8_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  T m = u.at(0);
#pragma unroll
  for (int a = 1; a < 8; ++a) m = m + u.at(a);
  m = m * 0.125;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const T d = u.at(a) - m;
    f[a] = u.w(0) * (d + p[0] * (d * d * d)) + 0.125 * (p[1] * u.at(a) - u.x(a, 0));
  }
}
"""


def _hex8(u, p, s):
    m = u.at(0)
    for a in range(1, 8):
        m = m + u.at(a)
    m = m * 0.125
    out = []
    for a in range(8):
        d = u.at(a) - m
        out.append(u.w(0) * (d + p[0] * (d * d * d)) + 0.125 * (p[1] * u.at(a) - u.x(a, 0)))
    return out


# ------------------------------------------------------------------------------------------------ indexed
INDEXED_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
#pragma unroll
  for (int a = 0; a < NK_NPE; ++a) {
    const int b = (a + 1) % NK_NPE;
    const nk_real c = (nk_real)(1 + (u.node(a) + s.e) % 7) + u.x(a, 0) * u.w(0);
    f[a] = c * (u.at(a) * u.at(b)) + ((nk_real)(u.node(b) % 5) * u.at(a) - (nk_real)((s.e + s.ne + s.nn) % 3));
  }
}
"""


def _indexed(u, p, s):
    out = []
    for a in range(u.npe):
        b = (a + 1) % u.npe
        c = u.real(1 + (u.node(a) + s.e) % 7) + u.x(a, 0) * u.w(0)
        out.append(c * (u.at(a) * u.at(b)) + (u.real(u.node(b) % 5) * u.at(a) - u.real((s.e + s.ne + s.nn) % 3)))
    return out


# ------------------------------------------------------------------------------------------------ the table
SOURCE, KAPPA = (-1.0, 1.0), (0.5, 1.5)
PROBLEMS = {
    "diffusion": Problem("diffusion", DIFFUSION_SRC, 3, 1, [], _diffusion, ["x", "y", SOURCE]),
    "bratu": Problem("bratu", BRATU_SRC, 3, 1, [1.0], _bratu, ["x", "y"]),
    "react2": Problem("react2", REACT2_SRC, 3, 2, [0.5, 0.3, 1.5], _react2, ["x", "y"]),
    "plap": Problem("plap", PLAP_SRC, 4, 1, [0.5, 0.1], _plap, ["x", "y", SOURCE]),
    "tetdiff": Problem("tetdiff", TETDIFF_SRC, 4, 1, [0.5], _tetdiff, ["x", "y", "z", SOURCE], [KAPPA]),
    "truss": Problem("truss", TRUSS_SRC, 2, 2, [0.0, -0.02], _truss, ["x", "y"], [(50.0, 100.0)]),
    "quad4": Problem("quad4", QUAD4_SRC, 4, 4, [1.5], _quad4, [], [KAPPA]),
    "hex8": Problem("hex8", HEX8_SRC, 8, 1, [2.0, 0.5], _hex8, [SOURCE], [KAPPA]),
}
for _npe in (2, 3, 4, 8):
    PROBLEMS[f"indexed{_npe}"] = Problem(f"indexed{_npe}", INDEXED_SRC, _npe, 1, [], _indexed, [("int", -3, 3)], [("int", -2, 2)])
EXACT = ("indexed2", "indexed3", "indexed4", "indexed8")   # no elementary function, integer data: bit for bit

PAIRS = [(p, m) for p in ("diffusion", "bratu", "react2", "indexed3") for m in TRIANGLES] + \
        [("plap", "quad7x5"), ("quad4", "quad7x5"), ("indexed4", "quad7x5"), ("tetdiff", "tet3x3x2"), ("indexed4", "tet3x3x2"),
         ("hex8", "hex3x2x2"), ("indexed8", "hex3x2x2"), ("truss", "truss"), ("indexed2", "truss")]
CASES = [(p, m, masked) for p, m in PAIRS for masked in (False, True)]

# a source written against the grid contract, one that does not parse, and one that reads data beyond the declared count
GRID_CONTRACT_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) { f[0] = u(0, 0); }
"""
SYNTAX_ERROR_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) { f[0] = no_such_symbol(u.at(0)); }
"""
UNDECLARED_DATA_SRC = r"""
template <typename T>
__device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f) {
  f[0] = u.at(0) + u.x(0, 1);
  f[1] = u.at(1) + u.w(0);
  f[2] = u.at(2) + u.at(3);
}
"""
