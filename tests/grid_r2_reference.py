"""NumPy restatement of the compiled grid problems with a radius-2 stencil (csrc/nk_grid.hip: NK_GRID_STAR2 in 2-D and 3-D,
NK_GRID_DIAMOND2 in 2-D), in the style of tests/grid_reference.py and tests/grid3_reference.py:
eight pointwise problems, each written once as HIP source (what the library compiles) and once as NumPy formulas with their
ANALYTIC derivatives, evaluated in float64 and in long double. From the formulas: the residual, J·v (the tangent written out by
hand, term for term in the source's order), the values of J on the pattern, Jᵀv, and for every entry the gap
|float64 − long double| and the sum of the absolute values of the entry's terms — the bound the device tests use:

    |device − float64 restatement| <= 16 × gap + 4 eps × Σ|terms|

One code for both dimensions: a shape is (nx, ny) or (nx, ny, nz), an offset (di, dj) or (di, dj, dk). Layout: unknown c of
node (i, j[, k]) is element c·nn + ((k·ny) + j)·nx + i. Seeded inputs have |u| <= 1. A Dirichlet neighbour up to two layers
outside the grid reads 0 and has no column; a periodic index wraps by ± n.
Stencil points in pattern order (ascending node index inside the grid):
star2, 2-D     (0,−2) (0,−1) (−2,0) (−1,0) C (1,0) (2,0) (0,1) (0,2)
diamond2, 2-D  (0,−2) (−1,−1) (0,−1) (1,−1) (−2,0) (−1,0) C (1,0) (2,0) (−1,1) (0,1) (1,1) (0,2)
star2, 3-D     (0,0,−2) (0,0,−1) (0,−2,0) (0,−1,0) (−2,0,0) (−1,0,0) C (1,0,0) (2,0,0) (0,1,0) (0,2,0) (0,0,1) (0,0,2)
This module is the table: sources, formulas, problems and sizes. The pattern, the access to u and v, the evaluation in both
arithmetics and the bound are tests/grid_core.py's."""
import numpy as np

from grid_core import STENCILS, Problem, _site, _sum, _wsum

DIAMOND2 = STENCILS[(2, "diamond2")]
PERMITTED = [(2, "star2", 1), (2, "star2", 2), (2, "diamond2", 1), (3, "star2", 1), (3, "star2", 2)]   # (dim, stencil, dof)
# the off-centre points of the stars in the order the sources add them: per direction −1 +1 −2 +2
EIGHT = [(-1, 0), (1, 0), (-2, 0), (2, 0), (0, -1), (0, 1), (0, -2), (0, 2)]
TWELVE = [o + (0,) for o in EIGHT] + [(0, 0, -1), (0, 0, 1), (0, 0, -2), (0, 0, 2)]
NEAR2, FAR2 = [(-1, 0), (1, 0), (0, -1), (0, 1)], [(-2, 0), (2, 0), (0, -2), (0, 2)]
DIAG2 = [(-1, -1), (1, -1), (-1, 1), (1, 1)]
NEAR3 = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
FAR3 = [(-2, 0, 0), (2, 0, 0), (0, -2, 0), (0, 2, 0), (0, 0, -2), (0, 0, 2)]


def _args(dim):
    return ("nk_nbhd<T>", "nk_site") if dim == 2 else ("nk_nbhd3<T>", "nk_site3")


def _head(dim):
    return "template <typename T>\n__device__ void nk_point(const %s &u, const nk_real *p, %s s, T *f) {\n" % _args(dim)


def _u(off, c=None):
    return "u(" + ", ".join(str(d) for d in off) + ("" if c is None else f", {c}") + ")"


# ------------------------------------------------------------------------------------------------ lap4, lap4_3
# Bratu with the fourth-order Laplacian, scaled by 12h²: F = c_lap·(60u − 16·Σ(±1) + Σ(±2)) − c_exp·eᵘ in 2-D (90u in 3-D);
# p = {c_lap, c_exp} = {1, 12h²λ}, h = 1/(nx + 1)
def _lap4_src(dim):
    near, far, diag = (NEAR2, FAR2, "60.0") if dim == 2 else (NEAR3, FAR3, "90.0")
    z = (0,) * dim
    return (_head(dim) + f"  const T c = {_u(z)};\n"
            + "  const T s1 = " + " + ".join(_u(o) for o in near) + ";\n"
            + "  const T s2 = " + " + ".join(_u(o) for o in far) + ";\n"
            + f"  f[0] = p[0] * ({diag} * c - 16.0 * s1 + s2) - p[1] * exp(c);\n}}\n")


LAP4_SRC, LAP4_3_SRC = _lap4_src(2), _lap4_src(3)


def lap4_params(nx, lam=3.0):
    """−Δu = λ eᵘ with the fourth-order Laplacian and mesh width h = 1/(nx + 1) in every direction, scaled by 12h²"""
    h = 1.0 / (nx + 1)
    return [1.0, 12.0 * (h * h) * lam]


def _lap4_lin(N, T):
    dim = N.dim
    near, far, diag = (NEAR2, FAR2, 60) if dim == 2 else (NEAR3, FAR3, 90)
    c = N(*(0,) * dim)
    s1, m1 = _sum([N(*o) for o in near])
    s2, m2 = _sum([N(*o) for o in far])
    return T(diag) * c - T(16) * s1 + s2, T(diag) * np.abs(c) + T(16) * m1 + m2


def _lap4_resid(N, _A, p, shape, T):
    lap, ml = _lap4_lin(N, T)
    e = p[1] * np.exp(N(*(0,) * N.dim))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _lap4_jvp(N, V, _A, p, shape, T):
    z = (0,) * N.dim
    lap, ml = _lap4_lin(V, T)
    e = p[1] * (np.exp(N(*z)) * V(*z))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _lap4_jac(N, _A, p, shape, T):
    dim = N.dim
    near, far, diag = (NEAR2, FAR2, 60) if dim == 2 else (NEAR3, FAR3, 90)
    z = (0,) * dim
    c = N(*z)
    one = np.ones_like(c)
    e = p[1] * np.exp(c)
    J = {(0, *z, 0): (p[0] * T(diag) - e, np.abs(p[0] * T(diag)) + np.abs(e))}
    for o in near:
        J[(0, *o, 0)] = (-(p[0] * T(16)) * one, np.abs(p[0] * T(16)) * one)
    for o in far:
        J[(0, *o, 0)] = (p[0] * one, np.abs(p[0]) * one)
    return J


# ------------------------------------------------------------------------------------------------ upwind2, upwind3
# two components on the star, m = 8 (2-D) or 12 (3-D) off-centre points in the order EIGHT / TWELVE:
#   f0 = Σ p[t]·a(off t)     − p[2m]·a     + p[2m+2]·(a·b) + g
#   f1 = Σ p[m + t]·b(off t) − p[2m + 1]·b − p[2m+2]·(a·b)
# a different weight for every point AND component (a third-order upwind difference has one per direction, sign and distance),
# so a swapped +2 / −2, ±1 / ±2 or i / j changes the answer. No elementary function. The forcing g = p[2m+3]·(…) reads all of
# the site; it is computed in double in both arithmetics, as the source computes it.
def _upwind_src(dim):
    offs = EIGHT if dim == 2 else TWELVE
    m, z = len(offs), (0,) * dim
    if dim == 2:
        site = ("  const nk_real x = (nk_real)s.i / (nk_real)s.nx, y = (nk_real)s.j / (nk_real)s.ny;\n"
                f"  const nk_real g = p[{2 * m + 3}] * (x + 2.0 * y);\n")
    else:
        site = ("  const nk_real x = (nk_real)s.i / (nk_real)s.nx, y = (nk_real)s.j / (nk_real)s.ny, "
                "z = (nk_real)s.k / (nk_real)s.nz;\n"
                f"  const nk_real g = p[{2 * m + 3}] * ((x + 2.0 * y) * z + 0.25 * x - 0.5 * y);\n")
    src = _head(dim) + site + f"  const T a = {_u(z, 0)}, b = {_u(z, 1)};\n"
    for c, nm in ((0, "la"), (1, "lb")):
        src += f"  const T {nm} = " + " + ".join(f"p[{c * m + t}] * {_u(o, c)}" for t, o in enumerate(offs))
        src += f" - p[{2 * m + c}] * {'ab'[c]};\n"
    src += f"  const T ab = p[{2 * m + 2}] * (a * b);\n  f[0] = la + ab + g;\n  f[1] = lb - ab;\n}}\n"
    return src


UPWIND2_SRC, UPWIND3_SRC = _upwind_src(2), _upwind_src(3)
UPWIND2_PARAMS = ([11.0, 7.5, -2.25, 1.5, 9.25, 6.0, -3.0, 0.75] + [5.5, 12.0, 1.25, -1.75, 4.0, 10.5, 0.5, -2.5]
                  + [31.0, 27.0, 0.875, 1.5])
UPWIND3_PARAMS = ([11.0, 7.5, -2.25, 1.5, 9.25, 6.0, -3.0, 0.75, 13.5, 4.75, -1.25, 2.0]
                  + [5.5, 12.0, 1.25, -1.75, 4.0, 10.5, 0.5, -2.5, 8.0, 3.5, 2.75, -0.625] + [52.0, 47.0, 0.875, 1.5])


def _upwind_forcing(p, shape, T):
    at, m = _site(shape), (8 if len(shape) == 2 else 12)
    x, y = at[0] / np.float64(shape[0]), at[1] / np.float64(shape[1])
    if len(shape) == 2:
        g = np.float64(p[2 * m + 3]) * (x + 2.0 * y)
    else:
        z = at[2] / np.float64(shape[2])
        g = np.float64(p[2 * m + 3]) * ((x + 2.0 * y) * z + 0.25 * x - 0.5 * y)
    return g.astype(T)


def _upwind_lin(N, p, c):
    dim = N.dim
    offs = EIGHT if dim == 2 else TWELVE
    m = len(offs)
    s, ms = _wsum(N, offs, p[c * m:(c + 1) * m], c)
    t = p[2 * m + c] * N(*(0,) * dim, c)
    return s - t, ms + np.abs(t)


def _upwind_resid(N, _A, p, shape, T):
    m, z = (8 if N.dim == 2 else 12), (0,) * N.dim
    la, ma = _upwind_lin(N, p, 0)
    lb, mb = _upwind_lin(N, p, 1)
    ab = p[2 * m + 2] * (N(*z, 0) * N(*z, 1))
    g = _upwind_forcing(p, shape, T)
    return [la + ab + g, lb - ab], [ma + np.abs(ab) + np.abs(g), mb + np.abs(ab)]


def _upwind_jvp(N, V, _A, p, shape, T):
    m, z = (8 if N.dim == 2 else 12), (0,) * N.dim
    la, ma = _upwind_lin(V, p, 0)
    lb, mb = _upwind_lin(V, p, 1)
    a, b, da, db = N(*z, 0), N(*z, 1), V(*z, 0), V(*z, 1)
    t1, t2 = da * b, a * db                          # the dual's product rule in the source's order
    d = (t1 + t2) * p[2 * m + 2]
    md = (np.abs(t1) + np.abs(t2)) * np.abs(p[2 * m + 2])
    return [la + d, lb - d], [ma + md, mb + md]


def _upwind_jac(N, _A, p, shape, T):
    dim = N.dim
    offs = EIGHT if dim == 2 else TWELVE
    m, z = len(offs), (0,) * dim
    a, b = N(*z, 0), N(*z, 1)
    one = np.ones_like(a)
    k = p[2 * m + 2]
    J = {
        (0, *z, 0): (-p[2 * m] + b * k, np.abs(p[2 * m]) + np.abs(b * k)),
        (0, *z, 1): (a * k, np.abs(a * k)),
        (1, *z, 1): (-p[2 * m + 1] - a * k, np.abs(p[2 * m + 1]) + np.abs(a * k)),
        (1, *z, 0): (-(b * k), np.abs(b * k)),
    }
    for t, o in enumerate(offs):
        for c in (0, 1):
            J[(c, *o, c)] = (p[c * m + t] * one, np.abs(p[c * m + t]) * one)
    return J


# ------------------------------------------------------------------------------------------------ sh
# Swift–Hohenberg steady state r·u − (1 + ∇²)²u − u³ = (r − 1)u − 2∇²u − ∇⁴u − u³ with the 5-point Laplacian and the 13-point
# biharmonic (weights 20 / −8 / 2 / 1); p = {r, 1/h², 1/h⁴}. Periodic; no elementary function. Its Jacobian may be singular.
SH_SRC = (_head(2) + "  const T c = u(0, 0);\n"
          + "  const T s1 = " + " + ".join(_u(o) for o in NEAR2) + ";\n"
          + "  const T sd = " + " + ".join(_u(o) for o in DIAG2) + ";\n"
          + "  const T s2 = " + " + ".join(_u(o) for o in FAR2) + ";\n"
          + "  const T lap = p[1] * (s1 - 4.0 * c);\n"
          + "  const T bih = p[2] * (20.0 * c - 8.0 * s1 + 2.0 * sd + s2);\n"
          + "  f[0] = (p[0] - 1.0) * c - 2.0 * lap - bih - c * c * c;\n}\n")
SH_PARAMS = [0.3, 1.5, 2.25]


def _sh_lin(N, p, T):
    c = N(0, 0)
    s1, m1 = _sum([N(*o) for o in NEAR2])
    sd, md = _sum([N(*o) for o in DIAG2])
    s2, m2 = _sum([N(*o) for o in FAR2])
    lap, mlap = p[1] * (s1 - T(4) * c), np.abs(p[1]) * (m1 + T(4) * np.abs(c))
    bih = p[2] * (T(20) * c - T(8) * s1 + T(2) * sd + s2)
    mbih = np.abs(p[2]) * (T(20) * np.abs(c) + T(8) * m1 + T(2) * md + m2)
    t0 = (p[0] - T(1)) * c
    return t0 - T(2) * lap - bih, np.abs(t0) + T(2) * mlap + mbih


def _sh_resid(N, _A, p, shape, T):
    c = N(0, 0)
    lin, ml = _sh_lin(N, p, T)
    c3 = c * c * c
    return [lin - c3], [ml + np.abs(c3)]


def _sh_jvp(N, V, _A, p, shape, T):
    c, dc = N(0, 0), V(0, 0)
    lin, ml = _sh_lin(V, p, T)
    t1, t2, t3 = dc * c, c * dc, (c * c) * dc         # d(c·c) = dc·c + c·dc ; d((c·c)·c) = d(c·c)·c + (c·c)·dc
    d3 = (t1 + t2) * c + t3
    return [lin - d3], [ml + (np.abs(t1) + np.abs(t2)) * np.abs(c) + np.abs(t3)]


def _sh_jac(N, _A, p, shape, T):
    c = N(0, 0)
    one = np.ones_like(c)
    d3 = (c + c) * c + c * c
    J = {(0, 0, 0, 0): ((p[0] - T(1)) - (T(-4) * p[1]) * T(2) - T(20) * p[2] - d3,
                        np.abs(p[0] - T(1)) + np.abs(T(8) * p[1]) + np.abs(T(20) * p[2]) + np.abs((c + c) * c) + np.abs(c * c))}
    for o in NEAR2:
        J[(0, *o, 0)] = ((-(T(2) * p[1]) - T(-8) * p[2]) * one, (np.abs(T(2) * p[1]) + np.abs(T(8) * p[2])) * one)
    for o in DIAG2:
        J[(0, *o, 0)] = (-(T(2) * p[2]) * one, np.abs(T(2) * p[2]) * one)
    for o in FAR2:
        J[(0, *o, 0)] = (-p[2] * one, np.abs(p[2]) * one)
    return J


# ------------------------------------------------------------------------------------------------ diamond_dirichlet
# f = Σ over the 13 offsets of (p0 + p1·(di + 5 dj))·u(di, dj) + p2·u³: thirteen distinct weights, made in the source, in
# pattern order
DIAMOND_SRC = _head(2) + r"""  T acc = T(0.0);
#pragma unroll
  for (int dj = -2; dj <= 2; ++dj) {
#pragma unroll
    for (int di = -2; di <= 2; ++di) {
      if ((di < 0 ? -di : di) + (dj < 0 ? -dj : dj) <= 2) {
        const nk_real w = p[0] + p[1] * (nk_real)(di + 5 * dj);
        acc = acc + w * u(di, dj);
      }
    }
  }
  const T c = u(0, 0);
  f[0] = acc + p[2] * c * c * c;
}
"""
DIAMOND_PARAMS = [0.3, 0.0625, 0.5]


def _diamond_w(p, T):
    return [p[0] + p[1] * T(di + 5 * dj) for (di, dj) in DIAMOND2]


def _diamond_resid(N, _A, p, shape, T):
    acc, m = _wsum(N, DIAMOND2, _diamond_w(p, T), 0)
    c = N(0, 0)
    e = ((p[2] * c) * c) * c
    return [acc + e], [m + np.abs(e)]


def _diamond_jvp(N, V, _A, p, shape, T):
    acc, m = _wsum(V, DIAMOND2, _diamond_w(p, T), 0)
    c, dc = N(0, 0), V(0, 0)
    t1, t2, t3 = (dc * p[2]) * c, (p[2] * c) * dc, ((p[2] * c) * c) * dc     # the dual's product rule in the source's order
    e = (t1 + t2) * c + t3
    return [acc + e], [m + (np.abs(t1) + np.abs(t2)) * np.abs(c) + np.abs(t3)]


def _diamond_jac(N, _A, p, shape, T):
    c = N(0, 0)
    one = np.ones_like(c)
    w = _diamond_w(p, T)
    J = {}
    for t, o in enumerate(DIAMOND2):
        J[(0, *o, 0)] = (w[t] * one, np.abs(w[t]) * one)
    t1, t3 = p[2] * c, (p[2] * c) * c
    e = (t1 + t1) * c + t3
    J[(0, 0, 0, 0)] = (w[6] + e, np.abs(w[6]) + np.abs((t1 + t1) * c) + np.abs(t3))
    return J


# ------------------------------------------------------------------------------------------------ the cases
_UP = (_upwind_resid, _upwind_jvp, _upwind_jac)
PROBLEMS = {
    "lap4": Problem("lap4", LAP4_SRC, 2, 1, "star2", "dirichlet", [1.0, 0.04], _lap4_resid, _lap4_jvp, _lap4_jac),
    "upwind2_dirichlet": Problem("upwind2_dirichlet", UPWIND2_SRC, 2, 2, "star2", "dirichlet", UPWIND2_PARAMS, *_UP),
    "upwind2_periodic": Problem("upwind2_periodic", UPWIND2_SRC, 2, 2, "star2", "periodic", UPWIND2_PARAMS, *_UP),
    "sh": Problem("sh", SH_SRC, 2, 1, "diamond2", "periodic", SH_PARAMS, _sh_resid, _sh_jvp, _sh_jac),
    "diamond_dirichlet": Problem("diamond_dirichlet", DIAMOND_SRC, 2, 1, "diamond2", "dirichlet", DIAMOND_PARAMS, _diamond_resid,
                                 _diamond_jvp, _diamond_jac),
    "lap4_3": Problem("lap4_3", LAP4_3_SRC, 3, 1, "star2", "dirichlet", [1.0, 0.04], _lap4_resid, _lap4_jvp, _lap4_jac),
    "upwind3_dirichlet": Problem("upwind3_dirichlet", UPWIND3_SRC, 3, 2, "star2", "dirichlet", UPWIND3_PARAMS, *_UP),
    "upwind3_periodic": Problem("upwind3_periodic", UPWIND3_SRC, 3, 2, "star2", "periodic", UPWIND3_PARAMS, *_UP),
}
# 5 × 5: every periodic row wraps in both layers both ways, every Dirichlet node misses points; 37 × 29 = 1073 nodes: five
# workgroups, the last ragged; 300 × 5: a wavefront spans lines
SIZES2 = [(5, 5), (37, 29), (300, 5)]
# 37 × 29 × 5: planes of 1073 nodes; 5 × 5 × 70: a wavefront spans planes
SIZES3 = [(5, 5, 5), (7, 6, 5), (37, 29, 5), (5, 5, 70)]
SIZES = {2: SIZES2, 3: SIZES3}
# sources that read an offset outside their stencil's shape: the residual is NaN at every node
OUTSIDE_SRC = {
    "star2": _head(2) + "  f[0] = 4.0 * u(0, 0) - u(1, 1) - u(-2, 0);\n}\n",
    "diamond2": _head(2) + "  f[0] = 4.0 * u(0, 0) - u(2, 1) - u(-1, -1);\n}\n",
    "star2_3": _head(3) + "  f[0] = 6.0 * u(0, 0, 0) - u(1, 1, 0) - u(0, 0, -2);\n}\n",
}
SYNTAX_ERROR_SRC = _head(2) + "  f[0] = u(0, 2) * no_such_symbol;\n}\n"
