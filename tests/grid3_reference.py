"""NumPy restatement of the compiled grid problems in three dimensions (csrc/nk_grid.hip, nk_problem_create_grid3), in the
style of tests/grid_reference.py: four pointwise problems — Bratu, a Brusselator with upwinded
(direction- and sign-dependent) weights and a site-dependent forcing, a 27-point box problem with 27 distinct coefficients, a
four-component star problem coupled at the centre — each written once as HIP source (what the library compiles) and once as
NumPy formulas with their ANALYTIC derivatives, evaluated in float64 and in long double. From the formulas: the residual, J·v
(the tangent written out by hand, term for term in the source's order), the values of J on the pattern, Jᵀv, and for every
entry the gap |float64 − long double| and the sum of the absolute values of the entry's terms — the bound the device tests use:

    |device − float64 restatement| <= 16 × gap + 4 eps × Σ|terms|

Layout: unknown c of node (i, j, k) is element c·nx·ny·nz + (k·ny + j)·nx + i. Seeded inputs have |u| <= 1.
Stencil points in pattern order (ascending node index inside the grid), as (di, dj, dk):
star (0,0,−1) (0,−1,0) (−1,0,0) C (1,0,0) (0,1,0) (0,0,1); box dk outermost, di innermost.
This module is the table: sources, formulas, problems and sizes. The pattern, the access to u and v, the evaluation in both
arithmetics and the bound are tests/grid_core.py's."""
import numpy as np

from grid_core import STENCILS, Problem, _site, _sum, _wsum

BOX = STENCILS[(3, "box")]
PERMITTED = [("star", 1), ("star", 2), ("star", 3), ("star", 4), ("box", 1)]                # (stencil, dof)
# the six neighbours in the order the sources add them: −i +i −j +j −k +k
SIX = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


# ------------------------------------------------------------------------------------------------ bratu3
# F = c_lap·(6u − Σ six neighbours) − c_exp·eᵘ ;  p = {c_lap, c_exp}
BRATU3_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  const T c = u(0, 0, 0);
  f[0] = p[0] * (6.0 * c - u(-1, 0, 0) - u(1, 0, 0) - u(0, -1, 0) - u(0, 1, 0) - u(0, 0, -1) - u(0, 0, 1)) - p[1] * exp(c);
}
"""


def bratu3_params(nx, lam=3.0):
    """−Δu = λ eᵘ with mesh width h = 1/(nx + 1) in all three directions, scaled by h²: c_lap = 1, c_exp = h²λ. The box
    (nx+1)h × (ny+1)h × (nz+1)h lies inside the unit cube when ny, nz <= nx, and a smaller box has a LARGER turning point than
    the unit cube's λ* ≈ 9.9: λ = 3 is well below it."""
    h = 1.0 / (nx + 1)
    return [1.0, (h * h) * lam]


def _bratu3_lap(N, T):
    return _sum([T(6) * N(0, 0, 0)] + [-N(*o) for o in SIX])


def _bratu3_resid(N, _A, p, shape, T):
    lap, ml = _bratu3_lap(N, T)
    e = p[1] * np.exp(N(0, 0, 0))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu3_jvp(N, V, _A, p, shape, T):
    lap, ml = _bratu3_lap(V, T)
    e = p[1] * (np.exp(N(0, 0, 0)) * V(0, 0, 0))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu3_jac(N, _A, p, shape, T):
    c = N(0, 0, 0)
    one = np.ones_like(c)
    e = p[1] * np.exp(c)
    J = {(0, 0, 0, 0, 0): (p[0] * T(6) - e, np.abs(p[0] * T(6)) + np.abs(e))}
    for o in SIX:
        J[(0, *o, 0)] = (-p[0] * one, np.abs(p[0]) * one)
    return J


# ------------------------------------------------------------------------------------------------ brusselator3
# p = {A, B, w(−i), w(+i), w(−j), w(+j), w(−k), w(+k), w_centre}: an upwinded advection–diffusion operator has a different
# weight per direction AND per sign, so a swapped +k / −k or j / k changes the answer. No elementary function. The forcing
# depends on the site and on all three sizes; it is decided in double in both arithmetics, as the source decides it.
BRUSSELATOR3_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  const nk_real A = p[0], B = p[1];
  const nk_real x = (nk_real)s.i / (nk_real)s.nx, y = (nk_real)s.j / (nk_real)s.ny, z = (nk_real)s.k / (nk_real)s.nz;
  const nk_real bf = (x + 2.0 * y) * z + 0.25 * x - 0.5 * y;
  const T uu = u(0, 0, 0, 0), vv = u(0, 0, 0, 1);
  const T lu = p[2] * u(-1, 0, 0, 0) + p[3] * u(1, 0, 0, 0) + p[4] * u(0, -1, 0, 0) + p[5] * u(0, 1, 0, 0)
             + p[6] * u(0, 0, -1, 0) + p[7] * u(0, 0, 1, 0) - p[8] * uu;
  const T lv = p[2] * u(-1, 0, 0, 1) + p[3] * u(1, 0, 0, 1) + p[4] * u(0, -1, 0, 1) + p[5] * u(0, 1, 0, 1)
             + p[6] * u(0, 0, -1, 1) + p[7] * u(0, 0, 1, 1) - p[8] * vv;
  f[0] = lu + B + uu * uu * vv - (A + 1.0) * uu + bf;
  f[1] = lv + A * uu - uu * uu * vv;
}
"""
BRUSSELATOR3_PARAMS = [3.4, 1.0, 11.0, 7.5, 9.25, 6.0, 13.5, 4.75, 52.0]


def _brus3_forcing(shape, T):
    nx, ny, nz = shape
    i, j, k = _site(shape)
    x, y, z = i / np.float64(nx), j / np.float64(ny), k / np.float64(nz)
    return ((x + 2.0 * y) * z + 0.25 * x - 0.5 * y).astype(T)


def _brus3_lap(N, p, c):
    s, m = _wsum(N, SIX, p[2:8], c)
    t = p[8] * N(0, 0, 0, c)
    return s - t, m + np.abs(t)


def _brus3_resid(N, _A, p, shape, T):
    A, B = p[0], p[1]
    uu, vv = N(0, 0, 0, 0), N(0, 0, 0, 1)
    lu, mu = _brus3_lap(N, p, 0)
    lv, mv = _brus3_lap(N, p, 1)
    bf = _brus3_forcing(shape, T)
    f0, m0 = _sum([lu, B * np.ones_like(uu), uu * uu * vv, -((A + T(1)) * uu), bf])
    f1, m1 = _sum([lv, A * uu, -(uu * uu * vv)])
    return [f0, f1], [m0 - np.abs(lu) + mu, m1 - np.abs(lv) + mv]


def _brus3_jvp(N, V, _A, p, shape, T):
    A = p[0]
    uu, vv, a, b = N(0, 0, 0, 0), N(0, 0, 0, 1), V(0, 0, 0, 0), V(0, 0, 0, 1)
    la, ma = _brus3_lap(V, p, 0)
    lb, mb = _brus3_lap(V, p, 1)
    # the dual's product rule, in the source's order: d(uu·uu) = a·uu + uu·a ; d((uu·uu)·vv) = d(uu·uu)·vv + (uu·uu)·b
    duu = a * uu + uu * a
    d3 = duu * vv + (uu * uu) * b
    m3 = np.abs(a * uu) * 2 * np.abs(vv) + np.abs((uu * uu) * b)
    t4 = (A + T(1)) * a
    return [la + d3 - t4, lb + A * a - d3], [ma + m3 + np.abs(t4), mb + np.abs(A * a) + m3]


def _brus3_jac(N, _A, p, shape, T):
    A = p[0]
    uu, vv = N(0, 0, 0, 0), N(0, 0, 0, 1)
    one = np.ones_like(uu)
    two_uv = (uu + uu) * vv
    J = {
        (0, 0, 0, 0, 0): (-p[8] + two_uv - (A + T(1)), np.abs(p[8]) + np.abs(two_uv) + np.abs(A + T(1))),
        (0, 0, 0, 0, 1): (uu * uu, uu * uu),
        (1, 0, 0, 0, 1): (-p[8] - uu * uu, np.abs(p[8]) + uu * uu),
        (1, 0, 0, 0, 0): (A - two_uv, np.abs(A) + np.abs(two_uv)),
    }
    for t, o in enumerate(SIX):
        for c in (0, 1):
            J[(c, *o, c)] = (p[2 + t] * one, np.abs(p[2 + t]) * one)
    return J


# ------------------------------------------------------------------------------------------------ box3
# f = Σ over the 27 offsets of (p0 + p1·(di + 3 dj + 9 dk))·u(di, dj, dk) + p2·u²: 27 distinct coefficients, made in the source
BOX3_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  T acc = T(0.0);
#pragma unroll
  for (int dk = -1; dk <= 1; ++dk) {
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
#pragma unroll
      for (int di = -1; di <= 1; ++di) {
        const nk_real w = p[0] + p[1] * (nk_real)(di + 3 * dj + 9 * dk);
        acc = acc + w * u(di, dj, dk);
      }
    }
  }
  const T c = u(0, 0, 0);
  f[0] = acc + p[2] * c * c;
}
"""
BOX3_PARAMS = [0.3, 0.0625, 0.5]


def _box3_w(p, T):
    return [p[0] + p[1] * T(di + 3 * dj + 9 * dk) for (di, dj, dk) in BOX]


def _box3_resid(N, _A, p, shape, T):
    acc, m = _wsum(N, BOX, _box3_w(p, T), 0)
    c = N(0, 0, 0)
    e = (p[2] * c) * c
    return [acc + e], [m + np.abs(e)]


def _box3_jvp(N, V, _A, p, shape, T):
    acc, m = _wsum(V, BOX, _box3_w(p, T), 0)
    c, dc = N(0, 0, 0), V(0, 0, 0)
    e1, e2 = (dc * p[2]) * c, (c * p[2]) * dc          # the dual's product rule in the source's order
    return [acc + (e1 + e2)], [m + np.abs(e1) + np.abs(e2)]


def _box3_jac(N, _A, p, shape, T):
    c = N(0, 0, 0)
    one = np.ones_like(c)
    w = _box3_w(p, T)
    J = {}
    for t, o in enumerate(BOX):
        J[(0, *o, 0)] = (w[t] * one, np.abs(w[t]) * one)
    e1, e2 = p[2] * c, c * p[2]
    J[(0, 0, 0, 0, 0)] = (w[13] + (e1 + e2), np.abs(w[13]) + np.abs(e1) + np.abs(e2))
    return J


# ------------------------------------------------------------------------------------------------ four3
# four components, star, Dirichlet. With a, b, d the components c+1, c+2, c+3 (mod 4) at the centre:
#   f_c = (c + 1)·(Σ six weighted neighbours of u_c − p6·u_c) + p7·(a·b) − p8·(u_c·d)
# every component is coupled to every other at the centre; the six directional weights p0..p5 are unequal.
FOUR3_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const T uc = u(0, 0, 0, c), a = u(0, 0, 0, (c + 1) % 4), b = u(0, 0, 0, (c + 2) % 4), d = u(0, 0, 0, (c + 3) % 4);
    const T lap = p[0] * u(-1, 0, 0, c) + p[1] * u(1, 0, 0, c) + p[2] * u(0, -1, 0, c) + p[3] * u(0, 1, 0, c)
                + p[4] * u(0, 0, -1, c) + p[5] * u(0, 0, 1, c) - p[6] * uc;
    f[c] = (nk_real)(c + 1) * lap + p[7] * (a * b) - p[8] * (uc * d);
  }
}
"""
FOUR3_PARAMS = [1.0, 0.75, 1.5, 0.5, 2.0, 1.25, 7.5, 0.625, 0.375]


def _four3_lap(N, p, c):
    s, m = _wsum(N, SIX, p[0:6], c)
    t = p[6] * N(0, 0, 0, c)
    return s - t, m + np.abs(t)


def _four3_resid(N, _A, p, shape, T):
    f, fm = [], []
    for c in range(4):
        uc, a, b, d = (N(0, 0, 0, (c + t) % 4) for t in range(4))
        lap, ml = _four3_lap(N, p, c)
        t1, t2 = p[7] * (a * b), p[8] * (uc * d)
        f.append(T(c + 1) * lap + t1 - t2)
        fm.append(T(c + 1) * ml + np.abs(t1) + np.abs(t2))
    return f, fm


def _four3_jvp(N, V, _A, p, shape, T):
    jv, jm = [], []
    for c in range(4):
        uc, a, b, d = (N(0, 0, 0, (c + t) % 4) for t in range(4))
        duc, da, db, dd = (V(0, 0, 0, (c + t) % 4) for t in range(4))
        lap, ml = _four3_lap(V, p, c)
        ab1, ab2, ud1, ud2 = da * b, a * db, duc * d, uc * dd
        t1, t2 = p[7] * (ab1 + ab2), p[8] * (ud1 + ud2)
        jv.append(T(c + 1) * lap + t1 - t2)
        jm.append(T(c + 1) * ml + np.abs(p[7]) * (np.abs(ab1) + np.abs(ab2)) + np.abs(p[8]) * (np.abs(ud1) + np.abs(ud2)))
    return jv, jm


def _four3_jac(N, _A, p, shape, T):
    J = {}
    one = np.ones_like(N(0, 0, 0, 0))
    for c in range(4):
        uc, a, b, d = (N(0, 0, 0, (c + t) % 4) for t in range(4))
        for t, o in enumerate(SIX):
            w = p[t] * T(c + 1)
            J[(c, *o, c)] = (w * one, np.abs(w) * one)
        t0, t2 = (-p[6]) * T(c + 1), p[8] * d
        J[(c, 0, 0, 0, c)] = (t0 - t2, np.abs(t0) + np.abs(t2))
        J[(c, 0, 0, 0, (c + 1) % 4)] = (p[7] * b, np.abs(p[7] * b))
        J[(c, 0, 0, 0, (c + 2) % 4)] = (p[7] * a, np.abs(p[7] * a))
        J[(c, 0, 0, 0, (c + 3) % 4)] = (-(p[8] * uc), np.abs(p[8] * uc))
    return J


# ------------------------------------------------------------------------------------------------ the cases
PROBLEMS = {
    "bratu3": Problem("bratu3", BRATU3_SRC, 3, 1, "star", "dirichlet", [1.0, 0.04], _bratu3_resid, _bratu3_jvp, _bratu3_jac),
    "brusselator3": Problem("brusselator3", BRUSSELATOR3_SRC, 3, 2, "star", "periodic", BRUSSELATOR3_PARAMS, _brus3_resid,
                            _brus3_jvp, _brus3_jac),
    "box3_dirichlet": Problem("box3_dirichlet", BOX3_SRC, 3, 1, "box", "dirichlet", BOX3_PARAMS, _box3_resid, _box3_jvp, _box3_jac),
    "box3_periodic": Problem("box3_periodic", BOX3_SRC, 3, 1, "box", "periodic", BOX3_PARAMS, _box3_resid, _box3_jvp, _box3_jac),
    "four3": Problem("four3", FOUR3_SRC, 3, 4, "star", "dirichlet", FOUR3_PARAMS, _four3_resid, _four3_jvp, _four3_jac),
}
# 7·6·5: one ragged workgroup; 3·3·3: every node on the boundary; 37·29·3: 13 workgroups, planes of 1073 nodes;
# 5·3·70: planes of 15 nodes, a wavefront spans more than four planes
SIZES = [(7, 6, 5), (3, 3, 3), (37, 29, 3), (5, 3, 70)]
# a star source that reads an edge offset: the residual is NaN at every node
EDGE_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  f[0] = 6.0 * u(0, 0, 0) - u(1, 1, 0) - u(0, 0, -1);
}
"""
SYNTAX_ERROR_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {
  f[0] = u(0, 0, 0) * no_such_symbol;
}
"""
