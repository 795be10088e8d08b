"""NumPy restatement of the compiled grid problems (csrc/nk_grid.hip): three pointwise problems —
Bratu, the Brusselator with its disc forcing, a two-component 9-point box problem with a cross term — each written once as HIP
source (what the library compiles) and once as NumPy formulas with their ANALYTIC derivatives, evaluated in float64 and in long
double. From the formulas: the residual, J·v (the tangent of the residual written out by hand, term for term in the source's
order), the values of J on the pattern, Jᵀv, and for every entry the gap |float64 − long double| and the sum of the absolute
values of the entry's terms, which together make the bound the device tests use (the rule of tests/test_gpu_broyden.py):

    |device − float64 restatement| <= 16 × gap + 4 eps × Σ|terms|

Layout: unknown c of node (i, j) is element c·nx·ny + j·nx + i. Seeded inputs have |u| <= 1.
Stencil points in pattern order (ascending node index inside the grid): star S W C E N, box row by row.
This module is the table: sources, formulas, problems and sizes. The pattern, the access to u and v, the evaluation in both
arithmetics and the bound are tests/grid_core.py's."""
import numpy as np

from grid_core import Problem, _site, _sum


# ------------------------------------------------------------------------------------------------ Bratu
# F = c_lap·(4u − W − E − S − N) − c_exp·eᵘ ;  p = {c_lap, c_exp}. Bratu2D(n, λ) is c_lap = 1, c_exp = λ/(n + 1)², Dirichlet.
BRATU_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  const T c = u(0, 0);
  f[0] = p[0] * (4.0 * c - u(-1, 0) - u(1, 0) - u(0, -1) - u(0, 1)) - p[1] * exp(c);
}
"""


def bratu_params(n, lam=6.0):
    h = 1.0 / (n + 1)
    return [(h * h) / (h * h), (h * h) * lam]


def _bratu_resid(N, _A, p, shape, T):
    c = N(0, 0)
    lap, ml = _sum([T(4) * c, -N(-1, 0), -N(1, 0), -N(0, -1), -N(0, 1)])
    e = p[1] * np.exp(c)
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu_jvp(N, V, _A, p, shape, T):
    c = N(0, 0)
    lap, ml = _sum([T(4) * V(0, 0), -V(-1, 0), -V(1, 0), -V(0, -1), -V(0, 1)])
    e = p[1] * (np.exp(c) * V(0, 0))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu_jac(N, _A, p, shape, T):
    c = N(0, 0)
    one = np.ones_like(c)
    e = p[1] * np.exp(c)
    J = {(0, 0, 0, 0): (p[0] * T(4) - e, np.abs(p[0] * T(4)) + np.abs(e))}
    for di, dj in [(-1, 0), (1, 0), (0, -1), (0, 1)]:
        J[(0, di, dj, 0)] = (-p[0] * one, np.abs(p[0]) * one)
    return J


# ------------------------------------------------------------------------------------------------ Brusselator
# brusselator_2d_loop with α/dx² folded into p[2]; p = {A, B, α/dx²}; the disc forcing 5 on (x − 0.3)² + (y − 0.6)² <= 0.1².
# Brusselator2D(N, A, B, α, dx) is periodic, p = {A, B, α/dx²}.
BRUSSELATOR_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  const nk_real A = p[0], B = p[1], alpha = p[2];
  const nk_real x = (nk_real)s.i / (nk_real)(s.nx - 1), y = (nk_real)s.j / (nk_real)(s.ny - 1);
  const nk_real bf = (((x - 0.3) * (x - 0.3) + (y - 0.6) * (y - 0.6)) <= 0.1 * 0.1) ? 5.0 : 0.0;
  const T uu = u(0, 0, 0), vv = u(0, 0, 1);
  const T lu = u(-1, 0, 0) + u(1, 0, 0) - 4.0 * uu + u(0, 1, 0) + u(0, -1, 0);
  const T lv = u(-1, 0, 1) + u(1, 0, 1) - 4.0 * vv + u(0, 1, 1) + u(0, -1, 1);
  f[0] = alpha * lu + B + uu * uu * vv - (A + 1.0) * uu + bf;
  f[1] = alpha * lv + A * uu - uu * uu * vv;
}
"""


def brusselator_params(N, A=3.4, B=1.0, alpha=10.0, dx=None):
    dx = 1.0 / (N - 1) if dx is None else dx
    return [A, B, alpha / (dx * dx)]


def _brus_forcing(shape, T):
    nx, ny = shape
    # the disc is decided in float64 in both arithmetics (the source decides it in double): the two restatements then differ by
    # rounding only
    i, j = _site(shape)
    x, y = i / np.float64(nx - 1), j / np.float64(ny - 1)
    return np.where(((x - 0.3) * (x - 0.3) + (y - 0.6) * (y - 0.6)) <= 0.1 * 0.1, 5.0, 0.0).astype(T)


def _brus_lap(N, c, T):
    return _sum([N(-1, 0, c), N(1, 0, c), -(T(4) * N(0, 0, c)), N(0, 1, c), N(0, -1, c)])


def _brus_resid(N, _A, p, shape, T):
    A, B, al = p
    uu, vv = N(0, 0, 0), N(0, 0, 1)
    lu, mu = _brus_lap(N, 0, T)
    lv, mv = _brus_lap(N, 1, T)
    bf = _brus_forcing(shape, T)
    f0, m0 = _sum([al * lu, B * np.ones_like(uu), uu * uu * vv, -((A + T(1)) * uu), bf])
    f1, m1 = _sum([al * lv, A * uu, -(uu * uu * vv)])
    return [f0, f1], [m0 - np.abs(al * lu) + np.abs(al) * mu, m1 - np.abs(al * lv) + np.abs(al) * mv]


def _brus_jvp(N, V, _A, p, shape, T):
    A, B, al = p
    uu, vv, a, b = N(0, 0, 0), N(0, 0, 1), V(0, 0, 0), V(0, 0, 1)
    la, ma = _brus_lap(V, 0, T)
    lb, mb = _brus_lap(V, 1, T)
    # the dual's product rule, in the source's order: d(uu·uu) = a·uu + uu·a ; d((uu·uu)·vv) = d(uu·uu)·vv + (uu·uu)·b
    duu = a * uu + uu * a
    d3, m3 = _sum([duu * vv, (uu * uu) * b])
    m3 = np.abs(a * uu) * 2 * np.abs(vv) + np.abs((uu * uu) * b)
    t4 = (A + T(1)) * a
    jv0 = al * la + d3 - t4
    jv1 = al * lb + A * a - d3
    return [jv0, jv1], [np.abs(al) * ma + m3 + np.abs(t4), np.abs(al) * mb + np.abs(A * a) + m3]


def _brus_jac(N, _A, p, shape, T):
    A, B, al = p
    uu, vv = N(0, 0, 0), N(0, 0, 1)
    one = np.ones_like(uu)
    two_uv = (uu + uu) * vv
    J = {
        (0, 0, 0, 0): (al * T(-4) + two_uv - (A + T(1)), np.abs(al * T(4)) + np.abs(two_uv) + np.abs(A + T(1))),
        (0, 0, 0, 1): (uu * uu, uu * uu),
        (1, 0, 0, 1): (al * T(-4) - uu * uu, np.abs(al * T(4)) + uu * uu),
        (1, 0, 0, 0): (A - two_uv, np.abs(A) + np.abs(two_uv)),
    }
    for di, dj in [(-1, 0), (1, 0), (0, -1), (0, 1)]:
        for c in (0, 1):
            J[(c, di, dj, c)] = (al * one, np.abs(al) * one)
    return J


# ------------------------------------------------------------------------------------------------ 9-point box, two components
# a = component 0, b = component 1, X(w) = w(1,1) − w(1,−1) − w(−1,1) + w(−1,−1) (the mixed second difference):
#   f0 = p0·(4a − a_W − a_E − a_S − a_N) + p1·X(a)·b + p2·eᵃ
#   f1 = p0·(4b − b_W − b_E − b_S − b_N) + p1·X(b)·a − a·b
BOX_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  const T a = u(0, 0, 0), b = u(0, 0, 1);
  const T xa = u(1, 1, 0) - u(1, -1, 0) - u(-1, 1, 0) + u(-1, -1, 0);
  const T xb = u(1, 1, 1) - u(1, -1, 1) - u(-1, 1, 1) + u(-1, -1, 1);
  f[0] = p[0] * (4.0 * a - u(-1, 0, 0) - u(1, 0, 0) - u(0, -1, 0) - u(0, 1, 0)) + p[1] * (xa * b) + p[2] * exp(a);
  f[1] = p[0] * (4.0 * b - u(-1, 0, 1) - u(1, 0, 1) - u(0, -1, 1) - u(0, 1, 1)) + p[1] * (xb * a) - a * b;
}
"""
BOX_PARAMS = [1.25, 0.75, 0.5]
_CROSS = [((1, 1), 1.0), ((1, -1), -1.0), ((-1, 1), -1.0), ((-1, -1), 1.0)]


def _box_lap(N, c, T):
    return _sum([T(4) * N(0, 0, c), -N(-1, 0, c), -N(1, 0, c), -N(0, -1, c), -N(0, 1, c)])


def _box_cross(N, c):
    return _sum([N(1, 1, c), -N(1, -1, c), -N(-1, 1, c), N(-1, -1, c)])


def _box_resid(N, _A, p, shape, T):
    a, b = N(0, 0, 0), N(0, 0, 1)
    la, mla = _box_lap(N, 0, T)
    lb, mlb = _box_lap(N, 1, T)
    xa, mxa = _box_cross(N, 0)
    xb, mxb = _box_cross(N, 1)
    e = p[2] * np.exp(a)
    f0 = p[0] * la + p[1] * (xa * b) + e
    f1 = p[0] * lb + p[1] * (xb * a) - a * b
    return [f0, f1], [np.abs(p[0]) * mla + np.abs(p[1]) * mxa * np.abs(b) + np.abs(e),
                      np.abs(p[0]) * mlb + np.abs(p[1]) * mxb * np.abs(a) + np.abs(a * b)]


def _box_jvp(N, V, _A, p, shape, T):
    a, b, da, db = N(0, 0, 0), N(0, 0, 1), V(0, 0, 0), V(0, 0, 1)
    la, mla = _box_lap(V, 0, T)
    lb, mlb = _box_lap(V, 1, T)
    xa, _ = _box_cross(N, 0)
    xb, _ = _box_cross(N, 1)
    dxa, mdxa = _box_cross(V, 0)
    dxb, mdxb = _box_cross(V, 1)
    t0 = p[1] * (dxa * b + xa * db)          # the dual's product rule in the source's order
    e = p[2] * (np.exp(a) * da)
    t1 = p[1] * (dxb * a + xb * da)
    ab = da * b + a * db
    m0 = np.abs(p[0]) * mla + np.abs(p[1]) * (mdxa * np.abs(b) + np.abs(xa * db)) + np.abs(e)
    m1 = np.abs(p[0]) * mlb + np.abs(p[1]) * (mdxb * np.abs(a) + np.abs(xb * da)) + np.abs(da * b) + np.abs(a * db)
    return [p[0] * la + t0 + e, p[0] * lb + t1 - ab], [m0, m1]


def _box_jac(N, _A, p, shape, T):
    a, b = N(0, 0, 0), N(0, 0, 1)
    one = np.ones_like(a)
    xa, mxa = _box_cross(N, 0)
    xb, mxb = _box_cross(N, 1)
    e = p[2] * np.exp(a)
    J = {
        (0, 0, 0, 0): (p[0] * T(4) + e, np.abs(p[0] * T(4)) + np.abs(e)),
        (0, 0, 0, 1): (p[1] * xa, np.abs(p[1]) * mxa),
        (1, 0, 0, 1): (p[0] * T(4) - a, np.abs(p[0] * T(4)) + np.abs(a)),
        (1, 0, 0, 0): (p[1] * xb - b, np.abs(p[1]) * mxb + np.abs(b)),
    }
    for di, dj in [(-1, 0), (1, 0), (0, -1), (0, 1)]:
        for c in (0, 1):
            J[(c, di, dj, c)] = (-p[0] * one, np.abs(p[0]) * one)
    for (di, dj), sg in _CROSS:
        J[(0, di, dj, 0)] = (p[1] * (T(sg) * b), np.abs(p[1] * b))
        J[(1, di, dj, 1)] = (p[1] * (T(sg) * a), np.abs(p[1] * a))
    return J


# ------------------------------------------------------------------------------------------------ the cases
def _problem(name, source, dof, stencil, boundary, params, *formulas):
    """(this table's inputs are seeded with 7·nx + ny)"""
    return Problem(name, source, 2, dof, stencil, boundary, params, *formulas, seed_weights=(7, 1))


PROBLEMS = {
    "bratu": _problem("bratu", BRATU_SRC, 1, "star", "dirichlet", [1.0, 0.04], _bratu_resid, _bratu_jvp, _bratu_jac),
    "brusselator": _problem("brusselator", BRUSSELATOR_SRC, 2, "star", "periodic", [3.4, 1.0, 40.0], _brus_resid, _brus_jvp,
                            _brus_jac),
    "box_dirichlet": _problem("box_dirichlet", BOX_SRC, 2, "box", "dirichlet", BOX_PARAMS, _box_resid, _box_jvp, _box_jac),
    "box_periodic": _problem("box_periodic", BOX_SRC, 2, "box", "periodic", BOX_PARAMS, _box_resid, _box_jvp, _box_jac),
}
SIZES = [(37, 29), (3, 3), (300, 5)]   # 37 × 29 = 1073 nodes: five workgroups of 256, the last one ragged
# a star source that reads a corner: the residual is NaN at every node
CORNER_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  f[0] = 4.0 * u(0, 0) - u(1, 1) - u(-1, -1);
}
"""
SYNTAX_ERROR_SRC = r"""
template <typename T>
__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {
  f[0] = u(0, 0) * no_such_symbol;
}
"""


def bratu_builtin_pattern(ns):
    """the five-branch order written out in nk_problem_jac_csr for BRATU2D"""
    rp, ci = [], []
    for j in range(ns):
        for i in range(ns):
            k = j * ns + i
            rp.append(len(ci))
            if j > 0:
                ci.append(k - ns)
            if i > 0:
                ci.append(k - 1)
            ci.append(k)
            if i < ns - 1:
                ci.append(k + 1)
            if j < ns - 1:
                ci.append(k + ns)
    rp.append(len(ci))
    return np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32)
