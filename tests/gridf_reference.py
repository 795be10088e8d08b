"""NumPy restatement of the compiled grid problems WITH FIELDS (csrc/nk_grid.hip, nk_problem_create_grid_fields), in the style
of tests/grid_reference.py: problems that
read read-only data on the grid — a previous time level, a face-averaged coefficient, a source term — each written once as HIP
source (what the library compiles) and once as NumPy formulas with their ANALYTIC derivatives, evaluated in float64 and in long
double. From the formulas: the residual, J·v (the tangent written out by hand, term for term in the source's order), the values
of J on the pattern, Jᵀv, and for every entry the gap |float64 − long double| and the sum of the absolute values of the entry's
terms — the bound the device tests use:

    |device − float64 restatement| <= 16 × gap + 4 eps × Σ|terms|

Fields: field k of node m is element k·nn + m. A field is read through the stencil's offsets; at a periodic boundary the index
wraps, outside a Dirichlet boundary the read returns THE FIELD AT THE NODE ITSELF (u reads 0 there). Fields are constants of the
differentiation: no column, no partial. Seeded fields are 1 + 0.37·sin(0.9·m + k): positive, distinct at every node.
This module is the table: sources, formulas, problems and sizes. The pattern, the access to u, v and the fields, the evaluation in both
arithmetics and the bound are tests/grid_core.py's."""
import numpy as np

import grid3_reference as G3
import grid_r2_reference as G2
import grid_reference as G1
from grid_core import RADIUS, Problem, _sum


# ------------------------------------------------------------------------------------------------ sources
def _head(dim):
    if dim == 2:
        return ("\ntemplate <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, "
                "nk_site s, T *f) {\n")
    return ("\ntemplate <typename T>\n__device__ void nk_point(const nk_nbhd3<T> &u, const nk_flds3 &a, const nk_real *p, "
            "nk_site3 s, T *f) {\n")


def _o(off, *more):
    return ", ".join(str(x) for x in tuple(off) + more)


def _faces_src(offs, g, fk):
    """acc = acc + p[1]·((g·(a(0, fk) + a(off, fk)))·(c − u(off))) for every neighbour, in order"""
    zero = (0,) * len(offs[0])
    return "".join(f"  acc = acc + p[1] * (({gt!r} * (a({_o(zero, fk)}) + a({_o(off, fk)}))) * (c - u({_o(off)})));\n"
                   for off, gt in zip(offs, g))


def _faces(N, A, offs, g, fk, p1, T):
    """the terms p1·(w·(c − u(off))), their Σ|elementary terms|, and the weights w = g·(a(0) + a(off))"""
    zero = (0,) * len(offs[0])
    c = N(*zero)
    w = [T(gt) * (A(*zero, fk) + A(*off, fk)) for off, gt in zip(offs, g)]
    terms = [p1 * (wt * (c - N(*off))) for wt, off in zip(w, offs)]
    mags = [np.abs(p1 * wt) * (np.abs(c) + np.abs(N(*off))) for wt, off in zip(w, offs)]
    return terms, mags, w


FOUR = [(-1, 0), (1, 0), (0, -1), (0, 1)]                  # W E S N, the order the 2-D sources add them
CORNERS = [(-1, -1), (1, -1), (-1, 1), (1, 1)]
HALF4 = [0.5, 0.5, 0.5, 0.5]
G_CORNERS = [1.0, 0.5, 0.25, 2.0]
G_EIGHT = [0.5, 0.5, 0.125, 0.125, 0.5, 0.5, 0.125, 0.125]   # G2.EIGHT: −1 +1 −2 +2 in i, then in j
G_SIX = [0.5, 0.25, 1.0, 0.125, 2.0, 0.75]                   # G3.SIX: a weight per direction AND sign


def _diffusion(spec):
    """(source, resid, jvp, jac) of
        f = [p0·(c − a_prev)  |  p0·c  |  p0·(4c − W − E − S − N)]  +  p1·Σ_offs g·(a(0) + a(off))·(c − u(off))
            [+ p2·c³]  [− a_src]
    spec: dim, offs, g, coef (the coefficient's field), prev / src (field numbers or None), lap (the 2-D 5-point term in place of
    p0·c), cubic"""
    dim, offs, g, fk = spec["dim"], spec["offs"], spec["g"], spec["coef"]
    prev, src, lap, cubic = spec.get("prev"), spec.get("src"), spec.get("lap", False), spec.get("cubic", False)
    zero = (0,) * dim
    text = _head(dim) + f"  const T c = u({_o(zero)});\n"
    if lap:
        text += "  T acc = p[0] * (4.0 * c - u(-1, 0) - u(1, 0) - u(0, -1) - u(0, 1));\n"
    elif prev is not None:
        text += f"  T acc = p[0] * (c - a({_o(zero, prev)}));\n"
    else:
        text += "  T acc = p[0] * c;\n"
    text += _faces_src(offs, g, fk)
    if cubic:
        text += "  acc = acc + p[2] * ((c * c) * c);\n"
    text += (f"  f[0] = acc - a({_o(zero, src)});\n" if src is not None else "  f[0] = acc;\n") + "}\n"

    def first(N, A, p, T, tangent=None):
        """the first term at (u) or its tangent at (u; v), with Σ|elementary terms|"""
        X = N if tangent is None else tangent
        if lap:
            s, m = G1._box_lap(X, 0, T)
            return p[0] * s, np.abs(p[0]) * m
        if prev is not None and tangent is None:
            return p[0] * (X(*zero) - A(*zero, prev)), np.abs(p[0]) * (np.abs(X(*zero)) + np.abs(A(*zero, prev)))
        return p[0] * X(*zero), np.abs(p[0] * X(*zero))

    def resid(N, A, p, shape, T):
        c = N(*zero)
        t0, m0 = first(N, A, p, T)
        terms, mags, _w = _faces(N, A, offs, g, fk, p[1], T)
        if cubic:
            terms.append(p[2] * ((c * c) * c))
            mags.append(np.abs(terms[-1]))
        if src is not None:
            terms.append(-A(*zero, src))
            mags.append(np.abs(terms[-1]))
        return [_sum([t0] + terms)[0]], [_sum([m0] + mags)[0]]

    def jvp(N, V, A, p, shape, T):
        c, dc = N(*zero), V(*zero)
        t0, m0 = first(N, A, p, T, tangent=V)
        terms, mags, _w = _faces(V, A, offs, g, fk, p[1], T)
        if cubic:   # the dual's product rule in the source's order: d(c·c) = dc·c + c·dc ; d((c·c)·c) = d(c·c)·c + (c·c)·dc
            d2 = dc * c + c * dc
            terms.append(p[2] * (d2 * c + (c * c) * dc))
            mags.append(np.abs(p[2]) * (2 * np.abs(dc * c * c) + np.abs(c * c * dc)))
        return [_sum([t0] + terms)[0]], [_sum([m0] + mags)[0]]

    def jac(N, A, p, shape, T):
        c = N(*zero)
        one = np.ones_like(c)
        _t, _m, w = _faces(N, A, offs, g, fk, p[1], T)
        diag = [(p[0] * T(4) if lap else p[0]) * one] + [p[1] * wt for wt in w]
        if cubic:
            diag.append(p[2] * ((c + c) * c + c * c))
        J = {(0,) + zero + (0,): (_sum(diag)[0], _sum([np.abs(x) for x in diag])[0])}
        for off, wt in zip(offs, w):
            J[(0,) + tuple(off) + (0,)] = (-(p[1] * wt), np.abs(p[1] * wt))
        if lap:
            for off in FOUR:
                J[(0,) + off + (0,)] = (-p[0] * one, np.abs(p[0]) * one)
        return J

    return text, resid, jvp, jac


# ------------------------------------------------------------------------------------------------ react2
# a Brusselator whose cross term u0²·u1 carries a coefficient put together from the field at all five points, a weight per
# direction and sign: κ = a + ¼a_W + ½a_E + ⅛a_S + 2a_N.  p = {A, B, α}
REACT2_SRC = _head(2) + r"""  const nk_real A = p[0], B = p[1], alpha = p[2];
  const nk_real kap = a(0, 0) + 0.25 * a(-1, 0) + 0.5 * a(1, 0) + 0.125 * a(0, -1) + 2.0 * a(0, 1);
  const T uu = u(0, 0, 0), vv = u(0, 0, 1);
  const T lu = u(-1, 0, 0) + u(1, 0, 0) - 4.0 * uu + u(0, 1, 0) + u(0, -1, 0);
  const T lv = u(-1, 0, 1) + u(1, 0, 1) - 4.0 * vv + u(0, 1, 1) + u(0, -1, 1);
  const T r = kap * (uu * uu * vv);
  f[0] = alpha * lu + B + r - (A + 1.0) * uu;
  f[1] = alpha * lv + A * uu - r;
}
"""


def _kappa(A, T):
    return _sum([A(0, 0), T(0.25) * A(-1, 0), T(0.5) * A(1, 0), T(0.125) * A(0, -1), T(2) * A(0, 1)])[0]


def _react2_resid(N, A, p, shape, T):
    Ap, B, al = p
    k, uu, vv = _kappa(A, T), N(0, 0, 0), N(0, 0, 1)
    lu, mu = G1._brus_lap(N, 0, T)
    lv, mv = G1._brus_lap(N, 1, T)
    r = k * (uu * uu * vv)
    f0, m0 = _sum([al * lu, B * np.ones_like(uu), r, -((Ap + T(1)) * uu)])
    f1, m1 = _sum([al * lv, Ap * uu, -r])
    return [f0, f1], [m0 - np.abs(al * lu) + np.abs(al) * mu, m1 - np.abs(al * lv) + np.abs(al) * mv]


def _react2_jvp(N, V, A, p, shape, T):
    Ap, B, al = p
    k, uu, vv, a, b = _kappa(A, T), N(0, 0, 0), N(0, 0, 1), V(0, 0, 0), V(0, 0, 1)
    la, ma = G1._brus_lap(V, 0, T)
    lb, mb = G1._brus_lap(V, 1, T)
    duu = a * uu + uu * a                      # the dual's product rule, in the source's order
    dr = k * (duu * vv + (uu * uu) * b)
    mr = np.abs(k) * (np.abs(a * uu) * 2 * np.abs(vv) + np.abs((uu * uu) * b))
    t4 = (Ap + T(1)) * a
    return [al * la + dr - t4, al * lb + Ap * a - dr], [np.abs(al) * ma + mr + np.abs(t4), np.abs(al) * mb + np.abs(Ap * a) + mr]


def _react2_jac(N, A, p, shape, T):
    Ap, B, al = p
    k, uu, vv = _kappa(A, T), N(0, 0, 0), N(0, 0, 1)
    one = np.ones_like(uu)
    k2uv, kuu = k * ((uu + uu) * vv), k * (uu * uu)
    J = {
        (0, 0, 0, 0): (al * T(-4) + k2uv - (Ap + T(1)), np.abs(al * T(4)) + np.abs(k2uv) + np.abs(Ap + T(1))),
        (0, 0, 0, 1): (kuu, np.abs(kuu)),
        (1, 0, 0, 1): (al * T(-4) - kuu, np.abs(al * T(4)) + np.abs(kuu)),
        (1, 0, 0, 0): (Ap - k2uv, np.abs(Ap) + np.abs(k2uv)),
    }
    for off in FOUR:
        for c in (0, 1):
            J[(c,) + off + (c,)] = (al * one, np.abs(al) * one)
    return J


# ------------------------------------------------------------------------------------------------ bratu_f
# Bratu with the source strength taken from a field: F = p0·(4u − W − E − S − N) − (p1·a)·eᵘ — the one elementary function
BRATU_F_SRC = _head(2) + r"""  const T c = u(0, 0);
  f[0] = p[0] * (4.0 * c - u(-1, 0) - u(1, 0) - u(0, -1) - u(0, 1)) - (p[1] * a(0, 0)) * exp(c);
}
"""


def _bratu_f_resid(N, A, p, shape, T):
    lap, ml = G1._box_lap(N, 0, T)
    e = (p[1] * A(0, 0)) * np.exp(N(0, 0))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu_f_jvp(N, V, A, p, shape, T):
    lap, ml = G1._box_lap(V, 0, T)
    e = (p[1] * A(0, 0)) * (np.exp(N(0, 0)) * V(0, 0))
    return [p[0] * lap - e], [np.abs(p[0]) * ml + np.abs(e)]


def _bratu_f_jac(N, A, p, shape, T):
    one = np.ones_like(N(0, 0))
    e = (p[1] * A(0, 0)) * np.exp(N(0, 0))
    J = {(0, 0, 0, 0): (p[0] * T(4) - e, np.abs(p[0] * T(4)) + np.abs(e))}
    for off in FOUR:
        J[(0,) + off + (0,)] = (-p[0] * one, np.abs(p[0]) * one)
    return J


# ------------------------------------------------------------------------------------------------ the cases
def _diffusion_problem(name, stencil, boundary, params, nfields, **spec):
    source, resid, jvp, jac = _diffusion(spec)
    return Problem(name, source, spec["dim"], 1, stencil, boundary, params, resid, jvp, jac, nfields)


_BF = (_bratu_f_resid, _bratu_f_jvp, _bratu_f_jac)
_BOXSPEC = dict(dim=2, offs=CORNERS, g=G_CORNERS, coef=0, lap=True)
PROBLEMS = {
    # p0·(u − a0) + p1·Σ_faces ½(a1 + a1(face))·(u − u_face) − a2: a previous level, a face-averaged coefficient, a source
    "vardiff": _diffusion_problem("vardiff", "star", "dirichlet", [4.0, 1.5], 3, dim=2, offs=FOUR, g=HALF4, coef=1, prev=0, src=2),
    # … + p2·u³: the nonlinear problem of the time-stepping test
    "vardiff_r": _diffusion_problem("vardiff_r", "star", "dirichlet", [4.0, 1.5, 0.75], 3, dim=2, offs=FOUR, g=HALF4, coef=1,
                                    prev=0, src=2, cubic=True),
    "react2": Problem("react2", REACT2_SRC, 2, 2, "star", "periodic", [3.4, 1.0, 40.0], _react2_resid, _react2_jvp, _react2_jac, 1),
    "vardiff_box_dirichlet": _diffusion_problem("vardiff_box_dirichlet", "box", "dirichlet", [1.25, 0.75], 1, **_BOXSPEC),
    "vardiff_box_periodic": _diffusion_problem("vardiff_box_periodic", "box", "periodic", [1.25, 0.75], 1, **_BOXSPEC),
    "vardiff_s2": _diffusion_problem("vardiff_s2", "star2", "dirichlet", [0.5, 1.5], 1, dim=2, offs=G2.EIGHT, g=G_EIGHT, coef=0),
    "vardiff3": _diffusion_problem("vardiff3", "star", "dirichlet", [4.0, 1.5], 2, dim=3, offs=G3.SIX, g=G_SIX, coef=1, prev=0),
    "bratu_f": Problem("bratu_f", BRATU_F_SRC, 2, 1, "star", "dirichlet", [1.0, 0.04], *_BF, 1),
    # the same source with four fields declared: three of them are never read
    "bratu_f4": Problem("bratu_f4", BRATU_F_SRC, 2, 1, "star", "dirichlet", [1.0, 0.04], *_BF, 4),
}
SIZES_R1 = [(37, 29), (3, 3), (300, 5)]   # 37 × 29 = 1073 nodes: five workgroups of 256, the last one ragged
SIZES_R2 = [(5, 5), (37, 29)]
SIZES_3 = [(7, 6, 5), (3, 3, 3), (37, 29, 3)]


def sizes(prob):
    return SIZES_3 if prob.dim == 3 else (SIZES_R2 if RADIUS[prob.stencil] == 2 else SIZES_R1)


# the pre-field contract, for the error message test
OLD_SIGNATURE_SRC = G1.BRATU_SRC
