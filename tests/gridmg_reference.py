"""NumPy/SciPy float64 restatement of the geometric multigrid `precs` of compiled grid problems (csrc/nk_gridmg.hip) and the
problems its tests run on.

Geometry of one axis of n nodes, lengths in units of the fine spacing. A side has the offset a = 1 ("dirichlet": the wall is one
spacing outside the outermost node and the ghost reads 0), 0 ("mirror_node") or 1/2 ("mirror_face"):

    L = n − 1 + a_lo + a_hi, node i sits at a_lo + i, nc = ⌊L/2 + 1.5 − a_lo − a_hi⌋, H = L/(nc − 1 + a_lo + a_hi)
    periodic: L = n, nc = ⌊n/2 + 0.5⌋, H = n/nc

An axis is coarsened only while n > coarse_max and nc >= the stencil's smallest side (3; radius 2: 5); otherwise it keeps its
side, and the hierarchy ends when no axis is coarsened.

Prolongation on one axis: t = (a_lo + i)·(nc − 1 + a_lo + a_hi)/L − a_lo (periodic: i·nc/n), J0 = ⌊t⌋, weights 1 − w1 on J0 and
w1 = t − J0 on J0 + 1, a weight within 1e-12 of 0 or 1 snapped to the node; a coarse index outside 0 … nc−1 goes through the
grid's own side map (grid_core.axis_map: Dirichlet drops, periodic wraps, the mirrors reflect); weights landing on one
coarse node are added. Restriction = the row-normalised transpose, on every axis, for residuals, u and fields alike. Transfers
of a grid are tensor products (node = (k·ny + j)·nx + i: the outermost axis is the first Kronecker factor), components one by
one (vectors are component-major).

Level l is the same problem on the level's sides: A_l = its Jacobian at u_l = R u_{l−1} with fields R a_{l−1} and the same p.
Smoother: ν Chebyshev steps on D⁻¹A_l over [ρ/4, ρ], ρ = max_i Σ_j |a_ij| / |a_ii| — the recurrence of
oracle/reference_restatement.py::BratuMultigrid._smooth with r replaced by D⁻¹r, the residual recomputed as b − A x every step.
Cycle: ν pre-smoothing steps from a zero guess, residual, restrict, recurse, prolong and add, ν post-smoothing steps; sparse LU
on the coarsest level; a single level is smoothed only.

The problems take their spacing from the level they run on (s.nx, s.ny, s.nz), as the multigrid's contract asks: the unit
interval per axis, h = 1/(n − 1 + a_lo + a_hi) (periodic: 1/n). Every one is  F_c(u) = Σ_points coef·u(point) + g_c(u at the node),
so its Jacobian is the stencil matrix plus a pointwise block."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import grid_core as GC

OFFSET = {"dirichlet": 1.0, "periodic": 0.0, "mirror_node": 0.0, "mirror_face": 0.5}
ALL_KINDS = ("dirichlet", "mirror_node", "mirror_face")
# the 10 side pairs of an axis: 3 × 3 non-periodic ones and the periodic axis
SIDE_PAIRS = [(lo, hi) for lo in ALL_KINDS for hi in ALL_KINDS] + [("periodic", "periodic")]


# ------------------------------------------------------------------------------------------------ one axis
def coarse_side(n, lo, hi):
    if lo == "periodic":
        return int(np.floor(n / 2 + 0.5))
    a = OFFSET[lo] + OFFSET[hi]
    return int(np.floor((n - 1 + a) / 2 + 1.5 - a))


def axis_table(n, lo, hi):
    """(nc, idx[n, 2], w[n, 2]): the folded prolongation table; a dropped, merged or zero-weight entry is (−1, 0)"""
    nc = coarse_side(n, lo, hi)
    per = lo == "periodic"
    alo, ahi = OFFSET[lo], OFFSET[hi]
    L = float(n) if per else n - 1 + alo + ahi
    Lc = float(nc) if per else nc - 1 + alo + ahi
    land = GC.axis_map(nc, lo, hi)                 # positions −PAD … nc−1+PAD
    idx, w = -np.ones((n, 2), dtype=np.int64), np.zeros((n, 2))
    for i in range(n):
        t = i * Lc / L if per else (alo + i) * Lc / L - alo
        J0 = int(np.floor(t))
        w1 = t - J0
        if w1 < 1e-12:
            w1 = 0.0
        elif w1 > 1.0 - 1e-12:
            J0, w1 = J0 + 1, 0.0
        for s, wt in enumerate((1.0 - w1, w1)):
            if wt == 0.0:
                continue
            J = int(land[J0 + s + GC.PAD])
            if J < 0:
                continue
            if s == 1 and idx[i, 0] == J:
                w[i, 0] += wt
            else:
                idx[i, s], w[i, s] = J, wt
    return nc, idx, w


def axis_prolongation(n, lo, hi):
    """the n × nc matrix of the table"""
    nc, idx, w = axis_table(n, lo, hi)
    rows, cols = np.nonzero(idx >= 0)
    return sp.csr_matrix((w[rows, cols], (rows, idx[rows, cols])), shape=(n, nc))


def row_normalised_transpose(P):
    Rm = sp.csr_matrix(P.T)
    return sp.csr_matrix(sp.diags(1.0 / np.asarray(Rm.sum(axis=1)).ravel()) @ Rm)


def level_shapes(shape, sides, radius, coarse_max):
    """the sides of every level, finest first"""
    shape, out = tuple(int(x) for x in shape), []
    min_side = 2 * radius + 1
    while True:
        out.append(shape)
        nxt = list(shape)
        for a, n in enumerate(shape):
            if n <= coarse_max:
                continue
            nc = coarse_side(n, sides[2 * a], sides[2 * a + 1])
            if nc >= min_side and nc < n:
                nxt[a] = nc
        if tuple(nxt) == shape:
            return out
        shape = tuple(nxt)


def transfers(fine, coarse, sides):
    """(P, R) between two levels of one component: Kronecker products, outermost axis first"""
    P = R = None
    for a in range(len(fine)):
        if coarse[a] == fine[a]:
            P1 = R1 = sp.identity(fine[a], format="csr")
        else:
            P1 = axis_prolongation(fine[a], sides[2 * a], sides[2 * a + 1])
            assert P1.shape[1] == coarse[a]
            R1 = row_normalised_transpose(P1)
        P = P1 if P is None else sp.kron(P1, P, format="csr")
        R = R1 if R is None else sp.kron(R1, R, format="csr")
    return P, R


# ------------------------------------------------------------------------------------------------ the problems
STAR2, STAR3, STAR2_R2 = GC.STENCILS[(2, "star")], GC.STENCILS[(3, "star")], GC.STENCILS[(2, "star2")]


def spacing(shape, sides):
    return [1.0 / n if sides[2 * a] == "periodic" else 1.0 / (n - 1 + OFFSET[sides[2 * a]] + OFFSET[sides[2 * a + 1]])
            for a, n in enumerate(shape)]


class Problem:
    """F_c(u) = Σ_q Σ_c2 coef[c][c2][q]·u_c2(point q) + g_c(u at the node): `stencil_coef(shape, fields, p)` gives the
    coefficients (a number or an array per node; missing = 0), `react(u, fields, p)` the list of g_c and `dreact` the dof × dof
    list of ∂g_c/∂u_c2 (arrays per node or numbers)"""
    dof, nfields, stencil, radius = 1, 0, "star", 1

    def __init__(self, name, source, sides, offs, params):
        self.name, self.source, self.boundary, self.offs, self.params = name, source, tuple(sides), offs, list(params)
        self.dim = len(offs[0])

    def linear(self, shape, fields, p):
        """the stencil part as a sparse matrix (a point that left through a Dirichlet side has no column, points on one node add)"""
        nn = int(np.prod(shape))
        idx, inside = GC.neighbours(shape, self.offs, self.boundary)
        coef = self.stencil_coef(shape, fields, p, idx)
        rows, cols, vals = [], [], []
        nodes = np.arange(nn)
        for (c, c2, q), v in coef.items():
            ok = inside[:, q]
            rows.append(c * nn + nodes[ok])
            cols.append(c2 * nn + idx[ok, q])
            vals.append(np.broadcast_to(v, nn)[ok])
        return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                             shape=(self.dof * nn, self.dof * nn))

    def residual(self, shape, u, fields=None, p=None):
        p = self.params if p is None else p
        nn = int(np.prod(shape))
        g = self.react(np.asarray(u).reshape(self.dof, nn), fields, p)
        return self.linear(shape, fields, p) @ u + np.concatenate([np.broadcast_to(x, nn) for x in g])

    def jac(self, shape, u, fields=None, p=None):
        p = self.params if p is None else p
        nn = int(np.prod(shape))
        dg = self.dreact(np.asarray(u).reshape(self.dof, nn), fields, p)
        blocks = [[sp.diags(np.broadcast_to(dg[c][c2], nn).astype(float)) for c2 in range(self.dof)] for c in range(self.dof)]
        J = sp.csr_matrix(self.linear(shape, fields, p) + sp.bmat(blocks))
        J.sort_indices()
        return J

    def fields(self, shape):
        return None

    def coords(self, shape):
        """the positions of the nodes on the unit interval per axis, raveled in node order: [x, y[, z]]"""
        h = spacing(shape, self.boundary)
        ax = [(OFFSET[self.boundary[2 * a]] + np.arange(n)) * h[a] for a, n in enumerate(shape)]
        mesh = np.meshgrid(*ax[::-1], indexing="ij")[::-1]
        return [m.ravel() for m in mesh]


def _laplace_coef(offs, h, scale=1.0, c=0, out=None):
    """−scale·Δ_h on a star: the centre gets Σ 2/h_a², a neighbour along axis a −1/h_a²"""
    out = {} if out is None else out
    for q, off in enumerate(offs):
        nz = [a for a, d in enumerate(off) if d != 0]
        if not nz:
            out[(c, c, q)] = scale * sum(2.0 / (x * x) for x in h)
        elif len(nz) == 1 and abs(off[nz[0]]) == 1:
            out[(c, c, q)] = -scale / (h[nz[0]] * h[nz[0]])
    return out


_H2 = """  const nk_real hx = 1.0 / (s.nx + %s), hy = 1.0 / (s.ny + %s);
  const nk_real cx = 1.0 / (hx * hx), cy = 1.0 / (hy * hy);
"""


def _extra(sides, a):
    """n + this = 1/h of axis a"""
    return "0.0" if sides[2 * a] == "periodic" else repr(OFFSET[sides[2 * a]] + OFFSET[sides[2 * a + 1]] - 1.0)


class Bratu(Problem):
    """(a) −Δu − λ e^u, Dirichlet, star"""

    def __init__(self):
        sides = ("dirichlet",) * 4
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {\n"
               + _H2 % (_extra(sides, 0), _extra(sides, 1)) +
               "  const T c = u(0, 0);\n"
               "  f[0] = cx * (2.0 * c - u(-1, 0) - u(1, 0)) + cy * (2.0 * c - u(0, -1) - u(0, 1)) - p[0] * exp(c);\n}\n")
        super().__init__("bratu", src, sides, STAR2, [1.0])

    def stencil_coef(self, shape, fields, p, idx):
        return _laplace_coef(self.offs, spacing(shape, self.boundary))

    def react(self, u, fields, p):
        return [-p[0] * np.exp(u[0])]

    def dreact(self, u, fields, p):
        return [[-p[0] * np.exp(u[0])]]


class Channel(Problem):
    """(b) σ(u − u_old) − div(a ∇u) + u³ on the channel {"x": "periodic", "y": "mirror_face"}: a is field 0 (face values are
    the mean of the two nodes), u_old field 1"""
    nfields = 2

    def __init__(self):
        sides = ("periodic", "periodic", "mirror_face", "mirror_face")
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, "
               "nk_site s, T *f) {\n" + _H2 % (_extra(sides, 0), _extra(sides, 1)) +
               "  const T c = u(0, 0);\n"
               "  const nk_real a0 = a(0, 0, 0);\n"
               "  const nk_real aw = 0.5 * (a0 + a(-1, 0, 0)), ae = 0.5 * (a0 + a(1, 0, 0));\n"
               "  const nk_real as = 0.5 * (a0 + a(0, -1, 0)), an = 0.5 * (a0 + a(0, 1, 0));\n"
               "  f[0] = (cx * aw) * (c - u(-1, 0)) + (cx * ae) * (c - u(1, 0)) + (cy * as) * (c - u(0, -1)) + (cy * an) * (c - u(0, 1))\n"
               "         + p[0] * (c - a(0, 0, 1)) + c * c * c;\n}\n")
        super().__init__("channel", src, sides, STAR2, [50.0])

    def stencil_coef(self, shape, fields, p, idx):
        h = spacing(shape, self.boundary)
        a = np.asarray(fields).reshape(2, -1)[0]
        out, centre = {}, 0.0
        for q, off in enumerate(self.offs):
            if off == (0, 0):
                continue
            ax = 0 if off[0] != 0 else 1
            face = 0.5 * (a + a[idx[:, q]]) / (h[ax] * h[ax])      # (no Dirichlet side: every point lands on a node)
            out[(0, 0, q)] = -face
            centre = centre + face
        out[(0, 0, self.offs.index((0, 0)))] = centre
        return out

    def react(self, u, fields, p):
        uold = np.asarray(fields).reshape(2, -1)[1]
        return [p[0] * (u[0] - uold) + u[0] ** 3]

    def dreact(self, u, fields, p):
        return [[p[0] + 3.0 * u[0] ** 2]]

    def fields(self, shape):
        x, y = self.coords(shape)
        return np.concatenate([1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y), 0.3 * np.cos(2 * np.pi * x) * np.cos(np.pi * y)])


class Mixed(Problem):
    """(c) −Δu + σu + u³ with x = (dirichlet, mirror_face), y = (mirror_node, mirror_node)"""

    def __init__(self):
        sides = ("dirichlet", "mirror_face", "mirror_node", "mirror_node")
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {\n"
               + _H2 % (_extra(sides, 0), _extra(sides, 1)) +
               "  const T c = u(0, 0);\n"
               "  f[0] = cx * (2.0 * c - u(-1, 0) - u(1, 0)) + cy * (2.0 * c - u(0, -1) - u(0, 1)) + p[0] * c + c * c * c;\n}\n")
        super().__init__("mixed", src, sides, STAR2, [10.0])

    def stencil_coef(self, shape, fields, p, idx):
        return _laplace_coef(self.offs, spacing(shape, self.boundary))

    def react(self, u, fields, p):
        return [p[0] * u[0] + u[0] ** 3]

    def dreact(self, u, fields, p):
        return [[p[0] + 3.0 * u[0] ** 2]]


class Coupled(Problem):
    """(d) two components on the torus: −Δu + σu + κv + u³, −D Δv + σv − κu"""
    dof = 2

    def __init__(self):
        sides = ("periodic",) * 4
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {\n"
               + _H2 % (_extra(sides, 0), _extra(sides, 1)) +
               "  const T a = u(0, 0, 0), b = u(0, 0, 1);\n"
               "  f[0] = cx * (2.0 * a - u(-1, 0, 0) - u(1, 0, 0)) + cy * (2.0 * a - u(0, -1, 0) - u(0, 1, 0)) + p[0] * a + p[1] * b"
               " + a * a * a;\n"
               "  f[1] = (p[2] * cx) * (2.0 * b - u(-1, 0, 1) - u(1, 0, 1)) + (p[2] * cy) * (2.0 * b - u(0, -1, 1) - u(0, 1, 1))"
               " + p[0] * b - p[1] * a;\n}\n")
        super().__init__("coupled", src, sides, STAR2, [20.0, 5.0, 0.25])

    def stencil_coef(self, shape, fields, p, idx):
        h = spacing(shape, self.boundary)
        return _laplace_coef(self.offs, h, p[2], 1, _laplace_coef(self.offs, h))

    def react(self, u, fields, p):
        return [p[0] * u[0] + p[1] * u[1] + u[0] ** 3, p[0] * u[1] - p[1] * u[0]]

    def dreact(self, u, fields, p):
        return [[p[0] + 3.0 * u[0] ** 2, p[1]], [-p[1], p[0]]]


class Star3(Problem):
    """(e) −Δu + σu + u³ on the 3-D 7-point star: x and y Dirichlet, z mirror_face"""

    def __init__(self):
        sides = ("dirichlet",) * 4 + ("mirror_face",) * 2
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f) {\n"
               "  const nk_real hx = 1.0 / (s.nx + 1.0), hy = 1.0 / (s.ny + 1.0), hz = 1.0 / (s.nz + 0.0);\n"
               "  const nk_real cx = 1.0 / (hx * hx), cy = 1.0 / (hy * hy), cz = 1.0 / (hz * hz);\n"
               "  const T c = u(0, 0, 0);\n"
               "  f[0] = cx * (2.0 * c - u(-1, 0, 0) - u(1, 0, 0)) + cy * (2.0 * c - u(0, -1, 0) - u(0, 1, 0))"
               " + cz * (2.0 * c - u(0, 0, -1) - u(0, 0, 1)) + p[0] * c + c * c * c;\n}\n")
        super().__init__("star3", src, sides, STAR3, [10.0])

    def stencil_coef(self, shape, fields, p, idx):
        return _laplace_coef(self.offs, spacing(shape, self.boundary))

    def react(self, u, fields, p):
        return [p[0] * u[0] + u[0] ** 3]

    def dreact(self, u, fields, p):
        return [[p[0] + 3.0 * u[0] ** 2]]


class Fourth(Problem):
    """(f) the fourth-order Laplacian (1, −16, 30, −16, 1)/(12 h²) per axis on "star2", Dirichlet (both ghost layers read 0),
    plus σu + u³: radius 2, so coarsening stops at side 5"""
    stencil, radius = "star2", 2

    def __init__(self):
        sides = ("dirichlet",) * 4
        src = ("template <typename T>\n__device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f) {\n"
               + _H2 % (_extra(sides, 0), _extra(sides, 1)) +
               "  const nk_real qx = cx * (1.0 / 12.0), qy = cy * (1.0 / 12.0);\n"
               "  const T c = u(0, 0);\n"
               "  f[0] = qx * (30.0 * c - 16.0 * (u(-1, 0) + u(1, 0)) + (u(-2, 0) + u(2, 0)))"
               " + qy * (30.0 * c - 16.0 * (u(0, -1) + u(0, 1)) + (u(0, -2) + u(0, 2))) + p[0] * c + c * c * c;\n}\n")
        super().__init__("fourth", src, sides, STAR2_R2, [10.0])

    def stencil_coef(self, shape, fields, p, idx):
        h = spacing(shape, self.boundary)
        out = {}
        for q, off in enumerate(self.offs):
            if off == (0, 0):
                out[(0, 0, q)] = sum(30.0 / (12.0 * x * x) for x in h)
            else:
                ax = 0 if off[0] != 0 else 1
                out[(0, 0, q)] = (-16.0 if abs(off[ax]) == 1 else 1.0) / (12.0 * h[ax] * h[ax])
        return out

    def react(self, u, fields, p):
        return [p[0] * u[0] + u[0] ** 3]

    def dreact(self, u, fields, p):
        return [[p[0] + 3.0 * u[0] ** 2]]


PROBLEMS = {p.name: p for p in [Bratu(), Channel(), Mixed(), Coupled(), Star3(), Fourth()]}


def linearisation_point(prob, shape, amp=0.5):
    """a smooth u of moderate size, the same on every grid"""
    xs = prob.coords(shape)
    base = amp * np.prod([np.sin(np.pi * (x + 0.15 * (a + 1))) for a, x in enumerate(xs)], axis=0)
    return np.concatenate([base * (1.0 - 0.4 * c) for c in range(prob.dof)])


# ------------------------------------------------------------------------------------------------ the V-cycle
class GridMultigrid:
    """M(v) = one V-cycle of the hierarchy of `prob` on `shape`, linearised at u with `fields` and p"""

    def __init__(self, prob, shape, u, fields=None, p=None, nu=2, coarse_max=8):
        self.nu = int(nu) if nu > 0 else 2
        self.shapes = level_shapes(shape, prob.boundary, prob.radius, coarse_max)
        self.levels = []
        ul = np.asarray(u, dtype=np.float64)
        fl = None if fields is None else np.asarray(fields, dtype=np.float64)
        for l, shp in enumerate(self.shapes):
            A = prob.jac(shp, ul, fl, p)
            D = A.diagonal()
            lev = dict(shape=shp, A=A, dinv=1.0 / D, u=ul, fields=fl,
                       rho=float(np.max(np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(D))))
            self.levels.append(lev)
            if l + 1 < len(self.shapes):
                P1, R1 = transfers(shp, self.shapes[l + 1], prob.boundary)
                lev["P"] = sp.kron(sp.identity(prob.dof), P1, format="csr")
                lev["R"] = sp.kron(sp.identity(prob.dof), R1, format="csr")
                ul = lev["R"] @ ul
                if fl is not None:
                    fl = sp.kron(sp.identity(prob.nfields), R1, format="csr") @ fl
        self.lu = spla.splu(sp.csc_matrix(self.levels[-1]["A"])) if len(self.levels) > 1 else None

    def _smooth(self, lev, x, b, zero_guess):
        lmax, lmin = lev["rho"], lev["rho"] / 4.0
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sigma = theta / delta
        rho = 1.0 / sigma
        A, dinv = lev["A"], lev["dinv"]
        z = b * dinv if zero_guess else (b - A @ x) * dinv
        d = z / theta
        x = d.copy() if zero_guess else x + d
        for _ in range(1, self.nu):
            rho_new = 1.0 / (2.0 * sigma - rho)
            z = (b - A @ x) * dinv
            d = rho_new * rho * d + 2.0 * rho_new / delta * z
            x = x + d
            rho = rho_new
        return x

    def __call__(self, v):
        Lv = self.levels
        v = np.asarray(v, dtype=np.float64)
        if len(Lv) == 1:
            return self._smooth(Lv[0], None, v, True)
        bs, xs = [v], []
        for l in range(len(Lv) - 1):
            x = self._smooth(Lv[l], None, bs[l], True)
            xs.append(x)
            bs.append(Lv[l]["R"] @ (bs[l] - Lv[l]["A"] @ x))
        e = self.lu.solve(bs[-1])
        for l in range(len(Lv) - 2, -1, -1):
            e = self._smooth(Lv[l], xs[l] + Lv[l]["P"] @ e, bs[l], False)
        return e


def sparse_newton(prob, shape, u0, fields=None, p=None, tol=1e-12, maxiters=50):
    """plain Newton with sparse direct solves on the restatement"""
    u = np.array(u0, dtype=np.float64)
    for _ in range(maxiters):
        f = prob.residual(shape, u, fields, p)
        if np.max(np.abs(f)) <= tol * max(1.0, np.max(np.abs(u)) / min(spacing(shape, prob.boundary)) ** 2):
            break
        u = u - spla.spsolve(sp.csc_matrix(prob.jac(shape, u, fields, p)), f)
    return u


@functools.lru_cache(maxsize=None)
def reference(name, shape, coarse_max, nu=2, variant=0):
    """the shared reference of a case (computed once, not modified by its users): u, fields, b, the hierarchy, the result of
    one GMRES iteration with the V-cycle as right preconditioner and the iteration count to rtol 1e-9. variant = 1: other fields
    and another p (what the update tests switch to)"""
    from oracle import reference_restatement as R
    prob = PROBLEMS[name]
    u = linearisation_point(prob, shape)
    fields, p = prob.fields(shape), list(prob.params)
    if variant == 1:
        p[0] = 1.5 * p[0]
        if fields is not None:
            x, y = prob.coords(shape)[:2]
            fields = fields + np.concatenate([0.3 * np.cos(2 * np.pi * x) * np.cos(2 * np.pi * y), 0.1 * np.sin(2 * np.pi * x)])
    M = GridMultigrid(prob, shape, u, fields, p, nu, coarse_max)
    J = M.levels[0]["A"]
    b = np.random.default_rng(7 + len(name)).standard_normal(J.shape[0])
    x1, _ = R.gmres(lambda z: J @ z, b, restart=30, fixed_iters=1, M=M, ortho="cgs2")
    x, info = R.gmres(lambda z: J @ z, b, rtol=1e-9, restart=30, itmax=300, M=M, ortho="cgs2")

    class Ref:
        pass
    ref = Ref()
    ref.prob, ref.u, ref.fields, ref.p, ref.M, ref.J, ref.b, ref.x1, ref.x, ref.iters = prob, u, fields, p, M, J, b, x1, x, info.iters
    for arr in (u, fields, b, x1, x):
        if isinstance(arr, np.ndarray):
            arr.setflags(write=False)
    return ref
