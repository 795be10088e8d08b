"""NumPy restatement of the compiled grid problems WITH A KIND PER SIDE (csrc/nk_grid.hip, NK_GRID_SIDES), built on the four
earlier restatements — grid_reference, grid3_reference, grid_r2_reference, gridf_reference — whose sources and per-stencil-point
formulas it takes as they are: what is new here is where a stencil point lands, and what happens when several land on one node.

A ghost node at distance k = 1..radius outside a side of an axis of n nodes:

    "dirichlet"    reads 0, no column                              np.pad(..., "constant")
    "periodic"     wraps (both sides of the axis)                  np.pad(..., "wrap")
    "mirror_node"  −k ↦ k, n−1+k ↦ n−1−k                           np.pad(..., "reflect")
    "mirror_face"  −k ↦ k−1, n−1+k ↦ n−k                           np.pad(..., "symmetric")

Axes are independent; a point that leaves the grid through a Dirichlet side of ANY axis reads 0 and has no column, whatever the
other axes do, and a field read there is the field at the node itself. Otherwise u, v and the fields are read at the node the
axes map to. The Jacobian is the true dF/du: the analytic partial of every stencil point (the formulas of the four tables, one
per point) is ADDED into the entry of the node the point lands on, in ascending stencil-point order q — float64 and long double
— and the pattern holds that column once, columns ascending. The bound is the project's:

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms|

A boundary here is a tuple of 2·dim kinds: (x-lo, x-hi, y-lo, y-hi[, z-lo, z-hi])."""
import numpy as np

import grid3_reference as G3
import grid_r2_reference as G2
import grid_reference as G1
import gridf_reference as GF
from grid_reference import EPS, FLOOR_ULPS, LD, MARGIN   # noqa: F401  (shared)

KIND_ID = {"dirichlet": 0, "periodic": 1, "mirror_node": 2, "mirror_face": 3}
PAD_MODE = {"dirichlet": "constant", "periodic": "wrap", "mirror_node": "reflect", "mirror_face": "symmetric"}
STENCIL_ID = GF.STENCIL_ID
SIDES_BIT = 1 << 24
PAD = 2   # the largest radius


def sides_code(sides):
    """NK_GRID_SIDES of the header: one kind per 4 bits (x-lo lowest) under the marker bit; accepts names or numbers"""
    code = SIDES_BIT
    for s, k in enumerate(sides):
        code |= (KIND_ID[k] if isinstance(k, str) else int(k)) << (4 * s)
    return code


def uniform(kind, dim):
    return (kind,) * (2 * dim)


# ------------------------------------------------------------------------------------------------ where an index lands
def axis_map(n, lo, hi):
    """the node index of positions −PAD … n−1+PAD of an axis of n nodes, −1 outside a Dirichlet side: NumPy's own padding of
    the index vector, one side at a time"""
    ar = np.arange(n, dtype=np.int64)
    left = np.pad(ar, (PAD, 0), mode=PAD_MODE[lo], **({"constant_values": -1} if lo == "dirichlet" else {}))[:PAD]
    right = np.pad(ar, (0, PAD), mode=PAD_MODE[hi], **({"constant_values": -1} if hi == "dirichlet" else {}))[n:]
    return np.concatenate([left, ar, right])


def _coords(shape):
    return np.unravel_index(np.arange(int(np.prod(shape)), dtype=np.int64), tuple(shape)[::-1])[::-1]   # (i, j[, k])


def neighbours(shape, offs, sides):
    """(idx, inside): the node every stencil point of every node lands on ([nn, npts]; −1 where it left through a Dirichlet
    side of any axis)"""
    shape, nn = tuple(shape), int(np.prod(shape))
    maps = [axis_map(n, sides[2 * a], sides[2 * a + 1]) for a, n in enumerate(shape)]
    at = _coords(shape)
    idx = np.empty((nn, len(offs)), dtype=np.int64)
    for q, off in enumerate(offs):
        pos = [m[x + d + PAD] for m, x, d in zip(maps, at, off)]
        ok = np.logical_and.reduce([x >= 0 for x in pos])
        lin = np.zeros(nn, dtype=np.int64)
        for x, n in zip(pos[::-1], shape[::-1]):   # outermost direction first
            lin = lin * n + np.where(ok, x, 0)
        idx[:, q] = np.where(ok, lin, -1)
    return idx, idx >= 0


def slots(shape, dof, offs, sides):
    """(rowptr, cnt, rank, idx, inside, prim): prim[node, q] — q is the first point of the row (smallest q) that lands on its
    node; cnt = the row's distinct nodes; rank[node, q] = how many of them are smaller than q's (the same for all points that
    share a node). The entry (row c·nn + node, column c2·nn + idx[node, q]) sits at rowptr[c·nn + node] + c2·cnt[node] +
    rank[node, q]"""
    idx, inside = neighbours(shape, offs, sides)
    npts = len(offs)
    prim = inside.copy()
    for q in range(npts):
        for t in range(q):
            prim[:, q] &= ~(inside[:, t] & (idx[:, t] == idx[:, q]))
    rank = np.zeros(idx.shape, dtype=np.int64)
    for q in range(npts):
        rank[:, q] = np.sum(prim & (idx < idx[:, q:q + 1]), axis=1)
    cnt = prim.sum(axis=1)
    rowptr = np.concatenate([[0], np.cumsum(np.tile(cnt * dof, dof))]).astype(np.int64)
    return rowptr, cnt, rank, idx, inside, prim


def pattern(shape, dof, offs, sides):
    """CSR pattern (rowptr, colind), int32: every node a row's points land on once, ascending, for every component"""
    nn = int(np.prod(shape))
    rowptr, cnt, rank, idx, inside, prim = slots(shape, dof, offs, sides)
    colind = np.empty(int(rowptr[-1]), dtype=np.int64)
    nodes, qs = np.nonzero(prim)
    for c in range(dof):
        for c2 in range(dof):
            colind[rowptr[c * nn + nodes] + c2 * cnt[nodes] + rank[nodes, qs]] = c2 * nn + idx[nodes, qs]
    return rowptr.astype(np.int32), colind.astype(np.int32)


# ------------------------------------------------------------------------------------------------ grid access
class Grid:
    """N(di, dj[, dk][, c]) on whole-grid arrays [dof, (nz,) ny, nx]: component c at the node the offset lands on, 0 where it
    left through a Dirichlet side of any axis. (The call conventions of all four earlier Grid classes.)"""
    outside_is_zero = True

    def __init__(self, U, sides):
        self.U, self.sides, self.dim = U, tuple(sides), U.ndim - 1
        shape = U.shape[1:][::-1]                                   # (nx, ny[, nz])
        self.maps = [axis_map(n, self.sides[2 * a], self.sides[2 * a + 1]) for a, n in enumerate(shape)]

    def __call__(self, *a):
        off, c = a[:self.dim], (a[self.dim] if len(a) > self.dim else 0)
        A = self.U[c]
        # per axis (array order: outermost first) the landing index of every position, −1 outside a Dirichlet side
        sel = [self.maps[ax][PAD + d:PAD + d + A.shape[self.dim - 1 - ax]] for ax, d in enumerate(off)][::-1]
        out = np.zeros(A.shape, dtype=bool)
        for axis, s in enumerate(sel):
            out |= (s < 0).reshape([-1 if t == axis else 1 for t in range(self.dim)])
        moved = A[np.ix_(*[np.where(s < 0, 0, s) for s in sel])]
        return np.where(out, A.dtype.type(0) if self.outside_is_zero else A, moved)


class Fields(Grid):
    """A(di, dj[, dk][, k]): field k the same way, but a read that left through a Dirichlet side is the field at the node itself"""
    outside_is_zero = False


# ------------------------------------------------------------------------------------------------ the cases
class Problem:
    """an earlier table's problem (its source, its formulas) under another boundary. `call` adapts the three signature styles:
    grid_reference f(N, p, nx, ny, T), grid3 / grid_r2 f(N, p, shape, T), gridf f(N, A, p, shape, T)"""

    def __init__(self, name, base, sides, style, dim, params=None):
        self.name, self.base, self.boundary, self.style, self.dim = name, base, tuple(sides), style, dim
        self.source, self.dof, self.stencil = base.source, base.dof, base.stencil
        self.params = list(base.params if params is None else params)
        self.nfields = getattr(base, "nfields", 0)
        assert len(self.boundary) == 2 * dim

    def offsets(self):
        return GF.offsets(self.dim, self.stencil)

    def call(self, fn, grids, A, p, shape, T):
        if self.style == "g1":
            return fn(*grids, p, shape[0], shape[1], T)
        if self.style == "gf":
            return fn(*grids, A, p, shape, T)
        return fn(*grids, p, shape, T)


MN, MF, DI, PE = "mirror_node", "mirror_face", "dirichlet", "periodic"
PROBLEMS = {p.name: p for p in [
    Problem("bratu_mirror_node", G1.PROBLEMS["bratu"], uniform(MN, 2), "g1", 2),
    Problem("bratu_mirror_face", G1.PROBLEMS["bratu"], uniform(MF, 2), "g1", 2),
    # a channel: periodic along x, a Dirichlet-0 wall below, a symmetry line above
    Problem("bratu_channel", G1.PROBLEMS["bratu"], (PE, PE, DI, MN), "g1", 2),
    # a plate free at the low end and held at the high end of both axes: the mirror below, Dirichlet-0 above
    Problem("bratu_plate", G1.PROBLEMS["bratu"], (MF, DI, MN, DI), "g1", 2),
    Problem("brusselator_xface_yper", G1.PROBLEMS["brusselator"], (MF, MF, PE, PE), "g1", 2),
    # the 9-point box, 2 components and a cross term, mirrored in both axes (a kind of each at every corner): four points merge
    Problem("box_mirror", G1.PROBLEMS["box_dirichlet"], (MN, MF, MF, MN), "g1", 2),
    # x mirrored, y Dirichlet-0: at a corner the Dirichlet side wins
    Problem("box_xnode_ydir", G1.PROBLEMS["box_dirichlet"], (MN, MN, DI, DI), "g1", 2),
    Problem("star2_mirror", G2.PROBLEMS["upwind2_dirichlet"], (MN, MF, MF, MN), "g2", 2),
    Problem("diamond2_mirror", G2.PROBLEMS["diamond_dirichlet"], (MF, MN, MN, MF), "g2", 2),
    # the 3-D star, dof 2, three different axes: periodic, Dirichlet-0 below and mirror-node above, mirror-face
    Problem("star3_mixed", G3.PROBLEMS["brusselator3"], (PE, PE, DI, MN, MF, MF), "g3", 3),
    Problem("box3_mirror", G3.PROBLEMS["box3_dirichlet"], (MN, MF, MF, MF, MF, MN), "g3", 3),
    Problem("vardiff_mirror_face", GF.PROBLEMS["vardiff"], uniform(MF, 2), "gf", 2),
]}
# the same sources under the boundary they have in their own tables: what the conservation test and the solves compare with
DIRICHLET_TWIN = {"vardiff_mirror_face": Problem("vardiff_dirichlet", GF.PROBLEMS["vardiff"], uniform(DI, 2), "gf", 2)}


def sizes(prob):
    """each stencil's existing shapes: the smallest that reach every row wrapping or mirroring (3 × 3, 5 × 5, 3 × 3 × 3), a
    ragged last workgroup and five workgroups (37 × 29), and a long thin grid"""
    if prob.dim == 3:
        return [(3, 3, 3), (7, 6, 5), (37, 29, 3)]
    return [(5, 5), (37, 29)] if prob.stencil in G2.STENCIL_ID else [(3, 3), (37, 29), (300, 5)]


def inputs(prob, shape, seed=0):
    """seeded u and v in [−1, 1], float64, length dof·nn"""
    rng = np.random.default_rng(1000 * seed + sum(w * n for w, n in zip((49, 7, 1), shape)) + len(prob.name))
    n = prob.dof * int(np.prod(shape))
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


class Evaluation:
    """one problem at one (u, v, fields, p) in one arithmetic: f, Jv, CSR values, Jᵀv, fill·v and the Σ|terms| of each entry"""


def evaluate(prob, shape, u, v, fields=None, T=np.float64, params=None):
    shape = tuple(shape)
    p = [T(x) for x in (prob.params if params is None else params)]
    dof, nn, dim, base = prob.dof, int(np.prod(shape)), len(shape), prob.base
    N = Grid(np.asarray(u, dtype=T).reshape(dof, *shape[::-1]), prob.boundary)
    V = Grid(np.asarray(v, dtype=T).reshape(dof, *shape[::-1]), prob.boundary)
    A = Fields(np.asarray(fields, dtype=T).reshape(prob.nfields, *shape[::-1]), prob.boundary) if prob.nfields else None
    E = Evaluation()
    f, fm = prob.call(base._resid, (N,), A, p, shape, T)
    E.f, E.f_mag = np.concatenate([x.ravel() for x in f]), np.concatenate([x.ravel() for x in fm])
    jv, jm = prob.call(base._jvp, (N, V), A, p, shape, T)
    E.jv, E.jv_mag = np.concatenate([x.ravel() for x in jv]), np.concatenate([x.ravel() for x in jm])
    # CSR values: the analytic partial of every stencil point, added into the entry of the node the point lands on, in
    # ascending q (a row's first point on a node starts from 0 + x = x); points the formulas do not name add nothing
    offs = prob.offsets()
    rowptr, cnt, rank, idx, inside, _prim = slots(shape, dof, offs, prob.boundary)
    vals, mags = np.zeros(int(rowptr[-1]), dtype=T), np.zeros(int(rowptr[-1]), dtype=T)
    entries = prob.call(base._jac, (N,), A, p, shape, T)
    for key in sorted(entries, key=lambda k: offs.index(tuple(k[1:1 + dim]))):
        val, mag = entries[key]
        r, q, c2 = key[0], offs.index(tuple(key[1:1 + dim])), key[1 + dim]
        nodes = np.nonzero(inside[:, q])[0]
        pos = rowptr[r * nn + nodes] + c2 * cnt[nodes] + rank[nodes, q]     # (one position per node: no repeats within a q)
        vals[pos] = vals[pos] + np.broadcast_to(val, shape[::-1]).ravel()[nodes]
        mags[pos] = mags[pos] + np.broadcast_to(mag, shape[::-1]).ravel()[nodes]
    E.vals, E.vals_mag = vals, mags
    rp, ci = pattern(shape, dof, offs, prob.boundary)
    rows = np.repeat(np.arange(dof * nn), np.diff(rp))
    vv = np.asarray(v, dtype=T)
    E.jtv, E.jtv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.jtv, ci, vals * vv[rows])
    np.add.at(E.jtv_mag, ci, np.abs(vals * vv[rows]))
    E.spmv, E.spmv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.spmv, rows, vals * vv[ci])
    np.add.at(E.spmv_mag, rows, np.abs(vals * vv[ci]))
    return E


class Reference:
    """float64 restatement, per-entry gap to long double and the bound 16·gap + 4 eps·Σ|terms| for f, jv, vals, jtv, spmv"""

    def __init__(self, prob, shape, u, v, fields=None, params=None):
        a, b = evaluate(prob, shape, u, v, fields, np.float64, params), evaluate(prob, shape, u, v, fields, LD, params)
        for k in ("f", "jv", "vals", "jtv", "spmv"):
            x64, x80 = getattr(a, k), getattr(b, k)
            gap = np.abs(x64.astype(LD) - x80).astype(np.float64)
            setattr(self, k, x64)
            setattr(self, k + "_gap", gap)
            setattr(self, k + "_bound", MARGIN * gap + FLOOR_ULPS * EPS * getattr(a, k + "_mag"))


_CACHE = {}


def reference(name, shape, seed=0):
    """the shared reference of a case (computed once, not modified by its users): seeded u, v and fields"""
    shape = tuple(shape)
    key = (name, shape, seed)
    if key not in _CACHE:
        prob = PROBLEMS[name]
        u, v = inputs(prob, shape, seed)
        fields = GF.seeded_fields(prob.nfields, shape) if prob.nfields else None
        R = Reference(prob, shape, u, v, fields)
        R.u, R.v, R.fields = u, v, fields
        for arr in vars(R).values():
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = R
    return _CACHE[key]


def dense_jacobian(prob, shape, u, fields=None, params=None):
    """the float64 restatement's Jacobian as a dense matrix and its residual (small grids: the reference Newton)"""
    E = evaluate(prob, shape, u, np.zeros_like(u), fields, np.float64, params)
    rp, ci = pattern(shape, prob.dof, prob.offsets(), prob.boundary)
    n = rp.size - 1
    J = np.zeros((n, n))
    J[np.repeat(np.arange(n), np.diff(rp)), ci] = E.vals
    return J, E.f


def dense_newton(prob, shape, u0, fields=None, params=None, tol=1e-13, maxiters=50):
    """plain Newton with dense solves on the restatement"""
    u = np.array(u0, dtype=np.float64)
    for _ in range(maxiters):
        J, f = dense_jacobian(prob, shape, u, fields, params)
        if np.max(np.abs(f)) <= tol:
            break
        u = u - np.linalg.solve(J, f)
    return u
