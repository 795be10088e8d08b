"""The one NumPy restatement of the compiled grid problems (csrc/nk_grid.hip): where a stencil point lands, the CSR pattern, the
access to u, v and the fields, and the evaluation of a problem's formulas in float64 and in long double with the bound the
device tests use. The family modules — grid_reference, grid3_reference, grid_r2_reference, gridf_reference, gridbc_reference,
gridmr_reference — are tables on top of it: HIP sources, the formulas of each source with their ANALYTIC derivatives, and sizes.

Layout: unknown c of node (i, j[, k]) is element c·nn + ((k·ny) + j)·nx + i; a shape is (nx, ny[, nz]), an offset (di, dj[, dk]).
STENCILS is the Python twin of k_grid_stencils: the points of every stencil in pattern order (ascending node index inside the
grid). A boundary is "dirichlet", "periodic" or a tuple of 2·dim kinds (x-lo, x-hi, y-lo, y-hi[, z-lo, z-hi]); a ghost node at
distance k = 1..radius outside a side of an axis of n nodes:

    "dirichlet"    reads 0, no column                              np.pad(..., "constant")
    "periodic"     wraps (both sides of the axis)                  np.pad(..., "wrap")
    "mirror_node"  −k ↦ k, n−1+k ↦ n−1−k                           np.pad(..., "reflect")
    "mirror_face"  −k ↦ k−1, n−1+k ↦ n−k                           np.pad(..., "symmetric")

Axes are independent; a point that leaves the grid through a Dirichlet side of ANY axis reads 0 and has no column, whatever the
other axes do, and a field read there is the field at the node itself. Otherwise u, v and the fields are read at the node the
axes map to. The Jacobian is the true dF/du: the analytic partial of every stencil point (one formula per point) is ADDED into
the entry of the node the point lands on, in ascending stencil-point order q — float64 and long double — and the pattern holds
that column once, columns ascending. The formulas are resid(N, A, p, shape, T), jvp(N, V, A, p, shape, T) and
jac(N, A, p, shape, T), A = None without fields; each returns its values and the Σ|terms| of every entry. The bound:

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms|

(the rule of tests/test_gpu_broyden.py). Seeded inputs have |u| <= 1; seeded fields are 1 + 0.37·sin(0.9·m + k): positive,
distinct at every node, constants of the differentiation."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
MARGIN, FLOOR_ULPS = 16.0, 4.0

KIND_ID = {"dirichlet": 0, "periodic": 1, "mirror_node": 2, "mirror_face": 3}
PAD_MODE = {"dirichlet": "constant", "periodic": "wrap", "mirror_node": "reflect", "mirror_face": "symmetric"}
BOUNDARY_ID = {"dirichlet": 0, "periodic": 1}
SIDES_BIT = 1 << 24
PAD = 2   # the largest radius

STENCILS = {
    (2, "star"): [(0, -1), (-1, 0), (0, 0), (1, 0), (0, 1)],
    (2, "box"): [(di, dj) for dj in (-1, 0, 1) for di in (-1, 0, 1)],
    (3, "star"): [(0, 0, -1), (0, -1, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)],
    (3, "box"): [(di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)],
    (2, "star2"): [(0, -2), (0, -1), (-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0), (0, 1), (0, 2)],
    (2, "diamond2"): [(di, dj) for dj in range(-2, 3) for di in range(-2, 3) if abs(di) + abs(dj) <= 2],
    (3, "star2"): [(0, 0, -2), (0, 0, -1), (0, -2, 0), (0, -1, 0), (-2, 0, 0), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0),
                   (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2)],
}
STENCIL_ID = {"star": 0, "box": 1, "star2": 16, "diamond2": 17}
RADIUS = {"star": 1, "box": 1, "star2": 2, "diamond2": 2}


def uniform(kind, dim):
    return (kind,) * (2 * dim)


def sides(boundary, dim):
    """the canonical tuple of 2·dim kinds of "dirichlet", "periodic" or a tuple of kinds"""
    out = uniform(boundary, dim) if isinstance(boundary, str) else tuple(boundary)
    assert len(out) == 2 * dim
    return out


def sides_code(sides):
    """NK_GRID_SIDES of the header: one kind per 4 bits (x-lo lowest) under the marker bit; accepts names or numbers"""
    code = SIDES_BIT
    for s, k in enumerate(sides):
        code |= (KIND_ID[k] if isinstance(k, str) else int(k)) << (4 * s)
    return code


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


def stencil_pattern(shape, dof=1, stencil="star", boundary="dirichlet"):
    """the pattern by the names nk_grid_pattern takes"""
    return pattern(shape, dof, STENCILS[(len(shape), stencil)], sides(boundary, len(shape)))


# ------------------------------------------------------------------------------------------------ grid access
class Grid:
    """N(di, dj[, dk][, c]) on whole-grid arrays [dof, (nz,) ny, nx] of one floating-point type: component c at the node the
    offset lands on, 0 where it left through a Dirichlet side of any axis"""
    outside_is_zero = True

    def __init__(self, U, boundary):
        self.U, self.dim = U, U.ndim - 1
        self.sides = sides(boundary, self.dim)
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


def seeded_fields(nfields, shape, shift=0.0):
    """[nfields, nn] float64: 1 + 0.37·sin(0.9·m + k + shift)"""
    m = np.arange(int(np.prod(shape)), dtype=np.float64)
    return np.stack([1.0 + 0.37 * np.sin(0.9 * m + k + shift) for k in range(nfields)])


def _site(shape):
    """(i, j[, k]) as float64 arrays of the grid's shape [(nz,) ny, nx]"""
    at = np.meshgrid(*[np.arange(n) for n in shape[::-1]], indexing="ij")[::-1]
    return [x.astype(np.float64) for x in at]


def _sum(terms):
    """left-to-right sum of the terms and the sum of their absolute values"""
    s, m = terms[0], np.abs(terms[0])
    for t in terms[1:]:
        s = s + t
        m = m + np.abs(t)
    return s, m


def _wsum(N, offs, w, c):
    """Σ w[t]·N(offs[t], c), left to right, and Σ|terms|"""
    return _sum([w[t] * N(*offs[t], c) for t in range(len(offs))])


# ------------------------------------------------------------------------------------------------ the cases
class Problem:
    """a HIP source and its NumPy formulas on a stencil under a boundary. `boundary` is what CompiledGridProblem is handed (a
    string or a tuple of kinds), `sides` its canonical tuple; `seed_weights` are the weights of the shape in the seed of inputs"""

    def __init__(self, name, source, dim, dof, stencil, boundary, params, resid, jvp, jac, nfields=0, seed_weights=(49, 7, 1)):
        self.name, self.source, self.dim, self.dof, self.stencil, self.boundary = name, source, dim, dof, stencil, boundary
        self.params, self.nfields, self.resid, self.jvp, self.jac = list(params), nfields, resid, jvp, jac
        self.seed_weights, self.sides = seed_weights, sides(boundary, dim)

    def offsets(self):
        return STENCILS[(self.dim, self.stencil)]

    def with_boundary(self, name, sides, params=None):
        """the same source and formulas under a kind per side"""
        return Problem(name, self.source, self.dim, self.dof, self.stencil, tuple(sides), self.params if params is None else params,
                       self.resid, self.jvp, self.jac, self.nfields)


def inputs(prob, shape, seed=0):
    """seeded u and v in [−1, 1], float64, length dof·nn"""
    rng = np.random.default_rng(1000 * seed + sum(w * n for w, n in zip(prob.seed_weights, shape)) + len(prob.name))
    n = prob.dof * int(np.prod(shape))
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


class Evaluation:
    """one problem at one (u, v, fields, p) in one arithmetic: f, Jv, CSR values, Jᵀv, fill·v and the Σ|terms| of each entry"""


def evaluate(prob, shape, u, v, fields=None, *, T=np.float64, params=None):
    """fields: [nfields, nn] float64 (the data the device holds: converted, not recomputed, in long double)"""
    shape = tuple(shape)
    p = [T(x) for x in (prob.params if params is None else params)]
    dof, nn, dim = prob.dof, int(np.prod(shape)), len(shape)
    N = Grid(np.asarray(u, dtype=T).reshape(dof, *shape[::-1]), prob.sides)
    V = Grid(np.asarray(v, dtype=T).reshape(dof, *shape[::-1]), prob.sides)
    A = Fields(np.asarray(fields, dtype=T).reshape(prob.nfields, *shape[::-1]), prob.sides) if prob.nfields else None
    E = Evaluation()
    f, fm = prob.resid(N, A, p, shape, T)
    E.f, E.f_mag = np.concatenate([x.ravel() for x in f]), np.concatenate([x.ravel() for x in fm])
    jv, jm = prob.jvp(N, V, A, p, shape, T)
    E.jv, E.jv_mag = np.concatenate([x.ravel() for x in jv]), np.concatenate([x.ravel() for x in jm])
    # CSR values: the analytic partial of every stencil point, added into the entry of the node the point lands on, in
    # ascending q (a row's first point on a node starts from 0 + x = x); points the formulas do not name add nothing
    offs = prob.offsets()
    rowptr, cnt, rank, idx, inside, _prim = slots(shape, dof, offs, prob.sides)
    vals, mags = np.zeros(int(rowptr[-1]), dtype=T), np.zeros(int(rowptr[-1]), dtype=T)
    entries = prob.jac(N, A, p, shape, T)
    for key in sorted(entries, key=lambda k: offs.index(tuple(k[1:1 + dim]))):
        val, mag = entries[key]
        r, q, c2 = key[0], offs.index(tuple(key[1:1 + dim])), key[1 + dim]
        nodes = np.nonzero(inside[:, q])[0]
        pos = rowptr[r * nn + nodes] + c2 * cnt[nodes] + rank[nodes, q]     # (one position per node: no repeats within a q)
        vals[pos] = vals[pos] + np.broadcast_to(val, shape[::-1]).ravel()[nodes]
        mags[pos] = mags[pos] + np.broadcast_to(mag, shape[::-1]).ravel()[nodes]
    E.vals, E.vals_mag = vals, mags
    # Jᵀv and fill·v from the values (the consistency test's matvec)
    rp, ci = pattern(shape, dof, offs, prob.sides)
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

    def __init__(self, prob, shape, u, v, fields=None, *, params=None):
        a = evaluate(prob, shape, u, v, fields, T=np.float64, params=params)
        b = evaluate(prob, shape, u, v, fields, T=LD, params=params)
        for k in ("f", "jv", "vals", "jtv", "spmv"):
            x64, x80 = getattr(a, k), getattr(b, k)
            gap = np.abs(x64.astype(LD) - x80).astype(np.float64)
            setattr(self, k, x64)
            setattr(self, k + "_gap", gap)
            setattr(self, k + "_bound", MARGIN * gap + FLOOR_ULPS * EPS * getattr(a, k + "_mag"))


_CACHE = {}


def reference(prob, shape, seed=0, params=None, shift=0.0, zero_fields=False):
    """the shared reference of a case (computed once, not modified by its users): seeded u, v and fields (shift moves the
    fields' phase: another set of data; zero_fields: the fields as a fresh problem holds them)"""
    shape = tuple(shape)
    key = (prob, shape, seed, None if params is None else tuple(params), shift, zero_fields)
    if key not in _CACHE:
        u, v = inputs(prob, shape, seed)
        fields = seeded_fields(prob.nfields, shape, shift) if prob.nfields else None
        if zero_fields:
            fields = fields * 0.0
        R = Reference(prob, shape, u, v, fields, params=params)
        R.u, R.v, R.fields = u, v, fields
        for arr in vars(R).values():
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = R
    return _CACHE[key]


def dense_jacobian(prob, shape, u, fields=None, *, params=None):
    """the float64 restatement's Jacobian as a dense matrix and its residual (small grids: the reference Newton)"""
    E = evaluate(prob, shape, u, np.zeros_like(u), fields, params=params)
    rp, ci = pattern(shape, prob.dof, prob.offsets(), prob.sides)
    n = rp.size - 1
    J = np.zeros((n, n))
    J[np.repeat(np.arange(n), np.diff(rp)), ci] = E.vals
    return J, E.f


def dense_newton(prob, shape, u0, fields=None, *, params=None, tol=1e-13, maxiters=50):
    """plain Newton with dense solves on the restatement"""
    u = np.array(u0, dtype=np.float64)
    for _ in range(maxiters):
        J, f = dense_jacobian(prob, shape, u, fields, params=params)
        if np.max(np.abs(f)) <= tol:
            break
        u = u - np.linalg.solve(J, f)
    return u
