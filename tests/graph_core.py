"""The NumPy restatement of the compiled graph problems (csrc/nk_graph.hip): graphs, seeded data, the CSR pattern with its
slot numbering, and the evaluation of a problem's node formula in float64 and in long double with the bound the device tests
use. tests/graph_reference.py is the table on top of it: graphs, HIP sources and the same formula in NumPy.

Layout: unknown c of node i is element c·nn + i; edge datum k of edge e (its position in colind) is W[k, e], node datum k of
node i is A[k, i]. Row (c, i) of the Jacobian holds, for c2 = 0 .. dof − 1, node i and its neighbours in ascending node order
(its deg_i + 1 slots; the self slot is spos_i = the number of neighbours smaller than i, edge e is slot e + (e >= spos_i)); the
value of dF_c(i)/du_c2(slot s) is element c·dof·(ne + nn) + dof·(rowptr[i] + i) + c2·(deg_i + 1) + s.

A problem's formula is ONE Python function node(u, p, s) written like its HIP source — u.self(c), u.deg(), u.nbr(e, c),
u.node(e), u.w(e, k), u.a(k), u.an(e, k), s.i, s.nn, s.deg, a loop over the edges — and run through two views:

    VecNbrs     all nodes (or all slots) at once on arrays of one floating-point type. The numbers are Num: a value, NK_CH
                partials combined by the rules of the device's dual numbers in the device's operation order (so a formula
                without an elementary function agrees with the device bit for bit), and the Σ|terms| of the value and of every
                partial. Seeds: none (the residual), the one partial from v (J·v), or unit seeds on the dof unknowns of the
                instance's slot (the CSR values: one instance per slot, as the device's fill has one thread per slot).
    ScalarNbrs  one node at a time on NumPy scalars with plain Python loops: an independent walk over the edges and the data,
                which the vectorised residual is held against (tests/test_graph_reference.py).

Sums run in edge order: `for e in u.edges(): acc = u.add(e, acc, term)` adds the term of edge e to the nodes that have one.
Σ|terms|: a leaf's is its absolute value, a sum's the sum, a product's the product, and g(a) for g = exp, sin, cos has
|g(a)| + |g'(a)|·Σ|terms of a| when a is itself computed (a rounded argument moves g by g'·δ). The tolerance rule is
grid_core's, with its MARGIN and FLOOR_ULPS:

    |device − float64 restatement| <= MARGIN × |float64 − long double| + FLOOR_ULPS eps × Σ|terms|

Seeded u and v have |u| <= 1. `defect=` plants one of DEFECTS into the vectorised evaluation, for the tests that show the
assertions reject it."""
import numpy as np

from grid_core import EPS, FLOOR_ULPS, LD, MARGIN

DEFECTS = ("self_slot_off_by_one", "transposed_block", "dropped_last_edge", "datum_by_neighbour", "no_self_seed")


# ------------------------------------------------------------------------------------------------ graphs
class Graph:
    """a CSR adjacency: 0-based, columns strictly ascending within a row, no self-loops"""

    def __init__(self, name, nn, pairs):
        """pairs: directed edges (i, j), i's row gets column j"""
        self.name, self.nn = name, int(nn)
        rows = [[] for _ in range(self.nn)]
        for i, j in pairs:
            assert 0 <= i < nn and 0 <= j < nn and i != j
            rows[i].append(int(j))
        rows = [sorted(set(r)) for r in rows]
        self.deg = np.array([len(r) for r in rows], dtype=np.int64)
        self.rowptr = np.concatenate([[0], np.cumsum(self.deg)]).astype(np.int64)
        self.colind = np.array([j for r in rows for j in r], dtype=np.int64)
        self.ne = int(self.colind.size)
        self.rows = np.repeat(np.arange(self.nn), self.deg)                  # the node of every edge
        self.spos = np.array([sum(1 for j in r if j < i) for i, r in enumerate(rows)], dtype=np.int64)
        self.slot_node = np.repeat(np.arange(self.nn), self.deg + 1)        # the node of every global slot
        self.slot_s = np.arange(self.ne + self.nn) - (self.rowptr[self.slot_node] + self.slot_node)
        self.symmetric = set(zip(self.rows.tolist(), self.colind.tolist())) == set(zip(self.colind.tolist(), self.rows.tolist()))

    def csr(self):
        return self.rowptr.astype(np.int32), self.colind.astype(np.int32)

    def edge_of(self):
        """(i, j) → edge index"""
        return {(int(i), int(j)): e for e, (i, j) in enumerate(zip(self.rows, self.colind))}


def undirected(name, nn, pairs):
    return Graph(name, nn, [(i, j) for i, j in pairs] + [(j, i) for i, j in pairs])


def single():
    return Graph("single", 1, [])


def directed3():
    """edges 0→1 and 2→1 only: the residuals of nodes 0 and 2 read node 1, node 1 has degree 0"""
    return Graph("directed3", 3, [(0, 1), (2, 1)])


def tri(nx, ny, seed, permuted):
    """a grid's 4 neighbours plus one random diagonal per cell, symmetric, degrees 2–8, optionally renumbered at random"""
    rng = np.random.default_rng(7000 + 100 * seed + 3 * nx + ny)
    perm = rng.permutation(nx * ny) if permuted else np.arange(nx * ny)
    at = lambda i, j: int(perm[j * nx + i])   # noqa: E731
    pairs = []
    for j in range(ny):
        for i in range(nx):
            if i + 1 < nx:
                pairs.append((at(i, j), at(i + 1, j)))
            if j + 1 < ny:
                pairs.append((at(i, j), at(i, j + 1)))
            if i + 1 < nx and j + 1 < ny:
                pairs.append((at(i, j), at(i + 1, j + 1)) if rng.integers(2) else (at(i + 1, j), at(i, j + 1)))
    return undirected(f"tri{nx}x{ny}{'p' if permuted else 'n'}{seed}", nx * ny, pairs)


def ring(n):
    return undirected(f"ring{n}", n, [(i, (i + 1) % n) for i in range(n)])


def hub(n, centre):
    """node `centre` joined to all others, which also form a ring"""
    others = [i for i in range(n) if i != centre]
    pairs = [(centre, i) for i in others] + [(others[k], others[(k + 1) % len(others)]) for k in range(len(others))]
    return undirected(f"hub{n}", n, pairs)


def pattern(G, dof):
    """CSR pattern (rowptr, colind), int32, row by row from the definition: for every component c2 the sorted set of the node
    and its neighbours"""
    rp, ci = [0], []
    for c in range(dof):
        for i in range(G.nn):
            cols = sorted(G.colind[G.rowptr[i]:G.rowptr[i + 1]].tolist() + [i])
            for c2 in range(dof):
                ci.extend(c2 * G.nn + j for j in cols)
            rp.append(len(ci))
    return np.array(rp, dtype=np.int32), np.array(ci, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ numbers
class Num:
    """value v, partials d[0 .. CH), Σ|terms| m of the value and dm[t] of every partial; the rules and the operation order of
    the device's Dual (csrc/nk_rtc.hip). leaf: read from u, not computed"""
    __array_ufunc__ = None

    def __init__(self, v, d, m, dm, leaf=False):
        self.v, self.d, self.m, self.dm, self.leaf = v, d, m, dm, leaf

    @staticmethod
    def const(x, like):
        z = np.zeros_like(like.v)
        return Num(x + z, [z for _ in like.d], np.abs(x) + z, [z for _ in like.d])

    def inexact(self):
        return 0.0 * self.m if self.leaf else self.m

    def __add__(self, o):
        if isinstance(o, Num):
            return Num(self.v + o.v, [a + b for a, b in zip(self.d, o.d)], self.m + o.m, [a + b for a, b in zip(self.dm, o.dm)])
        return Num(self.v + o, list(self.d), self.m + np.abs(o), list(self.dm))

    __radd__ = __add__

    def __neg__(self):
        return Num(-self.v, [-a for a in self.d], self.m, list(self.dm))

    def __sub__(self, o):
        if isinstance(o, Num):
            return Num(self.v - o.v, [a - b for a, b in zip(self.d, o.d)], self.m + o.m, [a + b for a, b in zip(self.dm, o.dm)])
        return Num(self.v - o, list(self.d), self.m + np.abs(o), list(self.dm))

    def __rsub__(self, o):   # o − self: the device negates, then adds
        return Num(-self.v + o, [-a for a in self.d], self.m + np.abs(o), list(self.dm))

    def __mul__(self, o):
        if isinstance(o, Num):
            return Num(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)], self.m * o.m,
                       [a * o.m + self.m * b for a, b in zip(self.dm, o.dm)])
        return Num(self.v * o, [a * o for a in self.d], self.m * np.abs(o), [a * np.abs(o) for a in self.dm])

    __rmul__ = __mul__


def _chain(a, g, dg, ddg):
    """g(a) with g' = dg and |g''| <= ddg at a.v"""
    ix = a.inexact()
    return Num(g, [dg * x for x in a.d], np.abs(g) + np.abs(dg) * ix, [np.abs(dg) * x + ddg * ix * x for x in a.dm])


def gexp(a):
    if not isinstance(a, Num):
        return np.exp(a)
    e = np.exp(a.v)
    return _chain(a, e, e, np.abs(e))


def gsin(a):
    if not isinstance(a, Num):
        return np.sin(a)
    return _chain(a, np.sin(a.v), np.cos(a.v), np.abs(np.sin(a.v)))


def gcos(a):
    if not isinstance(a, Num):
        return np.cos(a)
    return _chain(a, np.cos(a.v), -np.sin(a.v), np.abs(np.cos(a.v)))


# ------------------------------------------------------------------------------------------------ the two views
class Vertex:
    def __init__(self, i, nn, deg):
        self.i, self.nn, self.deg = i, nn, deg


class VecNbrs:
    """all instances at once. An instance is a node (seeds "none" and "v") or a slot of a node (seeds "unit")"""

    def __init__(self, G, U, V, W, A, T, node, slot, seeds, defect=None):
        self.G, self.U, self.V, self.W, self.A, self.T, self.i, self.slot, self.seeds, self.defect = G, U, V, W, A, T, node, slot, seeds, defect
        self.dof = U.shape[0]
        self.dg = G.deg[node]
        self.e0 = G.rowptr[node]
        self.spos = G.spos[node]
        if defect == "self_slot_off_by_one":
            self.spos = (self.spos + 1) % (self.dg + 1)
        self.live = self.dg - 1 if defect == "dropped_last_edge" else self.dg   # edges the loop visits
        self.ch = {"none": 0, "v": 1, "unit": self.dof}[seeds]

    def vertex(self):
        return Vertex(self.i, self.G.nn, self.dg)

    def deg(self):
        return self.dg

    def edges(self):
        return range(int(self.live.max()) if self.live.size else 0)

    def _eid(self, e):
        """the edge of position e in every instance's row (any valid edge where the row is shorter: the value is masked out)"""
        return np.minimum(self.e0 + np.minimum(e, np.maximum(self.dg - 1, 0)), max(self.G.ne - 1, 0))

    def _leaf(self, c, at, hot):
        T, x = self.T, self.U[c][at]
        if self.seeds == "none":
            d = []
        elif self.seeds == "v":
            d = [self.V[c][at]]
        else:
            d = [np.where(hot & (t == c), T(1), T(0)).astype(T) for t in range(self.dof)]
        return Num(x, d, np.abs(x), [np.abs(y) for y in d], leaf=True)

    def self(self, c=0):
        hot = (self.slot == self.spos) if self.seeds == "unit" else None
        if self.defect == "no_self_seed" and self.seeds == "unit":
            hot = hot & False
        return self._leaf(c, self.i, hot)

    def nbr(self, e, c=0):
        hot = (self.slot == e + (e >= self.spos)) if self.seeds == "unit" else None
        return self._leaf(c, self.G.colind[self._eid(e)], hot)

    def node(self, e):
        return self.G.colind[self._eid(e)]

    def w(self, e, k=0):
        eid = self._eid(e)
        if self.defect == "datum_by_neighbour":
            eid = self.G.colind[eid] % max(self.G.ne, 1)
        return self.W[k][eid]

    def a(self, k=0):
        return self.A[k][self.i]

    def an(self, e, k=0):
        return self.A[k][self.G.colind[self._eid(e)]]

    def real(self, x):
        return np.asarray(x).astype(self.T)

    def zero(self):
        z = np.zeros(self.i.size, dtype=self.T)
        return Num(z, [z for _ in range(self.ch)], z, [z for _ in range(self.ch)])

    def where(self, mask, x, y):
        like = x if isinstance(x, Num) else y
        x = x if isinstance(x, Num) else Num.const(x, like)
        y = y if isinstance(y, Num) else Num.const(y, like)
        pick = lambda a, b: np.where(mask, a, b)   # noqa: E731
        return Num(pick(x.v, y.v), [pick(a, b) for a, b in zip(x.d, y.d)], pick(x.m, y.m), [pick(a, b) for a, b in zip(x.dm, y.dm)])

    def add(self, e, acc, term):
        """acc + term where the instance's node has an edge e, acc elsewhere"""
        return self.where(self.live > e, acc + term, acc)


class ScalarNbrs:
    """one node, NumPy float64 scalars, plain loops"""

    def __init__(self, G, U, W, A, i):
        self.G, self.U, self.W, self.A, self.i = G, U, W, A, i
        self.nbrs = [int(j) for j in G.colind[G.rowptr[i]:G.rowptr[i + 1]]]
        self.first = int(G.rowptr[i])

    def vertex(self):
        return Vertex(self.i, self.G.nn, len(self.nbrs))

    def deg(self):
        return len(self.nbrs)

    def edges(self):
        return range(len(self.nbrs))

    def self(self, c=0):
        return self.U[c][self.i]

    def nbr(self, e, c=0):
        return self.U[c][self.nbrs[e]]

    def node(self, e):
        return self.nbrs[e]

    def w(self, e, k=0):
        return self.W[k][self.first + e]

    def a(self, k=0):
        return self.A[k][self.i]

    def an(self, e, k=0):
        return self.A[k][self.nbrs[e]]

    def real(self, x):
        return np.float64(x)

    def zero(self):
        return np.float64(0.0)

    def where(self, mask, x, y):
        return x if mask else y

    def add(self, e, acc, term):
        return acc + term


# ------------------------------------------------------------------------------------------------ the cases
class Problem:
    """a HIP source and the same formula in NumPy. edge_ranges / node_ranges: (lo, hi) of every seeded datum; a node datum with
    the range "slack" is the flag of node 0"""

    def __init__(self, name, source, dof, params, node, edge_ranges=(), node_ranges=()):
        self.name, self.source, self.dof, self.params, self.node = name, source, dof, list(params), node
        self.edge_ranges, self.node_ranges = list(edge_ranges), list(node_ranges)
        self.nedge, self.nnode = len(self.edge_ranges), len(self.node_ranges)


def data(prob, G, seed=1):
    """(W [nedge, ne], A [nnode, nn]) float64, seeded; on a symmetric graph an edge datum is the same in both directions"""
    rng = np.random.default_rng(5000 + 10 * seed + len(prob.name) + G.nn)
    W = np.zeros((prob.nedge, G.ne))
    eo = G.edge_of() if G.symmetric else None
    for k, (lo, hi) in enumerate(prob.edge_ranges):
        W[k] = rng.uniform(lo, hi, G.ne)
        if eo is not None:
            for (i, j), e in eo.items():
                if i > j:
                    W[k, e] = W[k, eo[(j, i)]]
    A = np.zeros((prob.nnode, G.nn))
    for k, r in enumerate(prob.node_ranges):
        if r == "slack":
            A[k, 0] = 1.0
        else:
            A[k] = rng.uniform(r[0], r[1], G.nn)
    return W, A


def inputs(prob, G, seed=0):
    """seeded u and v in [−1, 1], float64, length dof·nn"""
    rng = np.random.default_rng(1000 * seed + 13 * G.nn + G.ne + len(prob.name))
    n = prob.dof * G.nn
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


class Evaluation:
    """one problem at one (u, v, data, p) in one arithmetic: f, Jv, CSR values, Jᵀv, fill·v and the Σ|terms| of each entry"""


def _run(prob, view, p, T):
    out = prob.node(view, p, view.vertex())
    assert len(out) == prob.dof
    return [o if isinstance(o, Num) else Num.const(T(0) + o, view.zero()) for o in out]


def evaluate(prob, G, u, v, W, A, *, T=np.float64, params=None, defect=None):
    p = [T(x) for x in (prob.params if params is None else params)]
    dof, nn, S = prob.dof, G.nn, G.ne + G.nn
    U, V = np.asarray(u, dtype=T).reshape(dof, nn), np.asarray(v, dtype=T).reshape(dof, nn)
    Wt, At = np.asarray(W, dtype=T), np.asarray(A, dtype=T)
    nodes = np.arange(nn)
    E = Evaluation()
    out = _run(prob, VecNbrs(G, U, V, Wt, At, T, nodes, None, "none", defect), p, T)
    E.f, E.f_mag = np.concatenate([o.v for o in out]), np.concatenate([o.m for o in out])
    out = _run(prob, VecNbrs(G, U, V, Wt, At, T, nodes, None, "v", defect), p, T)
    E.jv, E.jv_mag = np.concatenate([o.d[0] for o in out]), np.concatenate([o.dm[0] for o in out])
    # the CSR values: one instance per global slot, unit seeds on the slot's dof unknowns
    i, s = G.slot_node, G.slot_s
    out = _run(prob, VecNbrs(G, U, V, Wt, At, T, i, s, "unit", defect), p, T)
    vals, mags = np.zeros(dof * dof * S, dtype=T), np.zeros(dof * dof * S, dtype=T)
    for c in range(dof):
        for c2 in range(dof):
            at = c * dof * S + dof * (G.rowptr[i] + i) + c2 * (G.deg[i] + 1) + s
            src = out[c2] if defect == "transposed_block" else out[c]
            k = c if defect == "transposed_block" else c2
            vals[at], mags[at] = src.d[k], src.dm[k]
    E.vals, E.vals_mag = vals, mags
    # Jᵀv and fill·v from the values
    rp, ci = pattern(G, dof)
    rows = np.repeat(np.arange(dof * nn), np.diff(rp))
    vv = np.asarray(v, dtype=T)
    E.jtv, E.jtv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.jtv, ci, vals * vv[rows])
    np.add.at(E.jtv_mag, ci, mags * np.abs(vv[rows]))
    E.spmv, E.spmv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.spmv, rows, vals * vv[ci])
    np.add.at(E.spmv_mag, rows, mags * np.abs(vv[ci]))
    return E


def scalar_residual(prob, G, u, W, A, params=None):
    """the residual node by node through ScalarNbrs (float64)"""
    p = [np.float64(x) for x in (prob.params if params is None else params)]
    U = np.asarray(u, dtype=np.float64).reshape(prob.dof, G.nn)
    f = np.zeros((prob.dof, G.nn))
    for i in range(G.nn):
        view = ScalarNbrs(G, U, np.asarray(W, dtype=np.float64), np.asarray(A, dtype=np.float64), i)
        f[:, i] = prob.node(view, p, view.vertex())
    return f.ravel()


class Reference:
    """float64 restatement, per-entry gap to long double and the bound MARGIN·gap + FLOOR_ULPS eps·Σ|terms| for f, jv, vals,
    jtv, spmv (grid_core's rule and constants)"""

    def __init__(self, prob, G, u, v, W, A, *, params=None):
        a = evaluate(prob, G, u, v, W, A, T=np.float64, params=params)
        b = evaluate(prob, G, u, v, W, A, T=LD, params=params)
        for k in ("f", "jv", "vals", "jtv", "spmv"):
            x64, x80 = getattr(a, k), getattr(b, k)
            gap = np.abs(x64.astype(LD) - x80).astype(np.float64)
            setattr(self, k, x64)
            setattr(self, k + "_gap", gap)
            setattr(self, k + "_bound", MARGIN * gap + FLOOR_ULPS * EPS * getattr(a, k + "_mag"))


_CACHE = {}


def reference(prob, G, seed=0, params=None, data_seed=1):
    """the shared reference of a case (computed once, not modified by its users): seeded u, v and data"""
    key = (prob.name, G.name, seed, None if params is None else tuple(params), data_seed)
    if key not in _CACHE:
        u, v = inputs(prob, G, seed)
        W, A = data(prob, G, data_seed)
        R = Reference(prob, G, u, v, W, A, params=params)
        R.u, R.v, R.W, R.A = u, v, W, A
        for arr in vars(R).values():
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = R
    return _CACHE[key]


def dense_jacobian(prob, G, u, W, A, *, params=None):
    """the float64 restatement's Jacobian as a dense matrix and its residual (small graphs: the reference Newton)"""
    E = evaluate(prob, G, u, np.zeros_like(u), W, A, params=params)
    rp, ci = pattern(G, prob.dof)
    n = rp.size - 1
    J = np.zeros((n, n))
    J[np.repeat(np.arange(n), np.diff(rp)), ci] = E.vals
    return J, E.f


def dense_newton(prob, G, u0, W, A, *, params=None, tol=1e-13, maxiters=50):
    """plain Newton with dense solves on the restatement: (u, steps taken)"""
    u = np.array(u0, dtype=np.float64)
    for it in range(maxiters):
        J, f = dense_jacobian(prob, G, u, W, A, params=params)
        if np.max(np.abs(f)) <= tol:
            return u, it
        u = u - np.linalg.solve(J, f)
    return u, maxiters
