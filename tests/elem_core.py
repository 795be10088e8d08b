"""The NumPy restatement of the compiled element problems (csrc/nk_elem.hip): meshes, seeded data, the node graph and the CSR
pattern, the gather order, the fixed rows, and the evaluation of a problem's element formula in float64 and in long double with
the bound the device tests use. tests/elem_reference.py is the table on top of it: meshes, HIP sources and the same formula in
NumPy.

Layout: unknown c of node i is element c·nn + i; node datum k of node i is A[k, i], element datum k of element e is W[k, e]. Two
nodes are adjacent when they share an element; the pattern is graph_core's pattern of that node graph (a Mesh holds a
graph_core.Graph built from the element's node pairs, so slots, spos and the value index are graph_core's and are not restated).

A problem's formula is ONE Python function elem(u, p, s) written like its HIP source — u.at(a, c), u.node(a), u.x(a, k), u.w(k),
s.e, s.ne, s.nn — that returns the npe·dof contributions f[a·dof + c]. It runs through two views:

    VecElem     all elements (or all (local node b, element) pairs) at once on arrays of one floating-point type. The numbers
                are graph_core's Num: a value, NK_CH partials combined by the rules of the device's dual numbers in the device's
                operation order, and the Σ|terms| of the value and of every partial. Seeds: none (the residual), the one partial
                from v (J·v), or unit seeds on the dof unknowns of local node b (the element matrices: one instance per
                (b, element), as the device's nk_elem_jac has one thread per pair).
    ScalarElem  one element at a time on NumPy scalars, accumulated into the rows element after element: an independent walk
                which the vectorised residual is held against (tests/test_elem_reference.py).

The gather adds the contributions of a row (of an entry) in ASCENDING ELEMENT ORDER starting from 0, as k_elem_gather does, and
carries Σ|terms| through the sum. A fixed row r (mask != 0) has F_r = u_r − g_r, (Jv)_r = v_r and the unit row in J. The
tolerance rule is grid_core's, with its MARGIN and FLOOR_ULPS:

    |device − float64 restatement| <= MARGIN × |float64 − long double| + FLOOR_ULPS eps × Σ|terms|

Σ|terms| of the functions graph_core lacks: a quotient a/b is the device's a·(1/b) — its terms are those of a times |1/b| plus
|a/b|·|1/b| times the inexactness of b; sqrt and pow follow graph_core's chain rule (|g| + |g'|·Σ|terms of the argument|).
Seeded u and v have |u| <= 1. `defect=` plants one of DEFECTS into the vectorised evaluation, for the tests that show the
assertions reject it."""
import numpy as np

import graph_core as GC
from graph_core import Num, _chain, gexp  # noqa: F401  (gexp: for the table)
from grid_core import EPS, FLOOR_ULPS, LD, MARGIN

DEFECTS = ("ab_transposed", "transposed_block", "dropped_last_element", "datum_by_node", "fixed_row_left_as_sum",
           "fixed_offdiagonal_kept")


# ------------------------------------------------------------------------------------------------ functions on Num
def gdiv(a, b):
    """a / b with the device's rule: ib = 1/b.v, r.v = a.v·ib, r.d = (a.d − r.v·b.d)·ib"""
    if not isinstance(b, Num):
        return a * (1.0 / b) if isinstance(a, Num) else a / b
    if not isinstance(a, Num):
        a = Num.const(a, b)
    ib = 1.0 / b.v
    rv = a.v * ib if a.d else a.v / b.v   # (without partials the device divides two nk_real)
    aib = np.abs(ib)
    m = a.m * aib + np.abs(rv) * aib * b.inexact()
    return Num(rv, [(x - rv * y) * ib for x, y in zip(a.d, b.d)], m, [(x + m * y) * aib for x, y in zip(a.dm, b.dm)])


def gsqrt(a):
    if not isinstance(a, Num):
        return np.sqrt(a)
    s = np.sqrt(a.v)
    return _chain(a, s, 0.5 / s, 0.25 / (s * a.v))


def gpow(a, e):
    """pow(a, e) with a real exponent: the device's dual takes pw = pow(a.v, e − 1), value pw·a.v, slope e·pw"""
    if not isinstance(a, Num):
        return np.power(a, e)
    pw = np.power(a.v, e - 1.0)
    value = pw * a.v if a.d else np.power(a.v, e)   # (without partials the device calls pow(x, e) itself)
    return _chain(a, value, e * pw, np.abs(e * (e - 1.0)) * np.power(a.v, e - 2.0))


# ------------------------------------------------------------------------------------------------ meshes
class Mesh:
    """conn[ne, npe] over nn nodes, coordinates X[dim, nn], the nodes a mask fixes (`boundary`), and the node graph G"""

    def __init__(self, name, nn, conn, X, boundary):
        self.name, self.nn = name, int(nn)
        self.conn = np.asarray(conn, dtype=np.int64)
        self.ne, self.npe = self.conn.shape
        self.X = np.asarray(X, dtype=np.float64)
        self.boundary = np.asarray(sorted(set(int(i) for i in boundary)), dtype=np.int64)
        pairs = [(int(i), int(j)) for el in self.conn for i in el for j in el if i != j]
        self.G = GC.Graph(name, self.nn, pairs)
        eo = self.G.edge_of()
        G = self.G
        # the global slot of every (element, a, b): row node conn[e, a], column node conn[e, b]
        self.slot = np.zeros((self.ne, self.npe, self.npe), dtype=np.int64)
        for e, el in enumerate(self.conn):
            for a, i in enumerate(el):
                for b, j in enumerate(el):
                    if i == j:
                        s = G.spos[i]
                    else:
                        pos = eo[(int(i), int(j))] - G.rowptr[i]
                        s = pos + (pos >= G.spos[i])
                    self.slot[e, a, b] = G.rowptr[i] + i + s

    def conn32(self):
        return np.ascontiguousarray(self.conn, dtype=np.int32)


def renumbered(M, seed):
    """nodes and elements randomly renumbered, every element's local order cyclically rotated"""
    rng = np.random.default_rng(9000 + seed + M.nn)
    pn, pe = rng.permutation(M.nn), rng.permutation(M.ne)
    conn = np.empty_like(M.conn)
    for e in range(M.ne):
        conn[pe[e]] = np.roll(pn[M.conn[e]], int(rng.integers(M.npe)))
    X = np.empty_like(M.X)
    X[:, pn] = M.X
    return Mesh(M.name + "p", M.nn, conn, X, pn[M.boundary])


def one_triangle():
    return Mesh("tri1", 3, [[0, 1, 2]], [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [0])


def two_triangles():
    return Mesh("tri2", 4, [[0, 1, 2], [1, 3, 2]], [[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.25]], [0, 3])


def rectangle(nx, ny, seed, extra_centre=False):
    """an nx × ny-node rectangle, every cell cut by a random diagonal (counter-clockwise triangles); extra_centre: the last
    cell gets a node at its centre and four triangles instead, which makes nn = nx·ny + 1"""
    rng = np.random.default_rng(8000 + 100 * seed + 3 * nx + ny)
    at = lambda i, j: j * nx + i   # noqa: E731
    conn = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            flip = bool(rng.integers(2))
            if extra_centre and i == nx - 2 and j == ny - 2:
                m = nx * ny
                conn += [[a, b, m], [b, c, m], [c, d, m], [d, a, m]]
            else:
                conn += [[a, b, d], [b, c, d]] if flip else [[a, b, c], [a, c, d]]
    nn = nx * ny + (1 if extra_centre else 0)
    xs, ys = np.meshgrid(np.arange(nx) / (nx - 1.0), 0.8 * np.arange(ny) / (ny - 1.0))
    X = np.stack([xs.ravel() + 0.1 * ys.ravel(), ys.ravel()])
    if extra_centre:
        X = np.concatenate([X, 0.25 * X[:, [at(nx - 2, ny - 2), at(nx - 1, ny - 2), at(nx - 1, ny - 1), at(nx - 2, ny - 1)]].sum(axis=1, keepdims=True)], axis=1)
    bd = [at(i, j) for j in range(ny) for i in range(nx) if i in (0, nx - 1) or j in (0, ny - 1)]
    return Mesh(f"tri{nn}", nn, conn, X, bd)


def fan(n, hub):
    """a closed fan: node `hub` in n triangles, the n rim nodes on a circle; every second rim node is fixed by a mask"""
    rim = [i for i in range(n + 1) if i != hub]
    conn = [[hub, rim[k], rim[(k + 1) % n]] for k in range(n)]
    X = np.zeros((2, n + 1))
    ang = 2 * np.pi * np.arange(n) / n
    X[0, rim], X[1, rim] = np.cos(ang), np.sin(ang)
    return Mesh(f"fan{n}", n + 1, conn, X, rim[::2])


def strip_with_orphans():
    """a 6 × 2-node strip of 10 triangles; nodes 5 and 13 (the last) are in no element. The mask fixes both ends and node 13"""
    ids = [i for i in range(13) if i != 5]   # 12 mesh nodes
    at = lambda i, j: ids[j * 6 + i]   # noqa: E731
    conn = []
    for i in range(5):
        conn += [[at(i, 0), at(i + 1, 0), at(i + 1, 1)], [at(i, 0), at(i + 1, 1), at(i, 1)]]
    X = np.zeros((2, 14))
    for j in range(2):
        for i in range(6):
            X[:, at(i, j)] = (0.2 * i, 0.3 * j + 0.02 * i)
    X[:, 5], X[:, 13] = (2.0, 2.0), (3.0, 3.0)
    return Mesh("strip", 14, conn, X, [at(0, 0), at(0, 1), at(5, 0), at(5, 1), 13])


def quads(cx, cy):
    """cx × cy quadrilaterals, counter-clockwise, slightly sheared"""
    nx, ny = cx + 1, cy + 1
    at = lambda i, j: j * nx + i   # noqa: E731
    conn = [[at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)] for j in range(cy) for i in range(cx)]
    xs, ys = np.meshgrid(np.arange(nx) / float(cx), 0.7 * np.arange(ny) / float(cy))
    X = np.stack([xs.ravel() + 0.15 * ys.ravel(), ys.ravel() + 0.05 * xs.ravel() ** 2])
    bd = [at(i, j) for j in range(ny) for i in range(nx) if i in (0, cx) or j in (0, cy)]
    return Mesh(f"quad{cx}x{cy}", nx * ny, conn, X, bd)


def _box_nodes(cx, cy, cz):
    nx, ny, nz = cx + 1, cy + 1, cz + 1
    at = lambda i, j, k: (k * ny + j) * nx + i   # noqa: E731
    zs, ys, xs = np.meshgrid(np.arange(nz) / float(cz), np.arange(ny) / float(cy), np.arange(nx) / float(cx), indexing="ij")
    X = np.stack([xs.ravel() + 0.1 * zs.ravel(), 0.9 * ys.ravel(), 0.8 * zs.ravel() + 0.05 * xs.ravel()])
    return nx * ny * nz, at, X


def tets(cx, cy, cz):
    """cx × cy × cz cubes cut into six tetrahedra each (Kuhn); the mask fixes the faces x = lo and x = hi"""
    import itertools
    nn, at, X = _box_nodes(cx, cy, cz)
    conn = []
    for k in range(cz):
        for j in range(cy):
            for i in range(cx):
                for perm in itertools.permutations(range(3)):
                    v = [i, j, k]
                    el = [at(*v)]
                    for ax in perm:
                        v[ax] += 1
                        el.append(at(*v))
                    conn.append(el)
    bd = [at(i, j, k) for k in range(cz + 1) for j in range(cy + 1) for i in (0, cx)]
    return Mesh(f"tet{cx}x{cy}x{cz}", nn, conn, X, bd)


def hexes(cx, cy, cz):
    nn, at, X = _box_nodes(cx, cy, cz)
    conn = [[at(i, j, k), at(i + 1, j, k), at(i + 1, j + 1, k), at(i, j + 1, k),
             at(i, j, k + 1), at(i + 1, j, k + 1), at(i + 1, j + 1, k + 1), at(i, j + 1, k + 1)]
            for k in range(cz) for j in range(cy) for i in range(cx)]
    bd = [at(i, j, k) for k in range(cz + 1) for j in range(cy + 1) for i in (0, cx)]
    return Mesh(f"hex{cx}x{cy}x{cz}", nn, conn, X, bd)


def truss():
    """a planar truss of 15 bars on 9 nodes with node degrees 6, 2, 4, 5, 4, 2, 1, 3, 3; supports: nodes 1, 5, 6"""
    bars = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (2, 3), (3, 4), (4, 5), (2, 7), (3, 7), (3, 8), (4, 8), (7, 8)]
    ang = np.pi / 3 * np.arange(6)
    X = np.zeros((2, 9))
    X[0, 1:7], X[1, 1:7] = 4 * np.cos(ang), 4 * np.sin(ang)
    X[:, 7], X[:, 8] = (0.0, 7.2), (-6.6, 3.8)
    return Mesh("truss", 9, bars, X, [1, 5, 6])


def pattern(M, dof):
    return GC.pattern(M.G, dof)


# ------------------------------------------------------------------------------------------------ the two views
class Cell:
    def __init__(self, e, ne, nn):
        self.e, self.ne, self.nn = e, ne, nn


class VecElem:
    """all instances at once. An instance is an element (seeds "none" and "v") or a (local node b, element) pair ("unit")"""

    def __init__(self, M, U, V, A, W, T, e, hot, seeds, defect=None):
        self.M, self.U, self.V, self.A, self.W, self.T, self.e, self.hot, self.seeds, self.defect = M, U, V, A, W, T, e, hot, seeds, defect
        self.npe, self.dof = M.npe, U.shape[0]
        self.ch = {"none": 0, "v": 1, "unit": self.dof}[seeds]

    def cell(self):
        return Cell(self.e, self.M.ne, self.M.nn)

    def node(self, a):
        return self.M.conn[self.e, a]

    def at(self, a, c=0):
        T, j = self.T, self.node(a)
        x = self.U[c][j]
        if self.seeds == "none":
            d = []
        elif self.seeds == "v":
            d = [self.V[c][j]]
        else:
            d = [np.where((self.hot == a) & (t == c), T(1), T(0)).astype(T) for t in range(self.dof)]
        return Num(x, d, np.abs(x), [np.abs(y) for y in d], leaf=True)

    def x(self, a, k=0):
        return self.A[k][self.node(a)]

    def w(self, k=0):
        if self.defect == "datum_by_node":
            return self.W[k][self.node(0) % self.M.ne]
        return self.W[k][self.e]

    def real(self, x):
        return np.asarray(x).astype(self.T)

    def zero(self):
        z = np.zeros(self.e.size, dtype=self.T)
        return Num(z, [z for _ in range(self.ch)], z, [z for _ in range(self.ch)])


class ScalarElem:
    """one element, NumPy float64 scalars"""

    def __init__(self, M, U, A, W, e):
        self.M, self.U, self.A, self.W, self.e = M, U, A, W, e
        self.npe, self.dof = M.npe, U.shape[0]
        self.nodes = [int(j) for j in M.conn[e]]

    def cell(self):
        return Cell(self.e, self.M.ne, self.M.nn)

    def node(self, a):
        return self.nodes[a]

    def at(self, a, c=0):
        return self.U[c][self.nodes[a]]

    def x(self, a, k=0):
        return self.A[k][self.nodes[a]]

    def w(self, k=0):
        return self.W[k][self.e]

    def real(self, x):
        return np.float64(x)

    def zero(self):
        return np.float64(0.0)


# ------------------------------------------------------------------------------------------------ the cases
class Problem:
    """a HIP source and the same formula in NumPy. node_spec / elem_spec: per datum "x", "y", "z" (a coordinate), (lo, hi) (a
    seeded range) or ("int", lo, hi) (seeded integers)"""

    def __init__(self, name, source, npe, dof, params, elem, node_spec=(), elem_spec=()):
        self.name, self.source, self.npe, self.dof, self.params, self.elem = name, source, npe, dof, list(params), elem
        self.node_spec, self.elem_spec = list(node_spec), list(elem_spec)
        self.nnode, self.nelem = len(self.node_spec), len(self.elem_spec)


def _seeded(rng, spec, n, X):
    if isinstance(spec, str):
        return X["xyz".index(spec)].copy()
    if spec[0] == "int":
        return rng.integers(spec[1], spec[2] + 1, n).astype(np.float64)
    return rng.uniform(spec[0], spec[1], n)


def data(prob, M, seed=1):
    """(A [nnode, nn], W [nelem, ne]) float64: coordinates and seeded data"""
    rng = np.random.default_rng(5000 + 10 * seed + len(prob.name) + M.nn)
    A = np.zeros((prob.nnode, M.nn))
    for k, spec in enumerate(prob.node_spec):
        A[k] = _seeded(rng, spec, M.nn, M.X)
    W = np.zeros((prob.nelem, M.ne))
    for k, spec in enumerate(prob.elem_spec):
        W[k] = _seeded(rng, spec, M.ne, None)
    return A, W


def inputs(prob, M, seed=0):
    """seeded u and v in [−1, 1], float64, length dof·nn"""
    rng = np.random.default_rng(1000 * seed + 13 * M.nn + M.ne + len(prob.name))
    n = prob.dof * M.nn
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


def fixed(prob, M, seed=3):
    """(mask int32, values) of dof·nn entries: component c is fixed on every (c + 1)-th node of the mesh's boundary list starting
    at its c-th (dof 1: the whole list), at seeded nonzero values"""
    rng = np.random.default_rng(300 + seed + M.nn + prob.dof)
    mask = np.zeros((prob.dof, M.nn), dtype=np.int32)
    for c in range(prob.dof):
        mask[c, M.boundary[c::c + 1]] = 1
    g = np.where(mask != 0, rng.uniform(0.25, 0.75, mask.shape) * rng.choice([-1.0, 1.0], mask.shape), 0.0)
    return mask.ravel(), g.ravel()


class _Plan:
    """a gather: contribution q goes to target[q]; within a target the contributions are added in their given order (the
    caller lists them element after element), starting from 0"""

    def __init__(self, target, n, drop_last=False):
        self.n = n
        self.order = np.argsort(target, kind="stable")
        tg = target[self.order]
        rank = np.arange(tg.size) - np.searchsorted(tg, tg, side="left")
        if drop_last:
            keep = rank + 1 < np.bincount(tg, minlength=n)[tg]
            self.order, tg, rank = self.order[keep], tg[keep], rank[keep]
        self.rounds = [(tg[rank == r], np.flatnonzero(rank == r)) for r in range(int(rank.max()) + 1 if rank.size else 0)]

    def __call__(self, vals, T):
        vv = vals[self.order]
        out = np.zeros(self.n, dtype=T)
        for tg, idx in self.rounds:
            out[tg] = out[tg] + vv[idx]
        return out


class Evaluation:
    """one problem at one (u, v, data, p, mask) in one arithmetic: f, Jv, CSR values, Jᵀv, fill·v and the Σ|terms| of each"""


def _run(prob, view, p, T):
    out = prob.elem(view, p, view.cell())
    assert len(out) == prob.npe * prob.dof
    return [o if isinstance(o, Num) else Num.const(T(0) + o, view.zero()) for o in out]


def evaluate(prob, M, u, v, A, W, *, T=np.float64, params=None, mask=None, values=None, defect=None):
    p = [T(x) for x in (prob.params if params is None else params)]
    dof, npe, nn, ne, G = prob.dof, M.npe, M.nn, M.ne, M.G
    S = G.ne + G.nn
    U, V = np.asarray(u, dtype=T).reshape(dof, nn), np.asarray(v, dtype=T).reshape(dof, nn)
    At, Wt = np.asarray(A, dtype=T), np.asarray(W, dtype=T)
    fx = np.zeros(dof * nn, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    gv = np.zeros(dof * nn, dtype=T) if values is None else np.asarray(values, dtype=T).ravel()
    uu, vv = np.asarray(u, dtype=T), np.asarray(v, dtype=T)
    drop = defect == "dropped_last_element"
    rows = _Plan(M.conn.ravel(), nn, drop)              # contributions (e, a), element-major
    entries = _Plan(M.slot.ravel(), S, drop)            # contributions (e, a, b), element-major
    els = np.arange(ne)
    E = Evaluation()

    def rows_of(out, pick):
        x, m = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
        for c in range(dof):
            x[c * nn:(c + 1) * nn] = rows(np.stack([pick(out[a * dof + c])[0] for a in range(npe)], axis=1).ravel(), T)
            m[c * nn:(c + 1) * nn] = rows(np.stack([pick(out[a * dof + c])[1] for a in range(npe)], axis=1).ravel(), T)
        return x, m

    out = _run(prob, VecElem(M, U, V, At, Wt, T, els, None, "none", defect), p, T)
    E.f, E.f_mag = rows_of(out, lambda o: (o.v, o.m))
    if defect != "fixed_row_left_as_sum":
        E.f[fx], E.f_mag[fx] = (uu - gv)[fx], (np.abs(uu) + np.abs(gv))[fx]
    out = _run(prob, VecElem(M, U, V, At, Wt, T, els, None, "v", defect), p, T)
    E.jv, E.jv_mag = rows_of(out, lambda o: (o.d[0], o.dm[0]))
    E.jv[fx], E.jv_mag[fx] = vv[fx], np.abs(vv)[fx]
    # the element matrices: one instance per (local node b, element), unit seeds on the dof unknowns of local node b
    out = _run(prob, VecElem(M, U, V, At, Wt, T, np.tile(els, npe), np.repeat(np.arange(npe), ne), "unit", defect), p, T)
    vals, mags = np.zeros(dof * dof * S, dtype=T), np.zeros(dof * dof * S, dtype=T)
    i, s = G.slot_node, G.slot_s
    for c in range(dof):
        for c2 in range(dof):
            at = c * dof * S + dof * (G.rowptr[i] + i) + c2 * (G.deg[i] + 1) + s
            cc, cc2 = (c2, c) if defect == "transposed_block" else (c, c2)
            # X[e, a, b] = dF_{a,cc}/du_{b,cc2} of element e
            X = np.stack([out[a * dof + cc].d[cc2].reshape(npe, ne).T for a in range(npe)], axis=1)
            Xm = np.stack([out[a * dof + cc].dm[cc2].reshape(npe, ne).T for a in range(npe)], axis=1)
            if defect == "ab_transposed":
                X, Xm = X.transpose(0, 2, 1), Xm.transpose(0, 2, 1)
            vals[at], mags[at] = entries(X.ravel(), T), entries(Xm.ravel(), T)
            frow = fx[c * nn + i]
            unit = np.where((c2 == c) & (s == G.spos[i]), T(1), T(0)).astype(T)
            if defect == "fixed_offdiagonal_kept":
                sel = frow & (c2 == c) & (s == G.spos[i])
            else:
                sel = frow
            vals[at[sel]], mags[at[sel]] = unit[sel], 0
    E.vals, E.vals_mag = vals, mags
    rp, ci = pattern(M, dof)
    rws = np.repeat(np.arange(dof * nn), np.diff(rp))
    E.jtv, E.jtv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.jtv, ci, vals * vv[rws])
    np.add.at(E.jtv_mag, ci, mags * np.abs(vv[rws]) + np.where(mags == 0, np.abs(vals * vv[rws]), 0))
    E.spmv, E.spmv_mag = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
    np.add.at(E.spmv, rws, vals * vv[ci])
    np.add.at(E.spmv_mag, rws, mags * np.abs(vv[ci]) + np.where(mags == 0, np.abs(vals * vv[ci]), 0))
    return E


def scalar_residual(prob, M, u, A, W, params=None, mask=None, values=None):
    """the residual element by element through ScalarElem (float64), accumulated in element order; then the fixed rows"""
    p = [np.float64(x) for x in (prob.params if params is None else params)]
    U = np.asarray(u, dtype=np.float64).reshape(prob.dof, M.nn)
    f = np.zeros((prob.dof, M.nn))
    for e in range(M.ne):
        view = ScalarElem(M, U, np.asarray(A, dtype=np.float64), np.asarray(W, dtype=np.float64), e)
        out = prob.elem(view, p, view.cell())
        for a in range(M.npe):
            for c in range(prob.dof):
                f[c, view.node(a)] += out[a * prob.dof + c]
    f = f.ravel()
    if mask is not None:
        for r in np.flatnonzero(np.asarray(mask).ravel()):
            f[r] = u[r] - (0.0 if values is None else values[r])
    return f


class Reference:
    """float64 restatement, per-entry gap to long double and the bound MARGIN·gap + FLOOR_ULPS eps·Σ|terms| for f, jv, vals,
    jtv, spmv (grid_core's rule and constants)"""

    def __init__(self, prob, M, u, v, A, W, *, params=None, mask=None, values=None):
        a = evaluate(prob, M, u, v, A, W, T=np.float64, params=params, mask=mask, values=values)
        b = evaluate(prob, M, u, v, A, W, T=LD, params=params, mask=mask, values=values)
        for k in ("f", "jv", "vals", "jtv", "spmv"):
            x64, x80 = getattr(a, k), getattr(b, k)
            gap = np.abs(x64.astype(LD) - x80).astype(np.float64)
            setattr(self, k, x64)
            setattr(self, k + "_gap", gap)
            setattr(self, k + "_bound", MARGIN * gap + FLOOR_ULPS * EPS * getattr(a, k + "_mag"))


_CACHE = {}


def reference(prob, M, masked=False, seed=0, params=None, data_seed=1, fixed_seed=3):
    """the shared reference of a case (computed once, not modified by its users): seeded u, v, data and, if masked, fixed()"""
    key = (prob.name, M.name, masked, seed, None if params is None else tuple(params), data_seed, fixed_seed)
    if key not in _CACHE:
        u, v = inputs(prob, M, seed)
        A, W = data(prob, M, data_seed)
        mask, values = fixed(prob, M, fixed_seed) if masked else (None, None)
        R = Reference(prob, M, u, v, A, W, params=params, mask=mask, values=values)
        R.u, R.v, R.A, R.W, R.mask, R.values = u, v, A, W, mask, values
        for arr in vars(R).values():
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = R
    return _CACHE[key]


def dense_jacobian(prob, M, u, A, W, *, params=None, mask=None, values=None):
    """the float64 restatement's Jacobian as a dense matrix and its residual (small meshes: the reference Newton)"""
    E = evaluate(prob, M, u, np.zeros_like(u), A, W, params=params, mask=mask, values=values)
    rp, ci = pattern(M, prob.dof)
    n = rp.size - 1
    J = np.zeros((n, n))
    J[np.repeat(np.arange(n), np.diff(rp)), ci] = E.vals
    return J, E.f


def dense_newton(prob, M, u0, A, W, *, params=None, mask=None, values=None, tol=1e-13, maxiters=50):
    """plain Newton with dense solves on the restatement: (u, steps taken)"""
    u = np.array(u0, dtype=np.float64)
    for it in range(maxiters):
        J, f = dense_jacobian(prob, M, u, A, W, params=params, mask=mask, values=values)
        if np.max(np.abs(f)) <= tol:
            return u, it
        u = u - np.linalg.solve(J, f)
    return u, maxiters
