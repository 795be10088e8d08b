"""The NumPy restatement of compiled element problems made of several element blocks (csrc/nk_elem.hip, "Blocks"), on top of
tests/elem_core.py: its Mesh-like views, VecElem, ScalarElem, _Plan, Num and the bound rule are used, not restated.

A BlockMesh is nn nodes and a list of blocks, each a connectivity conn_k[ne_k, npe_k] (npe_k = 1 is a point element). It has
ONE union graph — two nodes are adjacent when they share an element of any block — and per block the global slot of every
(element, a, b). A BlockProblem is one elem_core.Problem per block (its source, its formula, its element data) with shared
dof, parameters and node data. The formula of block k sees u.block = k (the device's NK_BLOCK), s.e and s.ne counting within
the block, and u.w(k) its block's own data.

The evaluation computes every block's contributions as elem_core does and places them one block after the other in a buffer;
the gather adds a row's (an entry's) contributions in the order block 0's elements ascending, then block 1's, …, starting from
0, and carries Σ|terms| through: the running sum continues from block to block. Fixed rows, Jᵀv, fill·v and the bound

    |device − float64 restatement| <= MARGIN × |float64 − long double| + FLOOR_ULPS eps × Σ|terms|

are elem_core's. `defect=` plants one of DEFECTS, for the tests that show the assertions reject it."""
import numpy as np

import elem_core as EC
import graph_core as GC
from elem_core import EPS, FLOOR_ULPS, LD, MARGIN  # noqa: F401

DEFECTS = ("blocks_reversed", "base_dropped", "datum_stride_of_block0", "pairs_missing", "block_off_by_one")


# ------------------------------------------------------------------------------------------------ meshes
class _Block:
    """what elem_core's views ask of a mesh, for one block"""

    def __init__(self, nn, conn):
        self.nn = int(nn)
        self.conn = np.asarray(conn, dtype=np.int64)
        self.ne, self.npe = self.conn.shape

    def conn32(self):
        return np.ascontiguousarray(self.conn, dtype=np.int32)


def union_pairs(conns, defect=None):
    """the directed node pairs of all blocks (pairs_missing: the last block's are left out)"""
    use = conns[:-1] if defect == "pairs_missing" else conns
    return [(int(i), int(j)) for conn in use for el in np.asarray(conn) for i in el for j in el if i != j]


class BlockMesh:
    """blocks conn_k[ne_k, npe_k] over nn nodes, coordinates X[dim, nn], the nodes a mask fixes, the union graph G and the
    global slot of every (element, a, b) of every block"""

    def __init__(self, name, nn, conns, X, boundary):
        self.name, self.nn = name, int(nn)
        self.blocks = [_Block(nn, c) for c in conns]
        self.X = np.asarray(X, dtype=np.float64)
        self.boundary = np.asarray(sorted(set(int(i) for i in boundary)), dtype=np.int64)
        self.G = G = GC.Graph(name, self.nn, union_pairs([b.conn for b in self.blocks]))
        eo = G.edge_of()
        for B in self.blocks:
            B.slot = np.zeros((B.ne, B.npe, B.npe), dtype=np.int64)
            for e, el in enumerate(B.conn):
                for a, i in enumerate(el):
                    for b, j in enumerate(el):
                        if i == j:
                            s = G.spos[i]
                        else:
                            pos = eo[(int(i), int(j))] - G.rowptr[i]
                            s = pos + (pos >= G.spos[i])
                        B.slot[e, a, b] = G.rowptr[i] + i + s

    @property
    def nblocks(self):
        return len(self.blocks)

    def conns32(self):
        return [B.conn32() for B in self.blocks]


def pattern(M, dof):
    return GC.pattern(M.G, dof)


# ------------------------------------------------------------------------------------------------ the two views
class BlockVecElem(EC.VecElem):
    def __init__(self, k, ne0, *args):
        super().__init__(*args)
        self.block = k + 1 if self.defect == "block_off_by_one" else k
        self._ne0 = ne0

    def w(self, k=0):
        if self.defect == "datum_stride_of_block0":   # datum k read at k·ne_0 + e of the block's buffer
            flat = self.W.ravel()
            return flat[(k * self._ne0 + self.e) % flat.size]
        return self.W[k][self.e]


class BlockScalarElem(EC.ScalarElem):
    def __init__(self, k, *args):
        super().__init__(*args)
        self.block = k


# ------------------------------------------------------------------------------------------------ the cases
class BlockProblem:
    """one elem_core.Problem per block; dof, params and the node data (node_spec) are shared"""

    def __init__(self, name, parts, params, node_spec=()):
        self.name, self.parts, self.params, self.node_spec = name, list(parts), list(params), list(node_spec)
        self.dof, self.nnode = self.parts[0].dof, len(self.node_spec)
        assert all(p.dof == self.dof for p in self.parts)


def data(prob, M, seed=1):
    """(A [nnode, nn], [W_k [nelem_k, ne_k]]) float64: coordinates and seeded data"""
    rng = np.random.default_rng(6000 + 10 * seed + len(prob.name) + M.nn)
    A = np.zeros((prob.nnode, M.nn))
    for k, spec in enumerate(prob.node_spec):
        A[k] = EC._seeded(rng, spec, M.nn, M.X)
    Ws = []
    for part, B in zip(prob.parts, M.blocks):
        W = np.zeros((part.nelem, B.ne))
        for k, spec in enumerate(part.elem_spec):
            W[k] = EC._seeded(rng, spec, B.ne, None)
        Ws.append(W)
    return A, Ws


def inputs(prob, M, seed=0):
    rng = np.random.default_rng(1000 * seed + 13 * M.nn + sum(B.ne for B in M.blocks) + len(prob.name))
    n = prob.dof * M.nn
    return rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)


def fixed(prob, M, seed=3):
    """elem_core.fixed on the mesh's boundary list"""
    return EC.fixed(prob, M, seed)


def evaluate(prob, M, u, v, A, Ws, *, T=np.float64, params=None, mask=None, values=None, defect=None):
    p = [T(x) for x in (prob.params if params is None else params)]
    dof, nn, G = prob.dof, M.nn, M.G
    S = G.ne + G.nn
    U, V = np.asarray(u, dtype=T).reshape(dof, nn), np.asarray(v, dtype=T).reshape(dof, nn)
    At = np.asarray(A, dtype=T)
    fx = np.zeros(dof * nn, dtype=bool) if mask is None else np.asarray(mask).ravel() != 0
    gv = np.zeros(dof * nn, dtype=T) if values is None else np.asarray(values, dtype=T).ravel()
    uu, vv = np.asarray(u, dtype=T), np.asarray(v, dtype=T)
    order = list(range(M.nblocks))
    if defect == "blocks_reversed":
        order = order[::-1]
    # the buffers hold block after block; a list is the positions of a row's (an entry's) contributions in summation order
    sizes = [B.ne * B.npe for B in M.blocks]
    msizes = [B.ne * B.npe * B.npe for B in M.blocks]
    base = np.concatenate([[0], np.cumsum(sizes)])
    mbase = np.concatenate([[0], np.cumsum(msizes)])
    rows = EC._Plan(np.concatenate([M.blocks[k].conn.ravel() for k in order]), nn)
    entries = EC._Plan(np.concatenate([M.blocks[k].slot.ravel() for k in order]), S)
    pick_rows = np.concatenate([base[k] + np.arange(sizes[k]) for k in order])
    pick_entries = np.concatenate([mbase[k] + np.arange(msizes[k]) for k in order])

    def buffer(parts, starts, total):
        buf = np.zeros(total, dtype=T)
        for k, x in enumerate(parts):
            at = 0 if (defect == "base_dropped" and k > 0) else starts[k]
            buf[at:at + x.size] = x
        return buf

    def run(seeds):
        outs = []
        for k, (part, B) in enumerate(zip(prob.parts, M.blocks)):
            els = np.arange(B.ne)
            e, hot = (np.tile(els, B.npe), np.repeat(np.arange(B.npe), B.ne)) if seeds == "unit" else (els, None)
            view = BlockVecElem(k, M.blocks[0].ne, B, U, V, At, np.asarray(Ws[k], dtype=T), T, e, hot, seeds, defect)
            outs.append(EC._run(part, view, p, T))
        return outs

    E = EC.Evaluation()

    def rows_of(outs, pick):
        x, m = np.zeros(dof * nn, dtype=T), np.zeros(dof * nn, dtype=T)
        for c in range(dof):
            for j, dst in ((0, x), (1, m)):
                parts = [np.stack([pick(out[a * dof + c])[j] for a in range(B.npe)], axis=1).ravel() for out, B in zip(outs, M.blocks)]
                dst[c * nn:(c + 1) * nn] = rows(buffer(parts, base, base[-1])[pick_rows], T)
        return x, m

    E.f, E.f_mag = rows_of(run("none"), lambda o: (o.v, o.m))
    E.f[fx], E.f_mag[fx] = (uu - gv)[fx], (np.abs(uu) + np.abs(gv))[fx]
    E.jv, E.jv_mag = rows_of(run("v"), lambda o: (o.d[0], o.dm[0]))
    E.jv[fx], E.jv_mag[fx] = vv[fx], np.abs(vv)[fx]
    outs = run("unit")
    vals, mags = np.zeros(dof * dof * S, dtype=T), np.zeros(dof * dof * S, dtype=T)
    i, s = G.slot_node, G.slot_s
    for c in range(dof):
        for c2 in range(dof):
            at = c * dof * S + dof * (G.rowptr[i] + i) + c2 * (G.deg[i] + 1) + s
            for j, dst in ((0, vals), (1, mags)):
                # X[e, a, b] = dF_{a,c}/du_{b,c2} of element e of the block
                parts = [np.stack([(out[a * dof + c].d[c2] if j == 0 else out[a * dof + c].dm[c2]).reshape(B.npe, B.ne).T
                                   for a in range(B.npe)], axis=1).ravel() for out, B in zip(outs, M.blocks)]
                dst[at] = entries(buffer(parts, mbase, mbase[-1])[pick_entries], T)
            frow = fx[c * nn + i]
            unit = np.where((c2 == c) & (s == G.spos[i]), T(1), T(0)).astype(T)
            vals[at[frow]], mags[at[frow]] = unit[frow], 0
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


def scalar_residual(prob, M, u, A, Ws, params=None, mask=None, values=None):
    """the residual element by element (float64 scalars), block after block, accumulated in that order; then the fixed rows"""
    p = [np.float64(x) for x in (prob.params if params is None else params)]
    U = np.asarray(u, dtype=np.float64).reshape(prob.dof, M.nn)
    f = np.zeros((prob.dof, M.nn))
    for k, (part, B) in enumerate(zip(prob.parts, M.blocks)):
        for e in range(B.ne):
            view = BlockScalarElem(k, B, U, np.asarray(A, dtype=np.float64), np.asarray(Ws[k], dtype=np.float64), e)
            out = part.elem(view, p, view.cell())
            for a in range(B.npe):
                for c in range(prob.dof):
                    f[c, view.node(a)] += out[a * prob.dof + c]
    f = f.ravel()
    if mask is not None:
        for r in np.flatnonzero(np.asarray(mask).ravel()):
            f[r] = u[r] - (0.0 if values is None else values[r])
    return f


class Reference:
    """float64 restatement, per-entry gap to long double and the bound for f, jv, vals, jtv, spmv (elem_core.Reference's rule)"""

    def __init__(self, prob, M, u, v, A, Ws, *, params=None, mask=None, values=None):
        a = evaluate(prob, M, u, v, A, Ws, T=np.float64, params=params, mask=mask, values=values)
        b = evaluate(prob, M, u, v, A, Ws, T=LD, params=params, mask=mask, values=values)
        for k in ("f", "jv", "vals", "jtv", "spmv"):
            x64, x80 = getattr(a, k), getattr(b, k)
            gap = np.abs(x64.astype(LD) - x80).astype(np.float64)
            setattr(self, k, x64)
            setattr(self, k + "_gap", gap)
            setattr(self, k + "_bound", MARGIN * gap + FLOOR_ULPS * EPS * getattr(a, k + "_mag"))


_CACHE = {}


def reference(prob, M, masked=False, seed=0, params=None, data_seed=1):
    """the shared reference of a case (computed once, not modified by its users)"""
    key = (prob.name, M.name, masked, seed, None if params is None else tuple(params), data_seed)
    if key not in _CACHE:
        u, v = inputs(prob, M, seed)
        A, Ws = data(prob, M, data_seed)
        mask, values = fixed(prob, M) if masked else (None, None)
        R = Reference(prob, M, u, v, A, Ws, params=params, mask=mask, values=values)
        R.u, R.v, R.A, R.Ws, R.mask, R.values = u, v, A, Ws, mask, values
        for arr in list(vars(R).values()) + list(Ws):
            if isinstance(arr, np.ndarray):
                arr.setflags(write=False)
        _CACHE[key] = R
    return _CACHE[key]


def dense_jacobian(prob, M, u, A, Ws, *, params=None, mask=None, values=None):
    E = evaluate(prob, M, u, np.zeros_like(u), A, Ws, params=params, mask=mask, values=values)
    rp, ci = pattern(M, prob.dof)
    n = rp.size - 1
    J = np.zeros((n, n))
    J[np.repeat(np.arange(n), np.diff(rp)), ci] = E.vals
    return J, E.f


def dense_newton(prob, M, u0, A, Ws, *, params=None, mask=None, values=None, tol=1e-13, maxiters=50):
    """elem_core.dense_newton extended to blocks: (u, steps taken)"""
    u = np.array(u0, dtype=np.float64)
    for it in range(maxiters):
        J, f = dense_jacobian(prob, M, u, A, Ws, params=params, mask=mask, values=values)
        if np.max(np.abs(f)) <= tol:
            return u, it
        u = u - np.linalg.solve(J, f)
    return u, maxiters
