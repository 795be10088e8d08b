"""NumPy restatement of the compiled grid problems ON SEVERAL RANKS (csrc/nk_grid.hip, "several ranks: slabs of the outermost
axis"), built on the tables grid_reference, grid3_reference, grid_r2_reference and gridf_reference,
whose sources and formulas it takes as they are, and on grid_core's index maps, pattern and bound. Nothing is computed here that
they do not compute: a rank's residual, J·v, Jᵀv and fill values are the one-rank restatement's entries MOVED by a permutation.

    slabs        rank r of R owns the lines (3-D: planes) [n_outer·r // R, n_outer·(r + 1) // R) of the outermost axis
                 (nk_partition_range with granule 1), every slab at least radius + 1 of them
    local        component-major on the slab: c·nn_loc + slab node
    global       row_begin + local, row_begin = dof · (nodes of all lower slabs): slab after slab
    one-rank     c·nn + node

permutation(shape, dof, R)[g] is the one-rank index of the unknown with global index g. A rank's rows of the pattern are the
permuted one-rank pattern's rows with the columns renumbered to global and sorted ascending; `src` remembers where each entry
came from, so the expected fill values (and their bounds) are vals[src]. The bound is the project's, from grid_core:

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms|"""
import functools

import numpy as np

import grid3_reference as G3
import grid_r2_reference as G2
import grid_reference as G1
import gridf_reference as GF
from grid_core import RADIUS, pattern, reference
from gridbc_reference import DI, MF, MN, PE


def slab_ranges(n_outer, R):
    """[(l0, l1)] of every rank: nk_partition_range(n_outer, 1, R, r)"""
    return [(n_outer * r // R, n_outer * (r + 1) // R) for r in range(R)]


def thinnest(n_outer, R):
    return min(b - a for a, b in slab_ranges(n_outer, R))


def permutation(shape, dof, R):
    """perm[g] = c·nn + node of the unknown with the global (rank-contiguous) index g"""
    shape = tuple(shape)
    nn, line = int(np.prod(shape)), int(np.prod(shape[:-1]))
    return np.concatenate([c * nn + np.arange(a * line, b * line, dtype=np.int64)
                           for a, b in slab_ranges(shape[-1], R) for c in range(dof)])


class Slab:
    """rank r of R of a grid: its lines, its rows (their one-rank indices, in local order), its rows of the pattern with global
    columns, ascending, and for every entry the position of the same entry in the one-rank value array"""

    def __init__(self, shape, dof, offs, sides, R, r):
        shape = tuple(shape)
        self.shape, self.dof, self.R, self.r = shape, dof, R, r
        self.lines = slab_ranges(shape[-1], R)[r]
        line = int(np.prod(shape[:-1]))
        self.nn_loc = line * (self.lines[1] - self.lines[0])
        self.n_local, self.n_global = dof * self.nn_loc, dof * int(np.prod(shape))
        self.row_begin = dof * line * self.lines[0]
        perm = permutation(shape, dof, R)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        self.rows = perm[self.row_begin:self.row_begin + self.n_local]
        rp, ci = pattern(shape, dof, offs, sides)
        rp, ci = rp.astype(np.int64), ci.astype(np.int64)
        counts = rp[self.rows + 1] - rp[self.rows]
        self.rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        colind, src = [], []
        for one in self.rows:
            cols = inv[ci[rp[one]:rp[one + 1]]]
            order = np.argsort(cols, kind="stable")
            colind.append(cols[order])
            src.append(rp[one] + order)
        self.colind = np.concatenate(colind).astype(np.int64)
        self.src = np.concatenate(src).astype(np.int64)
        own = (self.colind >= self.row_begin) & (self.colind < self.row_begin + self.n_local)
        self.n_halo = int(np.unique(self.colind[~own]).size)   # distinct ghost unknowns the pattern names

    def local(self, full):
        """this rank's local vector of an array in one-rank order"""
        return np.asarray(full)[self.rows]

    def values(self, vals):
        """this rank's CSR values (or their bounds) of the one-rank value array"""
        return np.asarray(vals)[self.src]


def union_pattern(slabs):
    """the ranks' patterns mapped back through the permutation: (rowptr, colind) in one-rank numbering, columns ascending"""
    first = slabs[0]
    perm = permutation(first.shape, first.dof, first.R)
    rows = [None] * perm.size
    for S in slabs:
        for t, one in enumerate(S.rows):
            rows[one] = np.sort(perm[S.colind[S.rowptr[t]:S.rowptr[t + 1]]])
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    return rowptr.astype(np.int32), np.concatenate(rows).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the cases
# the five kinds of the split axis (2-D: y), Bratu's source, x Dirichlet-0
Y_KINDS = {"ydir": (DI, DI), "yper": (PE, PE), "ymnode": (MN, MN), "ymface": (MF, MF), "ymixed": (MF, DI)}
PROBLEMS = {p.name: p for p in [
    *[G1.PROBLEMS["bratu"].with_boundary("bratu_" + k, (DI, DI) + v) for k, v in Y_KINDS.items()],
    # the x axis periodic and mirrored: at the slab's first line the points (−1, −1) and (0, −1) of the box land on ONE ghost node
    G1.PROBLEMS["bratu"].with_boundary("bratu_xper_yper", (PE, PE, PE, PE)),
    G1.PROBLEMS["bratu"].with_boundary("bratu_xmface_ymixed", (MF, MF, MF, DI)),
    # star and box at dof 2; the Brusselator's source reads s.i, s.j, s.nx and s.ny
    G1.PROBLEMS["brusselator"].with_boundary("brus_site_yper", (MF, MF, PE, PE)),
    G1.PROBLEMS["brusselator"].with_boundary("brus_site_ydir", (PE, PE, DI, DI)),
    G1.PROBLEMS["box_dirichlet"].with_boundary("box_xmface_yper", (MF, MF, PE, PE)),
    G1.PROBLEMS["box_dirichlet"].with_boundary("box_xmnode_ymixed", (MN, MN, MF, DI)),
    # radius 2
    G2.PROBLEMS["upwind2_dirichlet"].with_boundary("star2_yper", (MN, MF, PE, PE)),
    G2.PROBLEMS["upwind2_dirichlet"].with_boundary("star2_ydir", (PE, PE, DI, DI)),
    G2.PROBLEMS["diamond_dirichlet"].with_boundary("diamond2_ymnode", (MF, MF, MN, MN)),
    G2.PROBLEMS["diamond_dirichlet"].with_boundary("diamond2_yper", (DI, DI, PE, PE)),
    # 3-D: the star at dof 2 (its source reads the site) and the radius-2 star
    G3.PROBLEMS["brusselator3"].with_boundary("star3_zper", (PE, PE, DI, MN, PE, PE)),
    G3.PROBLEMS["brusselator3"].with_boundary("star3_zmixed", (MF, MF, PE, PE, MF, DI)),
    G2.PROBLEMS["upwind3_dirichlet"].with_boundary("star2_3_zmnode", (PE, PE, DI, DI, MN, MN)),
    # fields: κ (field 1) is read at all four offsets, so across the cut
    GF.PROBLEMS["vardiff"].with_boundary("vardiff_yper", (DI, DI, PE, PE)),
    GF.PROBLEMS["vardiff"].with_boundary("vardiff_ymface", (MF, MF, MF, MF)),
]}
# sources without an elementary function: the same nk_point on the same inputs, bit for bit on any number of ranks
HAS_EXP = tuple(n for n, p in PROBLEMS.items() if "exp(" in p.source)


def small_shape(prob, R):
    """the smallest shape that still splits into R legal slabs: 4 × 5 (slabs 2|3) and 5 × 7 (3|4) for two ranks, 4 × 7 (2|2|3)
    and 5 × 9 for three, (radius + 1)·R lines for any R; 3-D: 4 × 3 and 5 × 5 nodes on the other axes"""
    rad = RADIUS[prob.stencil]
    n_outer = {1: 2 * rad + 1, 2: 2 * rad + 3, 3: 7 if rad == 1 else 9}.get(R, (rad + 1) * R)
    assert R == 1 or thinnest(n_outer, R) >= rad + 1
    inner = ((4, 3) if rad == 1 else (5, 5)) if prob.dim == 3 else ((4,) if rad == 1 else (5,))
    return inner + (n_outer,)


@functools.lru_cache(maxsize=None)
def slab(name, shape, R, r):
    prob = PROBLEMS[name]
    return Slab(shape, prob.dof, prob.offsets(), prob.sides, R, r)


def expected(name, shape, R, r, seed=0):
    """{quantity: (expected local array, its bound)} for f, jv, vals, jtv, spmv: the one-rank reference's entries, moved"""
    ref, S = reference(PROBLEMS[name], shape, seed), slab(name, shape, R, r)
    out = {k: (S.local(getattr(ref, k)), S.local(getattr(ref, k + "_bound"))) for k in ("f", "jv", "jtv", "spmv")}
    out["vals"] = (S.values(ref.vals), S.values(ref.vals_bound))
    return out
