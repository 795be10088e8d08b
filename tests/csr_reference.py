"""References and case list for the CSR layer (csrc/nk_csr.hip), shared by tests/test_csr_reference.py (no GPU: pins the
references, proves the case list reaches every path it is tagged for) and tests/test_gpu_csr.py (the device against them).

Two kinds of reference, and no measured tolerance anywhere:

  sequential   float64, every product rounded on its own (the library is built with -ffp-contract=off), summed in the order the
               kernel promises: CSR order inside a row for A x, ascending row inside a column for Aᵀ x, colsumsq and JᵀJ.
               Rows that `rowblocks` puts on the tile path must equal it BIT FOR BIT.
  long double  the same sum in np.longdouble next to |A||x|. A long row (more than `tile` non-zeros: one workgroup reduces it,
               256 strided partial sums, a butterfly, four wave sums) has another summation order, so it is held to the
               componentwise bound of ANY order of k separately rounded (or fused) products [Higham, Accuracy and Stability of
               Numerical Algorithms, §3.1]:   |ŝ − s| ≤ γ_k (|A||x|)_i,   γ_k = k u / (1 − k u),   u = 2⁻⁵³.

Epilogues (spmv_store_row) add one to four further roundings to ŝ. With δ = γ_k (|A||x|)_i the bound on ŝ and |fl(z) − z| ≤ u |z|
for each further operation, the error of a result z(s) is propagated as written out in `epilogue_bound`: an operation
z = a ∘ b whose operand a carries the error E_a has the error  E_z ≤ |∂z/∂a| E_a + u (|z| + |∂z/∂a| E_a)  (all operations here
are linear in the operand that carries the error)."""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
ROWCAP = 1024            # rows per block: 4 · NK_BLOCK (build_rowblocks)
TILES = (512, 1024, 2048, 4096)


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------ matrix
class Mat:
    """Square CSR matrix: rowptr (n + 1), col, val; the columns of a row ascend and are unique; stored zeros stay stored."""

    def __init__(self, n, rowptr, col, val):
        self.n = int(n)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int64)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        assert self.rowptr.size == self.n + 1 and self.rowptr[0] == 0 and self.rowptr[-1] == self.col.size == self.val.size
        assert self.col.size == 0 or (self.col.min() >= 0 and self.col.max() < self.n)

    @property
    def nnz(self):
        return int(self.col.size)

    @property
    def rowlen(self):
        return np.diff(self.rowptr)

    @property
    def rowof(self):
        return np.repeat(np.arange(self.n), self.rowlen)

    def with_values(self, val):
        return Mat(self.n, self.rowptr, self.col, val)

    def scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val, self.col, self.rowptr), shape=(self.n, self.n))

    def transpose(self):
        """(T, perm): Aᵀ in CSR with the entries of a column of A in ascending row order; T.val = A.val[perm]
        (build_transpose: a stable counting sort by column)."""
        perm = np.argsort(self.col, kind="stable")
        rp = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.n))])
        return Mat(self.n, rp, self.rowof[perm], self.val[perm]), perm

    def csc(self):
        """(colptr, rowval, perm) of the CSC form (0-based): nzval = val[perm]."""
        T, perm = self.transpose()
        return T.rowptr, T.col, perm


def from_rows(n, rows, rng, zeros=()):
    """rows: per row an array of columns (any order, duplicates dropped); values standard normal; `zeros`: positions (row, col)
    whose stored value is an exact zero."""
    rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in rows]
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    col = np.concatenate(rows) if rp[-1] else np.zeros(0, dtype=np.int64)
    val = rng.standard_normal(col.size)
    val[val == 0.0] = 1.0
    M = Mat(n, rp, col, val)
    for r, c in zeros:
        k = M.rowptr[r] + int(np.searchsorted(M.col[M.rowptr[r]:M.rowptr[r + 1]], c))
        assert M.col[k] == c
        M.val[k] = 0.0
    return M


# ---------------------------------------------------------------------------------------------------------------- row blocks
def rowblocks(rowptr, tile):
    """Block boundaries as build_rowblocks makes them: a block grows while it holds ≤ tile non-zeros and < 1024 rows; a row
    longer than a tile is a block of its own (the long-row path). Returns the array of first rows, closed by n."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = rowptr.size - 1
    rb = [0]
    r = 0
    while r < n:
        # the last e ≤ min(n, r + 1024) with rowptr[e] − rowptr[r] ≤ tile
        hi = min(n, r + ROWCAP)
        e = int(np.searchsorted(rowptr[r:hi + 1], rowptr[r] + tile, side="right")) - 1 + r
        if e == r:
            e = r + 1
        rb.append(e)
        r = e
    return np.asarray(rb, dtype=np.int64)


def long_rows(rowptr, tile):
    """Boolean per row: the row is reduced by a whole workgroup (more than `tile` non-zeros)."""
    return np.diff(np.asarray(rowptr, dtype=np.int64)) > tile


def block_offsets(M, tile):
    """(min, max) over all non-zeros of column − first row of the non-zero's block: what the 16-bit column path stores."""
    if M.nnz == 0:
        return 0, 0
    rb = rowblocks(M.rowptr, tile)
    first = np.repeat(rb[:-1], np.diff(rb))            # first row of every row's block
    d = M.col - first[M.rowof]
    return int(d.min()), int(d.max())


def fits16(M, tile):
    lo, hi = block_offsets(M, tile)
    return -32768 <= lo and hi <= 32767


# ---------------------------------------------------------------------------------------------------------------------- sums
def segsum(ptr, p, dtype=np.float64):
    """Per segment [ptr[i], ptr[i + 1]) the sum of p, accumulated front to back from 0 in `dtype` (one rounding per addition)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n = ptr.size - 1
    p = np.asarray(p, dtype=dtype)
    s = np.zeros(n, dtype=dtype)
    ln = np.diff(ptr)
    order = np.argsort(-ln, kind="stable")             # longest first: at step j the active segments are a prefix
    lsorted = ln[order]
    start = ptr[:-1][order]
    for j in range(int(lsorted[0]) if n else 0):
        m = int(np.searchsorted(-lsorted, -j, side="left"))      # segments with length > j
        idx = order[:m]
        s[idx] = s[idx] + p[start[:m] + j]
    return s


def spmv_sequential(A, x):
    """float64, products rounded separately, summed in CSR order from 0.0: what the tile path promises bit for bit."""
    with np.errstate(all="ignore"):
        return segsum(A.rowptr, A.val * np.asarray(x, dtype=np.float64)[A.col])


def spmv_longdouble(A, x):
    with np.errstate(all="ignore"):
        return segsum(A.rowptr, A.val.astype(LD) * np.asarray(x).astype(LD)[A.col], LD)


def abs_spmv(A, x):
    """|A||x| in long double."""
    return segsum(A.rowptr, np.abs(A.val).astype(LD) * np.abs(np.asarray(x)).astype(LD)[A.col], LD)


def spmv_t_sequential(A, x):
    return spmv_sequential(A.transpose()[0], x)


def spmv_t_longdouble(A, x):
    return spmv_longdouble(A.transpose()[0], x)


def abs_spmv_t(A, x):
    return abs_spmv(A.transpose()[0], x)


def squared(A):
    T = A.transpose()[0]
    return T.with_values(T.val * T.val)                # v·v rounded once; the product with the vector of ones is exact


def colsumsq_sequential(A):
    return spmv_sequential(squared(A), np.ones(A.n))


def colsumsq_longdouble(A):
    T = A.transpose()[0]
    return segsum(T.rowptr, T.val.astype(LD) * T.val.astype(LD), LD)


def check_rows(y, A, x, tile, what="", seq=None):
    """The SpMV contract on a device result y = A x: tile rows equal the sequential sum bit for bit, long rows are within
    γ_k (|A||x|)_i of the long-double sum. (For Aᵀ x pass the transpose.)"""
    y = np.asarray(y, dtype=np.float64)
    seq = spmv_sequential(A, x) if seq is None else seq
    lng = long_rows(A.rowptr, tile)
    bad = np.flatnonzero((y.view(np.int64) != seq.view(np.int64)) & ~lng)
    assert bad.size == 0, f"{what}: {bad.size} tile rows differ from the sequential sum, first row {bad[0]}: {y[bad[0]]!r} != {seq[bad[0]]!r}"
    if lng.any():
        rows = np.flatnonzero(lng)
        ref, mag = spmv_longdouble(A, x)[rows], abs_spmv(A, x)[rows]
        err = np.abs(y[rows].astype(LD) - ref)
        bound = gamma(A.rowlen[rows]).astype(LD) * mag
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (f"{what}: long row {rows[worst]} ({A.rowlen[rows[worst]]} non-zeros): error {float(err[worst]):.3e} "
                                      f"> γ_k|A||x| = {float(bound[worst]):.3e}")


# ---------------------------------------------------------------------------------------------------------------- Gershgorin
def gershgorin_rows(A, dtype=np.float64):
    """(d, rad) per row: d the sum of the stored diagonal entries, rad the sum of |v| of the others, both in CSR order."""
    diag = A.col == A.rowof
    zero = np.zeros(A.nnz)
    return (segsum(A.rowptr, np.where(diag, A.val, zero), dtype), segsum(A.rowptr, np.where(diag, zero, np.abs(A.val)), dtype))


def gershgorin_pair(A):
    """{max_i −(d_i − rad_i), max_i (d_i + rad_i)} in float64 as k_csr_gershgorin forms them (the device hands out −lo and hi)."""
    d, rad = gershgorin_rows(A)
    return float(np.max(-(d - rad))), float(np.max(d + rad))


def gershgorin_check(pair, A, tile, what=""):
    """Tile rows are exact (max is exact in any order), a long row's −(d − rad) and d + rad carry γ_{k+1} (Σ|v|) (k additions
    in some order and the final one). |max a − max b| ≤ max |a − b|, so the pair is within the largest per-row bound of the
    pair formed from the float64 values of the tile rows and the long-double values of the long rows."""
    lng = long_rows(A.rowptr, tile)
    d, rad = gershgorin_rows(A)
    if not lng.any():
        ref = (float(np.max(-(d - rad))), float(np.max(d + rad)))
        assert (float(pair[0]), float(pair[1])) == ref, f"{what}: {tuple(pair)!r} != {ref!r}"
        return
    dl, radl = gershgorin_rows(A, LD)
    mlo = np.where(lng, -(dl - radl), (-(d - rad)).astype(LD))
    mhi = np.where(lng, dl + radl, (d + rad).astype(LD))
    mag = segsum(A.rowptr, np.abs(A.val), LD)
    bound = float(np.max(np.where(lng, gamma(A.rowlen + 1).astype(LD) * mag, LD(0))))
    for got, ref, name in ((pair[0], np.max(mlo), "-lo"), (pair[1], np.max(mhi), "hi")):
        assert abs(LD(got) - ref) <= bound, f"{what}: {name} = {got!r}, reference {float(ref)!r}, bound {bound:.3e}"


# ---------------------------------------------------------------------------------------------------------------- JᵀJ + λ D
def normal_matrix(J, lam=0.0, d=None):
    """(rowptr, col, val) of N = JᵀJ + λ diag(d) as nk_normal_plan assembles it: the pattern of JᵀJ with every diagonal position
    present (a structurally missing one still receives the damping), each entry the sum over the rows r of J, ascending, of
    fl(J[r, i] · J[r, j]), then for a diagonal entry + fl(λ d_i) when d is given (d = None: no damping term at all)."""
    ii, jj, pp = [], [], []
    for r in range(J.n):
        a, e = J.rowptr[r], J.rowptr[r + 1]
        c, v = J.col[a:e], J.val[a:e]
        ii.append(np.repeat(c, e - a))
        jj.append(np.tile(c, e - a))
        pp.append(np.multiply.outer(v, v).ravel())
    ii = np.concatenate(ii + [np.arange(J.n)])          # the diagonal positions, with no product behind them
    jj = np.concatenate(jj + [np.arange(J.n)])
    pp = np.concatenate(pp + [np.zeros(J.n)])
    real = np.concatenate([np.ones(ii.size - J.n, dtype=bool), np.zeros(J.n, dtype=bool)])
    order = np.lexsort((jj, ii))                       # stable: the pairs of an entry stay in row order
    ii, jj, pp, real = ii[order], jj[order], pp[order], real[order]
    first = np.concatenate([[True], (ii[1:] != ii[:-1]) | (jj[1:] != jj[:-1])])
    ptr = np.concatenate([np.flatnonzero(first), [ii.size]])
    ci, cj = ii[first], jj[first]
    # the structural diagonal's zero product comes last in its entry (it was appended last): adding +0.0 changes nothing
    val = segsum(ptr, pp)
    if d is not None:
        dg = ci == cj
        val[dg] = val[dg] + lam * np.asarray(d, dtype=np.float64)[ci[dg]]
    rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=J.n))])
    return rp, cj, val


# ---------------------------------------------------------------------------------------------------------------- epilogues
def epilogue(mode, s, x, r=None, yacc=None, dinv=None, c1=0.0, c2=0.0, theta=0.0, out_scale=None):
    """spmv_store_row applied to the row sums s, every operation rounded in the dtype of s. Returns a dict of the vectors the
    mode writes (y, r, dnew, yacc)."""
    t = s.dtype.type
    cv = lambda a: None if a is None else np.asarray(a).astype(s.dtype)
    x, r, yacc, dinv = cv(x), cv(r), cv(yacc), cv(dinv)
    with np.errstate(all="ignore"):
        if mode == 0:
            return dict(y=s if out_scale is None else t(out_scale) * s)
        if mode == 3:
            v = s - t(theta) * x
            return dict(y=v if out_scale is None else t(out_scale) * v)
        if mode == 2:
            return dict(y=r - s)
        if mode == 4:
            return dict(r=r - s)
        rr = r - s
        dn = t(c1) * x + t(c2) * (rr if dinv is None else dinv * rr)
        return dict(r=rr, dnew=dn, yacc=yacc + dn)


def epilogue_bound(mode, delta, S, x, r=None, yacc=None, dinv=None, c1=0.0, c2=0.0, theta=0.0, out_scale=None):
    """Bounds on |computed − exact| of what `epilogue` returns when ŝ carries the error δ (δ, S = exact sums, long double).
    step(z, E): one more rounded operation whose exact result is z and whose operand error, scaled to the result, is E."""
    u = LD(U)
    step = lambda z, E: E + u * (np.abs(z) + E)
    cv = lambda a: None if a is None else np.asarray(a).astype(LD)
    x, r, yacc, dinv = cv(x), cv(r), cv(yacc), cv(dinv)
    if mode == 0:
        return dict(y=delta if out_scale is None else step(LD(out_scale) * S, abs(LD(out_scale)) * delta))
    if mode == 3:
        tx = LD(theta) * x                             # the device subtracts fl(θ x): u |θ x| more
        Ev = step(S - tx, delta + u * np.abs(tx))
        return dict(y=Ev if out_scale is None else step(LD(out_scale) * (S - tx), abs(LD(out_scale)) * Ev))
    if mode in (2, 4):
        return {("y" if mode == 2 else "r"): step(r - S, delta)}
    RR = r - S
    Err = step(RR, delta)
    W, Ew = (RR, Err) if dinv is None else (dinv * RR, step(dinv * RR, np.abs(dinv) * Err))
    c1x = LD(c1) * x                                   # the device adds fl(c1 x): u |c1 x| more
    E2 = step(LD(c2) * W, abs(LD(c2)) * Ew)
    DN = c1x + LD(c2) * W
    Edn = step(DN, E2 + u * np.abs(c1x))
    return dict(r=Err, dnew=Edn, yacc=step(yacc + DN, Edn))


# --------------------------------------------------------------------------------------------------------------------- cases
N_WIDE = 70000


def _near(r, n, rng, k):
    """k distinct columns within ±8 of r, the diagonal among them."""
    c = np.clip(r + rng.choice(np.arange(-8, 9), size=k + 4, replace=False), 0, n - 1)
    c = np.unique(np.concatenate([[r], c]))
    return c[:k] if r in c[:k] else np.concatenate([[r], c[:k - 1]])


def _exact_tile(tile, rng):
    """First block: tile / 8 rows of 8 non-zeros = exactly `tile`; the next row would overflow it. Then a second block of exactly
    `tile` made of rows of 1 … 15 non-zeros, then a tail."""
    n = tile // 8 + 600
    rows = [np.sort(rng.choice(n, 8, replace=False)) for _ in range(tile // 8)]
    left = tile
    while left > 0:
        k = min(left, int(rng.integers(1, 16)))
        rows.append(np.sort(rng.choice(n, k, replace=False)))
        left -= k
    while len(rows) < n:
        rows.append(np.sort(rng.choice(n, 3, replace=False)))
    return from_rows(n, rows, rng)


def _long(tile, rng):
    """Rows of tile (a tile-path block of its own), tile + 1 and 3·tile + 17 non-zeros (long rows) between short rows; row 1
    stores only its diagonal; column 0 is stored in some rows only."""
    n = 3 * tile + 17 + 40
    rows = [_near(r, n, rng, 3) for r in range(n)]
    rows = [c[c != 0] if r % 7 else c for r, c in enumerate(rows)]
    rows[1] = np.array([1])
    rows[5] = np.sort(rng.choice(n, tile, replace=False))
    rows[9] = np.sort(rng.choice(n, tile + 1, replace=False))
    rows[n - 3] = np.concatenate([[n - 3], np.sort(rng.choice(np.setdiff1d(np.arange(n), [n - 3]), 3 * tile + 16, replace=False))])
    rows[20] = np.arange(n)                            # dense: also column 20 … of the transpose
    rows = [np.union1d(c, [20]) if 30 <= r < 30 + tile + 300 else c for r, c in enumerate(rows)]   # column 20: a long row of Aᵀ
    return from_rows(n, rows, rng)


def _empty_run(tile, rng):
    """First and last rows empty; 2600 empty rows with a few 1-entry rows inside (blocks that reach the 1024-row cap: the loop
    past a lane's second row), then rows of 2 (blocks of > 512 rows for the large tiles) and of 3 (> 256 rows)."""
    n = 2600 + 2200 + 1500 + 7
    rows = [np.array([], dtype=np.int64)] * n
    for r in (100, 700, 1023, 1024, 1500, 2047, 2599):
        rows[r] = np.array([int(rng.integers(0, n))])
    for r in range(2600, 4800):
        rows[r] = np.array([r, (r * 7) % n])
    for r in range(4800, n - 7):
        rows[r] = np.array([r - 1, r, (r * 11) % n])
    return from_rows(n, rows, rng)


def _n1(tile, rng):
    return Mat(1, [0, 1], [0], [rng.standard_normal()])


def _ragged(tile, rng):
    """Unsymmetric random pattern, 0 … 40 non-zeros a row; rows 50 … 99 store no diagonal, rows 100 … 119 only the diagonal,
    rows 200 … 209 are empty, column 7 is empty, column 0 is stored by a few rows, some stored values are exact zeros."""
    n = 2500
    rows = []
    for r in range(n):
        k = int(rng.integers(0, 41))
        c = rng.choice(n, k, replace=False) if r % 3 else np.clip(r + rng.integers(-60, 61, size=k), 0, n - 1)
        c = np.union1d(c, [r])
        if 50 <= r < 100:
            c = c[c != r]
        if 100 <= r < 120:
            c = np.array([r])
        if 200 <= r < 210:
            c = np.array([], dtype=np.int64)
        c = c[c != 7]
        if r % 97 != 3:
            c = c[c != 0]
        else:
            c = np.union1d(c, [0])
        rows.append(c)
    M = from_rows(n, rows, rng)
    k = np.flatnonzero((M.col != 0) & (np.arange(M.nnz) % 53 == 0))
    M.val[k] = 0.0
    return M


def _small(tile, rng):
    """The ragged pattern in small (0 … 8 non-zeros a row, n = 600): JᵀJ stays sparse. Column 7 is empty (a structurally
    missing diagonal of JᵀJ), rows 50 … 99 store no diagonal, some stored values are exact zeros."""
    n = 600
    rows = []
    for r in range(n):
        c = np.union1d(rng.choice(n, int(rng.integers(0, 9)), replace=False), [r] if not 50 <= r < 100 else [])
        rows.append(c[c != 7].astype(np.int64))
    M = from_rows(n, rows, rng)
    M.val[np.arange(M.nnz) % 31 == 0] = 0.0
    return M


def _uniform4(n, rng):
    """4 non-zeros a row at columns r − 2 … r + 2 (clipped): blocks of tile / 4 rows (the 1024-row cap at tile 4096)."""
    rows = []
    for r in range(n):
        lo = min(max(r - 2, 0), n - 4)
        rows.append(np.arange(lo, lo + 4))
    return rows


def _wide(tile, rng):
    """n = 70 000, 4 non-zeros a row: the diagonal, a neighbour and two columns anywhere — offsets from the block's first row
    far beyond ±32767 in both directions."""
    n = N_WIDE
    far = rng.integers(0, n, size=(n, 2))
    rows = [np.array([r, min(r + 1, n - 1), far[r, 0], far[r, 1]]) for r in range(n)]
    fix = []
    for r, c in enumerate(rows):                       # exactly 4 distinct columns a row, so the blocks stay uniform
        c = np.unique(c)
        k = 0
        while c.size < 4:
            k += 1
            c = np.unique(np.append(c, (r + 40000 + k) % n))
        fix.append(c)
    return from_rows(n, fix, rng)


def _edge(tile, rng, plus, minus):
    """Uniform blocks of tile / 4 rows; one entry at first row + `plus` in a block near the top, one at first row + `minus` (< 0)
    in a block near the bottom; every other offset is small."""
    n = N_WIDE
    rows = _uniform4(n, rng)
    rpb = min(tile // 4, ROWCAP)
    b_top, b_bot = 3, (n // rpb) - 3
    r0, r1 = b_top * rpb, b_bot * rpb
    assert r0 + plus < n and r1 + minus >= 0
    for r, target in ((r0 + rpb // 2, r0 + plus), (r1 + rpb // 3, r1 + minus)):
        c = rows[r].copy()
        c[0 if target < c[0] else 3] = target          # replace the outermost entry: still 4 ascending distinct columns
        rows[r] = c
    return from_rows(n, rows, rng)


# name: (generator, seed, tags). Tags name the paths the case is there for; tests/test_csr_reference.py proves each one from
# `rowblocks` for every tile.
_GEN = {
    "exact_tile": (_exact_tile, 11, ("block_exact_tile",)),
    "long": (_long, 12, ("long_row", "row_tile", "row_tile_plus_1", "row_3tile_17", "diag_only_row", "long_column")),
    "empty_run": (_empty_run, 13, ("row_cap", "rows_gt_256", "rows_gt_512", "first_last_empty")),
    "n1": (_n1, 14, ("n1",)),
    "ragged": (_ragged, 15, ("no_diagonal", "diag_only_row", "explicit_zero", "empty_column", "empty_row")),
    "small": (_small, 19, ("no_diagonal", "explicit_zero", "empty_column")),
    "wide": (_wide, 16, ("col32",)),
    "edge16": (lambda t, g: _edge(t, g, 32767, -32768), 17, ("col16_edge",)),
    "edge32": (lambda t, g: _edge(t, g, 32768, -32769), 18, ("col32_edge",)),
}
CASES = tuple(_GEN)
LARGE = ("wide", "edge16", "edge32")
TAGS = {name: g[2] for name, g in _GEN.items()}
FITS16 = {name: name not in ("wide", "edge32") for name in _GEN}     # the 16-bit predicate of every case, for every tile


@functools.lru_cache(maxsize=64)
def case(name, tile):
    gen, seed, _tags = _GEN[name]
    return gen(tile, np.random.default_rng(1000 * seed + tile))


def vector(name, tile, k=0):
    return np.random.default_rng(77 + 13 * k + tile + len(name)).standard_normal(case(name, tile).n)


def block_kinds(M, tile):
    """Which kinds of block `rowblocks` makes of M: the set of tags a matrix proves by its block structure."""
    rb = rowblocks(M.rowptr, tile)
    nnzb = M.rowptr[rb[1:]] - M.rowptr[rb[:-1]]
    nrow = np.diff(rb)
    ln = M.rowlen
    kinds = set()
    if np.any((nnzb == tile) & (nrow > 1)):
        kinds.add("block_exact_tile")
    if np.any(nnzb > tile):
        kinds.add("long_row")
    if np.any(ln == tile):
        kinds.add("row_tile")
    if np.any(ln == tile + 1):
        kinds.add("row_tile_plus_1")
    if np.any(ln == 3 * tile + 17):
        kinds.add("row_3tile_17")
    if np.any(nrow == ROWCAP):
        kinds.add("row_cap")
    if np.any((nrow > 256) & (nnzb <= tile)):
        kinds.add("rows_gt_256")
    if np.any((nrow > 512) & (nnzb <= tile)):
        kinds.add("rows_gt_512")
    if M.n > 1 and ln[0] == 0 and ln[-1] == 0:
        kinds.add("first_last_empty")
    if M.n == 1:
        kinds.add("n1")
    diag = np.bincount(M.rowof[M.col == M.rowof], minlength=M.n)
    if np.any((diag == 0) & (ln > 0)):
        kinds.add("no_diagonal")
    if np.any((diag == 1) & (ln == 1)):
        kinds.add("diag_only_row")
    if np.any(M.val == 0.0):
        kinds.add("explicit_zero")
    if M.n > 1 and np.any(np.bincount(M.col, minlength=M.n) == 0):
        kinds.add("empty_column")
    if M.n > 1 and np.any(ln == 0):
        kinds.add("empty_row")
    if np.any(np.bincount(M.col, minlength=M.n) > tile):
        kinds.add("long_column")
    lo, hi = block_offsets(M, tile)
    if lo < -40000 and hi > 40000:
        kinds.add("col32")
    if (lo, hi) == (-32768, 32767):
        kinds.add("col16_edge")
    if (lo, hi) == (-32769, 32768):
        kinds.add("col32_edge")
    return kinds
