"""Sequential references and the case list for the preconditioner objects (csrc/nk_precond.hip), shared by
tests/test_precond_reference.py (no GPU: pins the references and the schedule every case selects) and
tests/test_gpu_precond_direct.py (the device against them, bit for bit).

The library is built with -ffp-contract=off and every kernel does one rounding per operation, a row's entries in CSR order, so the
reference is the same sweep in float64 and the assertion is equality of bits. The sweeps are written once over a scalar type:
float64 (Python floats: IEEE double, one rounding per operation) and np.longdouble (the yardstick that says how far a float64
sweep is from the exact one).

  ilu0_sweep   IKJ factorisation of A[perm][:, perm] on its own pattern — ilu_factor_row: for every lower entry (i, k) in ascending
               k, l = a_ik / u_kk, then a_ij -= l * u_kj for the j > k both rows hold, ascending j.
  tri_apply    ilu_lower_row / ilu_upper_row: s = b[perm[i]]; s -= lu[p] * y[c] in ascending stored column; the upper row divides
               once at its end; the result is scattered to out[perm[i]].
  level_widths level(i) = 1 + max level of the rows i refers to (0 without any), for L from the lower entries and for U from the
               upper ones (rows descending): the number of rows in every level.
  chain_pays   the rule of ilu_symbolic / ilut_update: a schedule walks its levels inside one persistent workgroup of 1024 threads
               when nlev > 16 and sum(ceil(width / 1024)) < 5 * nlev, else it launches one kernel per level.

Every builder is seeded and strictly diagonally dominant by rows (off-diagonal entries uniform in (−1, 1) divided by their number
in the row, diagonal in [1.5, 2.5)), except dense(40) = randn + 6 I."""
import functools
import math

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = 2.0 ** -52
CHAIN_THREADS = 1024     # ILU_CHAIN_THREADS


# ------------------------------------------------------------------------------------------------------------------ sweeps
def _scalars(a, dtype):
    """a as a list of scalars of `dtype` (Python floats for float64: the fastest IEEE double there is in Python)"""
    if dtype in (np.float64, float):
        return np.asarray(a, dtype=np.float64).tolist()
    return list(np.asarray(a).astype(dtype))


def permuted(A, perm=None):
    """A[perm][:, perm] as CSR with ascending columns: row i is the original row perm[i]"""
    A = sp.csr_matrix(A)
    if perm is not None:
        A = A[perm][:, perm].tocsr()
    A = A.copy()
    A.sort_indices()
    return A


def diag_positions(rp, ci):
    n = rp.size - 1
    dg = np.empty(n, dtype=np.int64)
    for i in range(n):
        row = ci[rp[i]:rp[i + 1]]
        d = int(np.searchsorted(row, i))
        if d >= row.size or row[d] != i:
            raise ArithmeticError(f"row {i} has no stored diagonal entry")
        dg[i] = rp[i] + d
    return dg


def ilu0_sweep(A, perm=None, dtype=np.float64):
    """(rp, ci, dg, lu): the factors in one row-major array on the pattern of A[perm][:, perm] — L strictly below the diagonal
    (unit diagonal implied), U on and above; lu as an array of `dtype`. Raises ArithmeticError on a zero or non-finite pivot."""
    Ap = permuted(A, perm)
    rp, ci = Ap.indptr.astype(np.int64), Ap.indices.astype(np.int64)
    dg = diag_positions(rp, ci)
    n = rp.size - 1
    lu = _scalars(Ap.data, dtype)
    rpl, cil, dgl = rp.tolist(), ci.tolist(), dg.tolist()
    for i in range(n):
        qe = rpl[i + 1]
        for p in range(rpl[i], dgl[i]):
            k = cil[p]
            l = lu[p] / lu[dgl[k]]
            lu[p] = l
            q, s, se = p + 1, dgl[k] + 1, rpl[k + 1]
            while q < qe and s < se:
                if cil[q] == cil[s]:
                    lu[q] -= l * lu[s]
                    q += 1
                    s += 1
                elif cil[q] < cil[s]:
                    q += 1
                else:
                    s += 1
        d = lu[dgl[i]]
        if d == 0.0 or not math.isfinite(d):
            raise ArithmeticError(f"ILU(0): zero or non-finite pivot in row {i}")
    return rp, ci, dg, np.array(lu, dtype=dtype)


def tri_apply(rp, ci, dg, lu, perm, x, dtype=np.float64):
    """out = Pᵀ U⁻¹ L⁻¹ P x by the two substitutions of the device rows, in their order of operations, in `dtype`"""
    n = rp.size - 1
    x = np.asarray(x)
    b = _scalars(x if perm is None else x[np.asarray(perm)], dtype)
    luv = _scalars(lu, dtype)
    rpl, cil, dgl = np.asarray(rp).tolist(), np.asarray(ci).tolist(), np.asarray(dg).tolist()
    y = [None] * n
    for i in range(n):
        s = b[i]
        for p in range(rpl[i], dgl[i]):
            s -= luv[p] * y[cil[p]]
        y[i] = s
    z = [None] * n
    for i in range(n - 1, -1, -1):
        s = y[i]
        for p in range(dgl[i] + 1, rpl[i + 1]):
            s -= luv[p] * z[cil[p]]
        s /= luv[dgl[i]]
        z[i] = s
    z = np.array(z, dtype=dtype)
    if perm is None:
        return z
    out = np.empty_like(z)
    out[np.asarray(perm)] = z
    return out


def split_lu(rp, ci, lu):
    """(L with its unit diagonal, U) as SciPy CSR — what ILU0Preconditioner.factors() and the oracle's ilu0 / ilut return"""
    n = rp.size - 1
    M = sp.csr_matrix((np.asarray(lu, dtype=np.float64), ci, rp), shape=(n, n))
    return (sp.tril(M, -1) + sp.identity(n)).tocsr(), sp.triu(M, 0).tocsr()


def pack_lu(L, U):
    """the inverse of split_lu: (rp, ci, dg, lu) with ascending columns from a unit lower L and an upper U (no entry is added or
    summed: the patterns are disjoint)"""
    L, U = sp.coo_matrix(sp.tril(L, -1)), sp.coo_matrix(U)
    n = U.shape[0]
    r = np.concatenate([L.row, U.row]).astype(np.int64)
    c = np.concatenate([L.col, U.col]).astype(np.int64)
    v = np.concatenate([L.data, U.data])
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, r + 1, 1)
    rp = np.cumsum(rp)
    return rp, c, diag_positions(rp, c), v


# --------------------------------------------------------------------------------------------------------------- schedules
def level_widths(Ap):
    """(widths of L's levels, widths of U's levels) of a matrix in its final ordering (any object with indptr / indices)"""
    Ap = sp.csr_matrix(Ap).copy()
    Ap.sort_indices()
    rp, ci = Ap.indptr.tolist(), Ap.indices.tolist()
    n = len(rp) - 1
    lev = [0] * n
    for i in range(n):
        l = 0
        for p in range(rp[i], rp[i + 1]):
            if ci[p] >= i:
                break
            l = max(l, lev[ci[p]] + 1)
        lev[i] = l
    wl = np.bincount(np.array(lev, dtype=np.int64)) if n else np.zeros(0, dtype=np.int64)
    lev = [0] * n
    for i in range(n - 1, -1, -1):
        l = 0
        for p in range(rp[i + 1] - 1, rp[i] - 1, -1):
            if ci[p] <= i:
                break
            l = max(l, lev[ci[p]] + 1)
        lev[i] = l
    wu = np.bincount(np.array(lev, dtype=np.int64)) if n else np.zeros(0, dtype=np.int64)
    return wl, wu


def chain_pays(widths):
    nlev = len(widths)
    return nlev > 16 and sum((int(w) + CHAIN_THREADS - 1) // CHAIN_THREADS for w in widths) < 5 * nlev


# ---------------------------------------------------------------------------------------------------------------- builders
def _dominant(n, rows, cols, seed):
    """CSR with the given off-diagonal pattern and a full diagonal: off-diagonal entries uniform in (−1, 1) over the number of
    them in their row, diagonal in [1.5, 2.5) — strictly diagonally dominant by rows, so ILU(0) exists in any ordering"""
    rng = np.random.default_rng(seed)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    keep = rows != cols
    key = np.unique(rows[keep] * n + cols[keep])
    rows, cols = key // n, key % n
    cnt = np.bincount(rows, minlength=n)
    off = rng.uniform(-1.0, 1.0, rows.size) / cnt[rows]
    off[off == 0.0] = 0.25
    d = 1.5 + rng.random(n)
    A = sp.csr_matrix((np.concatenate([off, d]), (np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)]))),
                      shape=(n, n))
    A.sort_indices()
    assert A.nnz == rows.size + n
    return A


def interleaved_tridiag(m, nb, seed=11):
    """nb independent tridiagonal chains of length m, row index l * nb + b: m levels of exactly nb rows, for L and for U"""
    l, b = np.meshgrid(np.arange(m - 1), np.arange(nb), indexing="ij")
    lo = (l * nb + b).ravel()
    return _dominant(m * nb, np.concatenate([lo + nb, lo]), np.concatenate([lo, lo + nb]), seed)


def mixed_schedule(seed=12):
    """n = 1545: a 20-row tridiagonal chain, 1500 rows coupled (both ways) to the last row of that chain only, a 25-row
    tridiagonal chain each row of which is also coupled (both ways) to three of the 1500, all 75 distinct. L: levels 0–19 of one
    row, level 20 of 1500 rows, levels 21–45 of one row. U: the last chain backwards on levels 0–24, the 1425 uncoupled rows of
    the fan on level 0 with its last row (1426 rows), the coupled ones on levels 1–25, then the first chain on 26–45."""
    a, f, c = 20, 1500, 25
    r, q = [], []

    def both(i, j):
        r.extend((i, j)); q.extend((j, i))
    for i in range(1, a):
        both(i, i - 1)
    for i in range(a, a + f):
        both(i, a - 1)
    for k in range(c):
        i = a + f + k
        if k:
            both(i, i - 1)
        for t in range(3):
            both(i, a + 17 + 19 * (3 * k + t))      # 75 distinct rows of the fan, spread over it
    return _dominant(a + f + c, r, q, seed)


def lower_bidiagonal(n=500, seed=13):
    i = np.arange(1, n)
    return _dominant(n, i, i - 1, seed)


def upper_bidiagonal(n=500, seed=13):
    return lower_bidiagonal(n, seed).T.tocsr()


def random_unsymmetric(n=2000, density=0.002, seed=14):
    P = sp.random(n, n, density=density, random_state=np.random.default_rng(seed), format="coo")
    return _dominant(n, P.row, P.col, seed + 100)


def random_banded(n=2000, density=0.05, band=60, seed=15):
    P = sp.random(n, n, density=density, random_state=np.random.default_rng(seed), format="coo")
    keep = np.abs(P.row.astype(np.int64) - P.col) <= band
    return _dominant(n, P.row[keep], P.col[keep], seed + 100)


def dense(n=40, seed=16):
    A = sp.csr_matrix(np.random.default_rng(seed).standard_normal((n, n)) + 6.0 * np.eye(n))
    A.sort_indices()
    assert A.nnz == n * n
    return A


def diagonal(n=300, seed=17):
    return _dominant(n, [], [], seed)


# name → (builder, orderings it runs under)
CASES = {
    "tridiag16x300": (lambda: interleaved_tridiag(16, 300), ("natural",)),
    "tridiag17x300": (lambda: interleaved_tridiag(17, 300), ("natural",)),
    "tridiag17x4096": (lambda: interleaved_tridiag(17, 4096), ("natural",)),
    "tridiag17x4097": (lambda: interleaved_tridiag(17, 4097), ("natural",)),
    "mixed_schedule": (mixed_schedule, ("natural", "multicolor")),
    "lower_bidiagonal": (lower_bidiagonal, ("natural",)),
    "upper_bidiagonal": (upper_bidiagonal, ("natural",)),
    "random_unsymmetric": (random_unsymmetric, ("natural", "multicolor")),
    "random_banded": (random_banded, ("natural", "multicolor")),
    "dense40": (dense, ("natural",)),
    "diagonal300": (diagonal, ("natural",)),
    "one": (lambda: diagonal(1), ("natural",)),
}
CASE_IDS = [(name, o) for name, (_, orderings) in CASES.items() for o in orderings]

# (name, ordering) → (levels of L, levels of U, widest of L, widest of U, L in the chain kernel, U in the chain kernel): what the
# builders give under the rule above, asserted by test_precond_reference.py; a GPU case asserts its entry before it runs
EXPECTED = {
    ("tridiag16x300", "natural"): (16, 16, 300, 300, False, False),        # 16 levels: not more than 16
    ("tridiag17x300", "natural"): (17, 17, 300, 300, True, True),
    ("tridiag17x4096", "natural"): (17, 17, 4096, 4096, True, True),       # 17 · 4 = 68 < 85: four strided passes per level
    ("tridiag17x4097", "natural"): (17, 17, 4097, 4097, False, False),     # 17 · 5 = 85 is not < 85
    ("mixed_schedule", "natural"): (46, 46, 1500, 1426, True, True),       # a level of two strided passes inside a chain
    ("mixed_schedule", "multicolor"): (3, 3, 1510, 1484, False, False),
    ("lower_bidiagonal", "natural"): (500, 1, 1, 500, True, False),        # chainL != chainU inside one apply
    ("upper_bidiagonal", "natural"): (1, 500, 500, 1, False, True),
    ("random_unsymmetric", "natural"): (10, 13, 481, 485, False, False),
    ("random_unsymmetric", "multicolor"): (7, 7, 659, 497, False, False),
    ("random_banded", "natural"): (196, 185, 97, 120, True, True),
    ("random_banded", "multicolor"): (8, 8, 545, 325, False, False),
    ("dense40", "natural"): (40, 40, 1, 1, True, True),
    ("diagonal300", "natural"): (1, 1, 300, 300, False, False),
    ("one", "natural"): (1, 1, 1, 1, False, False),
}


@functools.lru_cache(maxsize=None)
def matrix(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def permutation(name, ordering):
    """perm[permuted row] = original row (None for the natural ordering) — the oracle's restatement of multicolor_perm"""
    if ordering == "natural":
        return None
    from oracle import reference_restatement as R
    return R.multicolor_permutation(matrix(name))[0]


@functools.lru_cache(maxsize=None)
def schedule(name, ordering):
    wl, wu = level_widths(permuted(matrix(name), permutation(name, ordering)))
    return (len(wl), len(wu), int(wl.max()), int(wu.max()), chain_pays(wl), chain_pays(wu))


@functools.lru_cache(maxsize=None)
def factors(name, ordering, dtype=np.float64):
    """the cached sweep of a case (callers must not write into it)"""
    out = ilu0_sweep(matrix(name), permutation(name, ordering), dtype)
    for a in out:
        a.setflags(write=False)
    return out


def vectors(name):
    """(a random x, A @ ones) of a case"""
    A = matrix(name)
    return np.random.default_rng(5).standard_normal(A.shape[0]), A @ np.ones(A.shape[0])


def new_values(A, seed=21):
    """other values on the same pattern, still strictly diagonally dominant: every entry scaled by a factor in [0.5, 1), the
    diagonal then raised by 1"""
    B = A.copy()
    B.data = A.data * (0.5 + 0.5 * np.random.default_rng(seed).random(A.nnz))
    B = sp.csr_matrix(B)
    B.setdiag(B.diagonal() + 1.0)
    B.sort_indices()
    assert B.nnz == A.nnz and np.array_equal(B.indices, A.indices)
    return B


def shuffled(A, seed=22):
    """(rowptr, col, order): the same matrix with every row's columns in a random order; order[k] is the position in A's sorted
    arrays of the entry stored at k, so A.data[order] are its values"""
    rng = np.random.default_rng(seed)
    order = np.arange(A.nnz)
    for i in range(A.shape[0]):
        rng.shuffle(order[A.indptr[i]:A.indptr[i + 1]])
    return A.indptr.astype(np.int32), A.indices[order].astype(np.int32), order


# ------------------------------------------------------------------------------------------------------------------ ILU(τ)
def _coo(n, entries):
    r, c, v = zip(*entries)
    A = sp.csr_matrix((np.array(v, dtype=np.float64), (r, c)), shape=(n, n))
    A.sort_indices()
    return A


# name → (A, τ, L without its unit diagonal, U), worked out by hand (every number is exact in float64)
ILUT_HAND = {
    # |z| == τ is kept: the rule is |z| ≥ τ, tested before the division by the pivot
    "tau_equal": (_coo(2, [(0, 0, 2.0), (0, 1, 1.0), (1, 0, 1.0), (1, 1, 2.0)]), 1.0,
                  [[0, 0], [0.5, 0]], [[2, 1], [0, 1.5]]),
    # one ulp above: both off-diagonal entries are dropped
    "tau_above": (_coo(2, [(0, 0, 2.0), (0, 1, 1.0), (1, 0, 1.0), (1, 1, 2.0)]), float(np.nextafter(1.0, 2.0)),
                  [[0, 0], [0, 0]], [[2, 0], [0, 2]]),
    # (1, 1) is not stored: its pivot 0 − 0.5 · 1 is created by fill
    "missing_diagonal": (_coo(3, [(0, 0, 2.0), (0, 1, 1.0), (1, 0, 1.0), (1, 2, 1.0), (2, 1, 1.0), (2, 2, 3.0)]), 0.0,
                         [[0, 0, 0], [0.5, 0, 0], [0, -2, 0]], [[2, 1, 0], [0, -0.5, 1], [0, 0, 5]]),
}


def ilut_random400():
    """the matrix of test_gpu_precond.py's ILU(τ) case"""
    rng = np.random.default_rng(3)
    A = (sp.random(400, 400, density=0.02, random_state=5, format="csr") + sp.diags(3.0 + rng.random(400))).tocsr()
    A.sort_indices()
    return A


def ilut_brusselator():
    from oracle import reference_restatement as R
    pb = R.Brusselator2D(16)
    A = sp.csr_matrix(pb.jac(pb.u0() + 0.05 * np.random.default_rng(3).standard_normal(pb.n)))
    A.sort_indices()
    return A


def tridiagonal3000():
    """the tridiagonal matrix of test_gpu_precond.py: 3000 levels of one row each way"""
    n = 3000
    return sp.diags([-1.0 * np.ones(n - 1), 2.5 + np.sin(np.arange(n)), -1.3 * np.ones(n - 1)], [-1, 0, 1]).tocsr()


# name → (builder, τ)
ILUT_CASES = {
    "random400": (ilut_random400, 0.05),
    "brusselator16": (ilut_brusselator, 50.0),
    "unsymmetric400_tau0": (lambda: random_unsymmetric(400, 0.005), 0.0),
    "unsymmetric400_tau0.05": (lambda: random_unsymmetric(400, 0.005), 0.05),
    "unsymmetric400_tau0.5": (lambda: random_unsymmetric(400, 0.005), 0.5),
    "tridiagonal3000_tau0": (tridiagonal3000, 0.0),
}


@functools.lru_cache(maxsize=None)
def ilut_case(name):
    """(A, τ, (rp, ci, dg, lu) of the oracle's Crout factors)"""
    from oracle import reference_restatement as R
    build, tau = ILUT_CASES[name]
    A = build()
    packed = pack_lu(*R.ilut(A, tau))
    for a in packed:
        a.setflags(write=False)
    return A, tau, packed


def gaps(name, ordering):
    """(factor gap, apply gap) in units of 2⁻⁵²: max |float64 sweep − long-double sweep| over max |long-double sweep|, for the
    factors and for one application to the case's random vector"""
    rp, ci, dg, lu = factors(name, ordering)
    _, _, _, lul = factors(name, ordering, LD)
    perm = permutation(name, ordering)
    x = vectors(name)[0]
    y, yl = tri_apply(rp, ci, dg, lu, perm, x), tri_apply(rp, ci, dg, lul, perm, x, LD)
    return (float(np.max(np.abs(lu.astype(LD) - lul)) / np.max(np.abs(lul)) / EPS),
            float(np.max(np.abs(y.astype(LD) - yl)) / np.max(np.abs(yl)) / EPS))
