"""Float64 restatement of block cyclic reduction (csrc/nk_bcr.hip), the case list of tests/test_gpu_bcr.py and the bounds
those cases are tested with.

The restatement carries out the SAME operation as the device engine in NumPy float64: level 0 cut into b × b blocks (b the
bandwidth rounded up to 32, identity padding of the last block row), the odd rows inverted explicitly, P = A D⁻¹, Q = C D⁻¹,
D' = D − P C − Q A, A' = −P A, C' = −Q C, recursion on the even rows, and the down / bottom / up solve sweeps. Blocks are
inverted as on the device: order ≤ 128 by Gauss–Jordan (on the diagonal, or with implicit row pivoting), larger orders by
the 2 × 2 Schur recursion with the leading part of order 128 (n ≤ 256) or 256.

It is the CALIBRATION INSTRUMENT, not the judge. The judge is the long-double solve of band_lu_reference.reference_solve;
the restatement tells how far a correct float64 implementation of this algorithm sits from it, and the bounds below are
8 × that (rounded up to a power of two). The factor 8 covers what legitimately differs between restatement and kernel: the
accumulation order of the 16×16×4 MFMA against BLAS over K up to 512, the sweeps' eight-way split sums, and the pivot
reciprocal by v_rcp_f64 + two Newton steps. tests/test_bcr_reference.py pins that the restatement stays at or below a
quarter of every bound on every committed case."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import band_lu_reference as BR
from band_lu_reference import U64

# ---------------------------------------------------------------------------------------------------------------- bounds
# (backward error in u, forward error in κ∞ u) per (family, inversion kernel). Each is 8 × the maximum the restatement
# reached over the committed runs (RUNS below) of that family and kernel, rounded up to a power of two;
# tests/test_bcr_reference.py::test_the_bounds_are_eight_times_the_restatement_rounded_up recomputes them. κ∞ is exact (dense
# inverse) up to n = 2500, and Hager–Higham's 1-norm estimate of A⁻ᵀ — a LOWER bound, so the stricter side — above.
# The Brusselator Jacobian is not diagonally dominant (its reaction block has row sums of either sign) and cyclic reduction
# with explicit inverses is not backward stable on it: the restatement itself sits at 250 … 310 u there, hence 4096 u.
BOUNDS = {
    # family, kernel: (backward u, forward κu)          measured maximum of the restatement
    ("dominant", "never"): (128, 64),                  # 9.65 u, 6.09 κu
    ("dominant", "always"): (64, 64),                  # 6.89 u, 4.31 κu
    ("spd", "never"): (32, 0.5),                       # 3.03 u, 0.045 κu
    ("spd", "always"): (32, 1),                        # 3.94 u, 0.069 κu
    ("outer", "never"): (32, 16),                      # 2.34 u, 1.26 κu
    ("bratu", "never"): (128, 0.125),                  # 13.0 u, 0.014 κu
    ("bratu", "always"): (128, 0.125),                 # 13.0 u, 0.014 κu
    ("brusselator", "never"): (4096, 0.125),           # 306 u, 0.011 κu
    ("exchanged", "always"): (64, 64),                 # 6.46 u, 4.04 κu
}
MARGIN = 8


class Breakdown(ArithmeticError):
    """A zero or non-finite pivot inside a block inversion: the device raises its failure flag there."""

    def __init__(self, level, what):
        super().__init__(f"level {level}: {what}")
        self.level = level


def block_order(kl, ku):
    return ((max(kl, ku, 1) + 31) // 32) * 32


def levels_of(m):
    """Levels of the reduction of m block rows: m, ⌈m/2⌉, …, 1."""
    return (m - 1).bit_length() + 1


# --------------------------------------------------------------------------------------------------------- leaf inverses
def _check(p):
    if not (p != 0 and np.isfinite(p)):
        raise Breakdown(-1, f"pivot {p}")


def inv_gauss_jordan(M):
    """In-register Gauss–Jordan on the diagonal pivots, as k_bcr_inv128<false>: per pivot k, a ← a − a[:, k] (a[k, :] / a_kk),
    then row k, column k and the pivot take their Gauss–Jordan values."""
    a = np.array(M, dtype=np.float64)
    for k in range(a.shape[0]):
        _check(a[k, k])
        pinv = 1.0 / a[k, k]
        mr = a[:, k].copy()
        rk = a[k, :] * pinv
        a -= np.multiply.outer(mr, rk)
        a[k, :] = rk
        a[:, k] = -mr * pinv
        a[k, k] = pinv
    return a


def inv_gauss_jordan_pivoted(M):
    """Gauss–Jordan with implicit row pivoting, as k_bcr_inv128<true>: the pivot of column k is the largest entry among the
    rows not yet used (the first of equals); no row moves, and with p_k the pivot row of column k and σ its inverse, entry
    (i, j) of the working array is entry (σ(i), p_j) of the inverse."""
    a = np.array(M, dtype=np.float64)
    n = a.shape[0]
    used = np.zeros(n, dtype=bool)
    prow = np.zeros(n, dtype=np.int64)
    for k in range(n):
        mag = np.where(used, -1.0, np.nan_to_num(np.abs(a[:, k]), nan=-0.5, posinf=np.inf))
        p = int(np.argmax(mag))
        prow[k], used[p] = p, True
        _check(a[p, k])
        pinv = 1.0 / a[p, k]
        mr = a[:, k].copy()
        rk = a[p, :] * pinv
        a -= np.multiply.outer(mr, rk)
        a[p, :] = rk
        a[:, k] = -mr * pinv
        a[p, k] = pinv
    sigma = np.empty(n, dtype=np.int64)
    sigma[prow] = np.arange(n)
    out = np.empty_like(a)
    out[np.ix_(sigma, prow)] = a
    return out


LEAVES = {"never": inv_gauss_jordan, "always": inv_gauss_jordan_pivoted}


def invert(M, leaf=inv_gauss_jordan):
    """Inverse of one block: order ≤ 128 by `leaf`; otherwise [E F; G H] with E of order 128 (n ≤ 256) or 256 and
    E ← E⁻¹; T = G E; W = E F; H ← (H − T F)⁻¹; F ← −W H; G ← −H T; E ← E − F T  (bcr_invert)."""
    n = M.shape[0]
    if n <= 128:
        return leaf(M)
    n1 = 128 if n <= 256 else 256
    E, F, G, H = M[:n1, :n1], M[:n1, n1:], M[n1:, :n1], M[n1:, n1:]
    E = invert(E, leaf)
    T = G @ E
    W = E @ F
    H = invert(H - T @ F, leaf)
    F = -(W @ H)
    G = -(H @ T)
    E = E - F @ T
    return np.block([[E, F], [G, H]])


# ------------------------------------------------------------------------------------------------------ cyclic reduction
def cut(J, b):
    """Level 0: (A, D, C) arrays of m blocks b × b — sub-diagonal, diagonal and super-diagonal blocks of the block
    tridiagonal form; rows ≥ n of the last block row carry a unit diagonal."""
    J = sp.coo_matrix(J)
    n = J.shape[0]
    m = (n + b - 1) // b
    A, D, C = (np.zeros((m, b, b)) for _ in range(3))
    bi, bj = J.row // b, J.col // b
    assert np.all(np.abs(bi - bj) <= 1), "bandwidth exceeds the block order"
    for arr, off in ((A, -1), (D, 0), (C, 1)):
        s = bj - bi == off
        arr[bi[s], J.row[s] % b, J.col[s] % b] = J.data[s]
    for r in range(n, m * b):
        D[m - 1, r - (m - 1) * b, r - (m - 1) * b] = 1.0
    return A, D, C


class Factorisation:
    """Block cyclic reduction of a banded matrix in float64; `pivot` = "never" | "always" selects the leaf inverse."""

    def __init__(self, J, pivot="never", b=None):
        self.n = J.shape[0]
        self.b = b or block_order(*BR.bandwidths(J))
        leaf = LEAVES[pivot]
        A, D, C = cut(J, self.b)
        self.lv = []
        level = 0
        while True:
            m = D.shape[0]
            L = dict(m=m, A=A, D=D, C=C)
            self.lv.append(L)
            try:
                if m == 1:
                    D[0] = invert(D[0], leaf)
                    break
                for k in range(1, m, 2):
                    D[k] = invert(D[k], leaf)
            except Breakdown as e:
                raise Breakdown(level, str(e)) from None
            m2 = (m + 1) // 2
            P, Q = np.zeros((m2,) + D.shape[1:]), np.zeros((m2,) + D.shape[1:])
            A2, D2, C2 = np.zeros_like(P), D[0::2].copy(), np.zeros_like(P)
            for i in range(m2):
                j = 2 * i
                if j >= 1:
                    P[i] = A[j] @ D[j - 1]
                    D2[i] -= P[i] @ C[j - 1]
                    A2[i] = -(P[i] @ A[j - 1])
                if j + 1 < m:
                    Q[i] = C[j] @ D[j + 1]
                    D2[i] -= Q[i] @ A[j + 1]
                    C2[i] = -(Q[i] @ C[j + 1])
            L["P"], L["Q"] = P, Q
            A, D, C = A2, D2, C2
            level += 1

    @property
    def levels(self):
        return len(self.lv)

    def solve(self, rhs):
        b = self.b
        f = np.zeros(self.lv[0]["m"] * b)
        f[:self.n] = rhs
        fs = [f.reshape(-1, b)]
        for L in self.lv[:-1]:                         # down
            f, m = fs[-1], L["m"]
            g = f[0::2].copy()
            for i in range(g.shape[0]):
                j = 2 * i
                if j >= 1:
                    g[i] -= L["P"][i] @ f[j - 1]
                if j + 1 < m:
                    g[i] -= L["Q"][i] @ f[j + 1]
            fs.append(g)
        x = (self.lv[-1]["D"][0] @ fs[-1][0])[None, :]  # bottom
        for L, f in zip(self.lv[-2::-1], fs[-2::-1]):  # up
            m = L["m"]
            y = np.empty_like(f)
            y[0::2] = x
            for k in range(1, m, 2):
                t = f[k] - L["A"][k] @ y[k - 1]
                if k + 1 < m:
                    t = t - L["C"][k] @ y[k + 1]
                y[k] = L["D"][k] @ t
            x = y
        return x.ravel()[:self.n].copy()


def solve(J, rhs, pivot="never"):
    return Factorisation(J, pivot).solve(rhs)


# -------------------------------------------------------------------------------------------------------------- families
def spd(n, w, seed, delta=1e-3):
    """B Bᵀ + δ ‖B Bᵀ‖∞ I with B lower banded of width w and one zero column: κ∞ ≈ 1e3 … 1e4 at δ = 1e-3, multipliers O(1),
    no dominant diagonal to damp a wrong P C or Q A term."""
    w = min(w, n - 1)
    rng = np.random.default_rng(seed)
    B = sp.diags([rng.standard_normal(n - k) for k in range(w + 1)], [-k for k in range(w + 1)], shape=(n, n)).tolil()
    B[:, n // 2] = 0.0
    B = sp.csr_matrix(B)
    G = (B @ B.T).tocsr()
    return (G + sp.identity(n) * (delta * BR.norm_inf(G))).tocsr()


def outer(n, kl, ku, seed):
    """Only the diagonals 0, −kl and +ku: everything between them is fill."""
    rng = np.random.default_rng(seed)
    d = {0: 4.0 + rng.random(n), -kl: rng.uniform(-1.0, 1.0, n - kl), ku: rng.uniform(-1.0, 1.0, n - ku)}
    return sp.diags(list(d.values()), list(d.keys()), shape=(n, n)).tocsr()


def bratu(ns, seed):
    from oracle import reference_restatement as R
    return sp.csr_matrix(R.Bratu2D(ns, 6.0).jac(0.3 * np.random.default_rng(seed).standard_normal(ns * ns)))


def brusselator(N, seed):
    """The Brusselator Jacobian with its unknowns renumbered (a symmetric permutation Π J Πᵀ: the same linear system). In the
    problem's own numbering i + N j + N² k the species couple at distance N² and the periodic boundary at N (N − 1): two
    block rows at N = 16 (the router sends that to the band LU) and beyond the largest block order at N = 24. Interleaving
    the species and folding the periodic index j (0, N − 1, 1, N − 2, …) gives 2 (i + N fold(j)) + k and half bandwidth 4N:
    block order 64 at N = 16, 96 at N = 24."""
    from oracle import reference_restatement as R
    P = R.Brusselator2D(N)
    J = sp.csr_matrix(P.jac(1.0 + 0.1 * np.random.default_rng(seed).standard_normal(P.n)))
    i, j, k = np.meshgrid(np.arange(N), np.arange(N), np.arange(2), indexing="ij")
    fold = np.where(j < (N + 1) // 2, 2 * j, 2 * (N - 1 - j) + 1)
    new = np.empty(P.n, dtype=np.int64)
    new[(i + N * j + N * N * k).ravel()] = (2 * (i + N * fold) + k).ravel()
    Pm = sp.csr_matrix((np.ones(P.n), (new, np.arange(P.n))), shape=(P.n, P.n))
    out = sp.csr_matrix(Pm @ J @ Pm.T)
    out.sort_indices()
    return out


def exchanged(n, kl, ku, seed):
    """(J, M, perm): rows 2i ↔ 2i + 1 of a dominant band matrix M exchanged, J = M[perm]. M[2i + 1, 2i] is zeroed first, so J
    has an exact zero on the diagonal of every even row and its dominant entries next to the diagonal — inside the diagonal
    blocks and inside their 128-leaves (pairs start on even rows), so row pivoting inside the leaves is sufficient."""
    assert n % 2 == 0
    M = BR.dominant_band(n, kl, ku, seed).tolil()
    for i in range(0, n, 2):
        M[i + 1, i] = 0.0
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    perm = np.arange(n).reshape(-1, 2)[:, ::-1].ravel()
    J = sp.csr_matrix(M[perm, :])
    J.sort_indices()
    return J, M, perm


def cond_inf_estimate(A):
    """Hager–Higham estimate of κ∞(A) = ‖A‖∞ ‖A⁻ᵀ‖₁ through a sparse LU (a lower bound, sharp within a small factor), for
    matrices too large to invert densely that are not diagonally dominant."""
    A = sp.csc_matrix(A)
    lu = spla.splu(A)
    op = spla.LinearOperator(A.shape, matvec=lambda v: lu.solve(v, trans="T"), rmatvec=lambda v: lu.solve(v))
    return BR.norm_inf(A) * float(spla.onenormest(op))


# ----------------------------------------------------------------------------------------------------------------- cases
def _case(name, family, args, modes=("never",), m=None):
    return dict(name=name, family=family, args=tuple(args), modes=tuple(modes), m=m)


def _order_pair(b):
    """(kl, ku) of the block-order sweep: kl ≠ ku with the larger on either side; kl = b exactly at b = 128, 256, 384, 512
    and ku = b exactly at b = 64, 192, 320, 448 (the diagonal of the triangular operand is populated there)."""
    i = b // 32
    return [(b, max(1, b - 37)), (b - 5, b // 2 + 3), (max(1, b - 41), b), (b // 3, b - 9)][i % 4]


BOTH = {32, 128, 160, 256, 288, 512}          # block orders run on both inversion kernels
ORDERS = list(range(32, 513, 32))
LEVEL_M = [4, 5, 6, 7, 8, 9, 15, 16, 17, 33]


def _cases():
    out = []
    # every block order: four block rows (five below b = 288), the last one partly padding
    for b in ORDERS:
        kl, ku = _order_pair(b)
        m = 4 if b >= 288 else 5
        out.append(_case(f"order{b}", "dominant", (m * b - b // 3, kl, ku, 100 + b), ("never", "always") if b in BOTH else ("never",), m))
    # every level shape at b = 32: n = m b, m b − (b − 1) (a full block of padding minus one row) and m b − 1
    for m in LEVEL_M:
        for n in (m * 32, m * 32 - 31, m * 32 - 1):
            kl, ku = ((29, 32), (32, 17))[(m + n) % 2]
            out.append(_case(f"levels{m}_{n}", "dominant", (n, kl, ku, 200 + n), m=m))
    for w, n in ((32, 150), (100, 600), (150, 700), (250, 1100), (270, 1200), (500, 2040)):
        out.append(_case(f"spd{w}", "spd", (n, w, 300 + w), ("never", "always")))
    for n, kl, ku in ((300, 64, 40), (777, 130, 160), (1500, 320, 300)):
        out.append(_case(f"outer{max(kl, ku)}", "outer", (n, kl, ku, 400 + n)))
    for ns in (32, 50, 100, 130):
        out.append(_case(f"bratu{ns}", "bratu", (ns, 500 + ns), ("never", "always") if ns != 50 else ("never",)))
    for N in (16, 24):
        out.append(_case(f"brusselator{N}", "brusselator", (N, 600 + N)))
    # pivoting that is needed, under the Schur recursion (128 + 32, 128 + 128, 256 + 256)
    for b, (kl, ku) in ((160, (140, 155)), (256, (250, 200)), (512, (470, 505))):
        out.append(_case(f"exchanged{b}", "exchanged", (4 * b - 2 * (b // 6), kl, ku, 700 + b), ("always",), 4))
    return out


CASES = {c["name"]: c for c in _cases()}
_BUILD = {"dominant": BR.dominant_band, "spd": spd, "outer": outer, "bratu": bratu, "brusselator": brusselator,
          "exchanged": lambda *a: exchanged(*a)[0]}


def matrix(name):
    c = CASES[name]
    return _BUILD[c["family"]](*c["args"])


# every (case, inversion kernel, right-hand side) the device is measured on; right-hand sides 1 … 3 belong to the
# factor-once-solve-many test
MANY_RHS = "order160"
RUNS = [(c["name"], mode, 0) for c in _cases() for mode in c["modes"]] + [(MANY_RHS, "never", r) for r in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def problem(name, rhs=0):
    """(J, b, x_ref, κ∞, block order, levels) of a committed case; b = J x_true in long double, x_ref the long-double solve
    (of the un-exchanged matrix with the permuted right-hand side for the "exchanged" family: an unpivoted LU cannot factor
    J itself)."""
    c = CASES[name]
    J = matrix(name)
    n = J.shape[0]
    x_true = np.random.default_rng(c["args"][-1] + 7 + 1000 * rhs).standard_normal(n)
    b = BR.manufactured(J, x_true)
    if c["family"] == "exchanged":
        _J, M, perm = exchanged(*c["args"])
        x_ref = BR.reference_solve(M, b[np.argsort(perm)])
    else:
        x_ref = BR.reference_solve(J, b)
    kappa = BR.cond_inf(J) if n <= 2500 else cond_inf_estimate(J)
    blk = block_order(*BR.bandwidths(J))
    m = (n + blk - 1) // blk
    assert m >= 4 and (c["m"] is None or c["m"] == m), (name, m)
    return J, b, x_ref, kappa, blk, levels_of(m)


def errors(J, x, b, x_ref, kappa):
    """(backward error in u, forward error in κ∞ u)."""
    return BR.backward_error(J, x, b) / U64, BR.forward_error(x, x_ref) / (kappa * U64)


def check(name, mode, x, what="", rhs=0):
    """Assert the bounds of the case's family and inversion kernel; returns (backward u, forward κu)."""
    J, b, x_ref, kappa, _blk, _lev = problem(name, rhs)
    bb, fb = BOUNDS[(CASES[name]["family"], mode)]
    assert np.all(np.isfinite(x)), f"{name} {mode} {what}: non-finite solution"
    be, fe = errors(J, x, b, x_ref, kappa)
    print(f"{name} {mode} {what}: backward {be:.2f} u (bound {bb}), forward {fe:.3f} κu (bound {fb}), κ∞ = {kappa:.3e}")
    assert be <= bb, f"{name} {mode} {what}: backward error {be:.1f} u > {bb} u"
    assert fe <= fb, f"{name} {mode} {what}: forward error {fe:.3f} κu > {fb} κu (κ∞ = {kappa:.3e})"
    return be, fe


# ------------------------------------------------------------------------------------------------------------ breakdowns
def breakdown(kind, n=256, kl=20, ku=30, seed=21):
    """(pattern matrix, values on that pattern, dense matrix) of a 32-block, eight-block-row matrix on which the reduction
    meets a singular block:
      zero_column  column 40 exactly zero (the diagonal block of odd row 1 is singular at level 0)
      inf, nan     on the diagonal at row 40
      cancel_odd   [[2, 3], [4, 6]] on rows / columns 40, 41, otherwise decoupled: inside odd row 1's diagonal block
      cancel_schur rows / columns p = 93 (even block row 2) and q = 97 (odd block row 3) decoupled from everything else and
                   [[a_pp, a_pq], [a_qp, a_qq]] = [[6, 3], [4, 2]]: every level-0 block is regular (a_qq = 2), and the level-1
                   diagonal block gets 6 − (3 · 1/2) · 4 = 0 on an otherwise empty row and column — exactly, every factor
                   being a power of two times a small integer. Level-1 row 1 (odd) is inverted at level 1."""
    Jp = BR.dominant_band(n, kl, ku, seed)
    M = Jp.toarray()
    if kind == "zero_column":
        M[:, 40] = 0.0
    elif kind in ("inf", "nan"):
        M[40, 40] = np.inf if kind == "inf" else np.nan
    elif kind == "cancel_odd":
        M[40:42, :] = 0.0
        M[:, 40:42] = 0.0
        M[40, 40], M[40, 41], M[41, 40], M[41, 41] = 2.0, 3.0, 4.0, 6.0
    elif kind == "cancel_schur":
        p, q = 93, 97
        M[[p, q], :] = 0.0
        M[:, [p, q]] = 0.0
        M[p, p], M[p, q], M[q, p], M[q, q] = 6.0, 3.0, 4.0, 2.0
    else:
        raise KeyError(kind)
    vals = sp.csr_matrix((M[Jp.nonzero()], Jp.indices, Jp.indptr), shape=(n, n))   # the zeros stay stored entries
    return Jp, vals, M


BREAKDOWN_LEVEL = {"zero_column": 0, "inf": 0, "nan": 0, "cancel_odd": 0, "cancel_schur": 1}
