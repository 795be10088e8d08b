"""Reference for the device band LU (csrc/nk_band.hip): the same operation, an UNPIVOTED right-looking LU with its forward
and backward substitution, carried out in np.longdouble (x87 extended precision on x86-64: 64-bit mantissa, eps 1.1e-19).

The kernel does not pivot, so a pivoted reference would measure different pivot choices instead of the kernel's arithmetic.
Two storage forms run the same elimination: dense (n up to a few thousand) and band (long chains). Fill-in of an unpivoted
LU stays inside the band, so both only touch the kl × ku window below / right of each pivot.

Manufactured solutions: `manufactured(A, x_true)` forms b = A x_true in long double and rounds it to float64; the reference
then solves A x = b for that rounded b, which is what the kernel is given.
"""
import numpy as np
import scipy.sparse as sp
from numpy.lib.stride_tricks import as_strided

LD = np.longdouble
U64 = np.finfo(np.float64).eps / 2          # unit roundoff of float64 (2^-53)
BACKWARD_BOUND = 256                         # ‖b − A x‖∞ / (‖A‖∞ ‖x‖∞) ≤ 256 u
FORWARD_FACTOR = 64                          # ‖x − x_ref‖∞ / ‖x_ref‖∞ ≤ 64 κ∞(A) u


class ZeroPivot(ArithmeticError):
    """An exact zero (or non-finite) pivot: the unpivoted LU does not exist."""

    def __init__(self, k):
        super().__init__(f"zero or non-finite pivot at row {k}")
        self.k = k


def bandwidths(A):
    """(kl, ku) of a sparse or dense matrix, from its stored pattern (explicit zeros count, as on the device)."""
    C = sp.coo_matrix(A)
    if C.nnz == 0:
        return 0, 0
    d = C.col.astype(np.int64) - C.row.astype(np.int64)
    return int(max(0, -d.min())), int(max(0, d.max()))


def _check_pivot(p, k):
    if not (p != 0 and np.isfinite(p)):
        raise ZeroPivot(k)


# ------------------------------------------------------------------------------------------------------------ dense form
def lu_dense(A, kl=None, ku=None):
    """Unpivoted LU of a dense matrix in long double, L (unit lower) and U packed in one array. The rank-1 update of step k
    is restricted to rows k+1 … k+kl and columns k+1 … k+ku: everything outside that window is zero and stays zero."""
    M = np.array(A, dtype=LD)
    n = M.shape[0]
    if kl is None or ku is None:
        kl, ku = bandwidths(M)
    for k in range(n):
        _check_pivot(M[k, k], k)
        r1, c1 = min(n, k + 1 + kl), min(n, k + 1 + ku)
        if r1 == k + 1:
            continue
        M[k + 1:r1, k] /= M[k, k]
        if c1 > k + 1:
            M[k + 1:r1, k + 1:c1] -= np.multiply.outer(M[k + 1:r1, k], M[k, k + 1:c1])
    return M, kl, ku


def solve_dense(F, b):
    """Forward (unit L) and backward (U) substitution with the packed factors of `lu_dense`, in long double."""
    M, kl, ku = F
    n = M.shape[0]
    x = np.array(b, dtype=LD)
    for k in range(n):
        r1 = min(n, k + 1 + kl)
        x[k + 1:r1] -= M[k + 1:r1, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] /= M[k, k]
        r0 = max(0, k - ku)
        x[r0:k] -= M[r0:k, k] * x[k]
    return x


# ------------------------------------------------------------------------------------------------------------- band form
# Row-aligned band storage G[i, j − i + kl] (row i's band is one contiguous row of G). Element (k + 1 + r, k + 1 + c) of the
# trailing window sits at G[k + 1, kl] + r·(ldab − 1) + c, so the window is one strided view and the rank-1 update is in place.
def to_band(A, kl, ku):
    A = sp.coo_matrix(A)
    n = A.shape[0]
    G = np.zeros((n + 1, kl + ku + 1), dtype=LD)
    G[A.row, A.col - A.row + kl] = np.asarray(A.data, dtype=LD)
    return G


def lu_band(A, kl=None, ku=None):
    """The same elimination as `lu_dense` on row-aligned band storage (long chains: memory n (kl + ku + 1))."""
    if kl is None or ku is None:
        kl, ku = bandwidths(A)
    n = A.shape[0]
    G = to_band(A, kl, ku)
    ldab, it = kl + ku + 1, G.itemsize
    for k in range(n):
        piv = G[k, kl]
        _check_pivot(piv, k)
        ml, mu = min(kl, n - 1 - k), min(ku, n - 1 - k)
        if ml == 0:
            continue
        col = as_strided(G[k + 1:, kl - 1:], shape=(ml,), strides=((ldab - 1) * it,))      # (k + 1 + r, k)
        col /= piv
        if mu == 0:
            continue
        win = as_strided(G[k + 1:, kl:], shape=(ml, mu), strides=((ldab - 1) * it, it))   # (k + 1 + r, k + 1 + c)
        win -= np.multiply.outer(col, G[k, kl + 1:kl + 1 + mu])
    return G, n, kl, ku


def solve_band(F, b):
    G, n, kl, ku = F
    ldab, it = kl + ku + 1, G.itemsize
    x = np.array(b, dtype=LD)
    for k in range(n):
        ml = min(kl, n - 1 - k)
        if ml:
            x[k + 1:k + 1 + ml] -= as_strided(G[k + 1:, kl - 1:], shape=(ml,), strides=((ldab - 1) * it,)) * x[k]
    for k in range(n - 1, -1, -1):
        x[k] /= G[k, kl]
        mu = min(ku, k)
        if mu:   # column k above the diagonal: (k − m, k) at G[k − m, kl + m], m = mu … 1
            x[k - mu:k] -= as_strided(G[k - mu:, kl + mu:], shape=(mu,), strides=((ldab - 1) * it,)) * x[k]
    return x


# ------------------------------------------------------------------------------------------------------------- matrices
def dominant_band(n, kl, ku, seed):
    """Full band of N(0, 1) entries plus 1.5 (kl + ku + 1) on the diagonal: strictly row diagonally dominant (seeded, so that
    a child process rebuilds the same matrix)."""
    rng = np.random.default_rng(seed)
    kl, ku = min(kl, n - 1), min(ku, n - 1)
    M = sp.diags([rng.standard_normal(n - abs(k)) for k in range(-kl, ku + 1)], range(-kl, ku + 1), shape=(n, n)).tocsr()
    return (M + sp.identity(n) * (1.5 * (kl + ku + 1))).tocsr()


# --------------------------------------------------------------------------------------------------------- measurements
def matvec_ld(A, x):
    """A x in long double (A sparse or dense, x any float type)."""
    C = sp.coo_matrix(A)
    y = np.zeros(C.shape[0], dtype=LD)
    np.add.at(y, C.row, np.asarray(C.data, dtype=LD) * np.asarray(x, dtype=LD)[C.col])
    return y


def manufactured(A, x_true):
    """b = A x_true computed in long double, rounded to float64."""
    return matvec_ld(A, x_true).astype(np.float64)


def reference_solve(A, b, dense=None):
    """x_ref (long double) of A x = b by the unpivoted LU; dense storage up to n = 2500 unless told otherwise."""
    n = A.shape[0]
    if dense is None:
        dense = n <= 2500
    if dense:
        return solve_dense(lu_dense(A.toarray() if sp.issparse(A) else A), b)
    return solve_band(lu_band(sp.csr_matrix(A)), b)


def norm_inf(A):
    return float(abs(sp.csr_matrix(A)).sum(axis=1).max())


def cond_inf(A):
    """κ∞(A) = ‖A‖∞ ‖A⁻¹‖∞ from the dense matrix (float64 inverse: a bound needs it to a few digits only)."""
    D = A.toarray() if sp.issparse(A) else np.asarray(A)
    return float(np.abs(D).sum(axis=1).max() * np.abs(np.linalg.inv(D)).sum(axis=1).max())


def cond_inf_dominant(A):
    """Upper bound of κ∞(A) for a strictly row diagonally dominant A (Varah: ‖A⁻¹‖∞ ≤ 1 / min_i (|a_ii| − Σ_{j≠i} |a_ij|)),
    for matrices too large to invert densely."""
    A = sp.csr_matrix(A)
    d = np.abs(A.diagonal())
    off = np.asarray(abs(A).sum(axis=1)).ravel() - d
    gap = float((d - off).min())
    assert gap > 0, "not strictly diagonally dominant"
    return norm_inf(A) / gap


def backward_error(A, x, b):
    """‖b − A x‖∞ / (‖A‖∞ ‖x‖∞), residual in long double."""
    r = np.asarray(b, dtype=LD) - matvec_ld(A, x)   # the quotient in long double too: 2^±1000-scaled matrices stay in range
    nA = np.max(np.asarray(abs(sp.csr_matrix(A)).sum(axis=1), dtype=LD))
    return float(np.max(np.abs(r)) / (nA * np.max(np.abs(np.asarray(x, dtype=LD)))))


def forward_error(x, x_ref):
    x_ref = np.asarray(x_ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(x, dtype=LD) - x_ref)) / np.max(np.abs(x_ref)))


def check_solution(A, x, b, x_ref, kappa, what=""):
    """Assert both bounds of the band-LU tests; returns (backward, forward / (κ u)) for messages."""
    be = backward_error(A, x, b)
    fe = forward_error(x, x_ref)
    assert np.all(np.isfinite(x)), f"{what}: non-finite solution"
    assert be <= BACKWARD_BOUND * U64, f"{what}: backward error {be / U64:.1f} u > {BACKWARD_BOUND} u"
    assert fe <= FORWARD_FACTOR * kappa * U64, \
        f"{what}: forward error {fe:.3e} = {fe / (kappa * U64):.2f} κu > {FORWARD_FACTOR} κu (κ∞ = {kappa:.3e})"
    return be / U64, fe / (kappa * U64)
