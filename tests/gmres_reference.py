"""Cases, data, the reference and the assertions for restarted GMRES (csrc/nk_gmres.hip, csrc/nk_sstep.hip), in plain NumPy.
tests/test_gpu_gmres.py hands the device's iterates to the check_* functions below; tests/test_gmres_reference.py hands them
the oracle's float64 formulations (which must pass) and float64 copies of the reference with one planted defect each (which must
fail), without a GPU.

The reference is restarted GMRES(m) in np.longdouble: Arnoldi by modified Gram–Schmidt applied twice, Givens rotations and a
back-substitution, products formed from the CSR arrays — nothing is densified. In exact arithmetic every orthogonalisation the
library offers (mgs, cgs2, cgs, dcgs2, dcgs2_1r, sstep) produces the same iterates, so this one solve judges all of them. The
stopping rule is the device's (nk_gmres_begin_body, k_givens): tol = atol + rtol·‖r₀‖ fixed by the first cycle, the test made on
the recurrence residual after every column and on β at every cycle's begin, hn == 0 a (converged) breakdown, every norm the
preconditioned one under a left preconditioner.

Operator families (each with a seeded b):
  convdiff(nx, ny, pe)   five-point upwind convection–diffusion, nonsymmetric: diagonal 4 + 1.5·pe, west −1 − pe, south
                         −1 − pe/2, east and north −1; unknown i + nx·j
  cyclic(n)              the permutation P e_j = e_{j+1 mod n} with b = 4·e₀: every quantity exact in binary floating point, the
                         residual stays 4 for n − 1 steps, step n is an exact breakdown with x = 4·e_{n−1}
  scaled_identity(n)     A = 2 I, b = 4·e_j: an exact breakdown at step 1 with x = b/2

Tolerances. TABLE holds, per (operator, restart) of the fixed-work group, the largest relative deviation of the oracle's
float64 formulations (oracle.reference_restatement: gmres with mgs / cgs2 / dcgs2, gmres_dcgs2_1r, gmres_sstep with monomial
blocks of 4 and Newton blocks of 15) from this reference over the fixed-work counts the GPU file uses. GROUP_TABLE holds the same
for every other solve of the GPU file, one row per solve (all_specs): there the formulations are the column forms and, where
the GPU file runs s-step forms on the solve, gmres_sstep with monomial blocks of 4 and of 6 (the device's automatic size without
spectrum bounds) and Newton blocks of 15 on a plain CSR operator (oracle_on_spec). Each spread is rounded UP to a power of two —
the CPU file asserts the committed figure to be EQUAL to the measured one, and a rounded figure survives a NumPy whose sums
associate differently —; tol_x and tol_r are 100 times that and never below 1e-13. The device's rounding (tree reductions, lagged
normalisation, block orthogonalisation) is a further ordering, not one of those measured: the spread between orderings predicts
another ordering to a small factor, hence the 100. No bound may exceed the project's limits (1e-9 on x, 1e-10·rnorm0 on norms): a
solve that would is run for fewer steps (zero-rhs-63). The CPU file asserts all of this. Regenerate the tables with

    python tests/gmres_reference.py

which prints the two dictionaries below (TABLE and GROUP_TABLE)."""
import functools
import math
import zlib
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
LIMIT_X, LIMIT_R, FLOOR = 1e-9, 1e-10, 1e-13
FACTOR = 100.0
KMAX = 130

COLUMN_FORMS = ("mgs", "cgs2", "cgs", "dcgs2", "dcgs2_1r")
FORMS = COLUMN_FORMS + ("sstep0", "sstep4")          # sstep0: automatic block size, sstep4: blocks of 4


def form_args(form):
    """keyword arguments of nls.GMRES for a form name"""
    if form.startswith("sstep"):
        return dict(ortho="sstep", sstep=int(form[5:]))
    return dict(ortho=form)


def need_longdouble():
    if not LONGDOUBLE_OK:
        import pytest
        pytest.skip("np.longdouble has fewer than 64 significand bits on this machine")


# ------------------------------------------------------------------------------------------------------------- operators
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def rhs(n, *key):
    return np.random.default_rng(_seed("b", n, *key)).standard_normal(n)


def positive(n, *key):
    """seeded positive weights in [0.5, 2)"""
    return np.random.default_rng(_seed("w", n, *key)).uniform(0.5, 2.0, n)


@functools.lru_cache(maxsize=None)
def convdiff(nx, ny, pe):
    n = nx * ny
    rp, ci, va = [0], [], []
    for j in range(ny):
        for i in range(nx):
            row = []
            if j > 0:
                row.append((i + nx * (j - 1), -1.0 - pe / 2))
            if i > 0:
                row.append((i - 1 + nx * j, -1.0 - pe))
            row.append((i + nx * j, 4.0 + 1.5 * pe))
            if i < nx - 1:
                row.append((i + 1 + nx * j, -1.0))
            if j < ny - 1:
                row.append((i + nx * (j + 1), -1.0))
            ci += [c for c, _ in row]
            va += [v for _, v in row]
            rp.append(len(ci))
    return SimpleNamespace(name=f"convdiff{nx}x{ny}pe{pe}", n=n, rowptr=np.array(rp, dtype=np.int32),
                           colind=np.array(ci, dtype=np.int32), vals=np.array(va), b=rhs(n, "convdiff", nx, ny, pe))


CONVDIFF_SHAPE = {1: (1, 1), 2: (2, 1), 3: (3, 1), 31: (31, 1), 33: (33, 1), 63: (9, 7), 65: (13, 5), 99: (33, 3),
                  4097: (241, 17)}
PES = (0.5, 2.0)


def convdiff_n(n, pe):
    return convdiff(*CONVDIFF_SHAPE[n], pe)


@functools.lru_cache(maxsize=None)
def cyclic(n):
    b = np.zeros(n)
    b[0] = 4.0
    # row i of P has its one at column i − 1 (mod n): (P e_j)_i = [i == j + 1]
    return SimpleNamespace(name=f"cyclic{n}", n=n, rowptr=np.arange(n + 1, dtype=np.int32),
                           colind=((np.arange(n) - 1) % n).astype(np.int32), vals=np.ones(n), b=b)


@functools.lru_cache(maxsize=None)
def scaled_identity(n, j=None):
    j = n // 2 if j is None else j
    b = np.zeros(n)
    b[j] = 4.0
    return SimpleNamespace(name=f"scaled_identity{n}", n=n, rowptr=np.arange(n + 1, dtype=np.int32),
                           colind=np.arange(n, dtype=np.int32), vals=np.full(n, 2.0), b=b)


def to_scipy(case):
    import scipy.sparse as sp
    return sp.csr_matrix((case.vals, case.colind, case.rowptr), shape=(case.n, case.n))


class Operator:
    """x ↦ (A + σ·diag(w)) x, or (AᵀA + λ·diag(d)) x in the normal form, from the CSR arrays in `dtype`."""

    def __init__(self, case, shift=0.0, weights=None, normal=False, damping=None, dtype=LD, defect=None):
        self.n, self.dtype, self.defect = case.n, dtype, defect
        self.rp = np.asarray(case.rowptr, dtype=np.int64)
        assert np.all(np.diff(self.rp) > 0) or case.n == 0, "reduceat needs every row to hold an entry"
        self.ci = np.asarray(case.colind, dtype=np.int64)
        self.va = np.asarray(case.vals, dtype=dtype)
        self.row = np.repeat(np.arange(case.n), np.diff(self.rp))
        self.sigma = dtype(shift)
        self.w = None if weights is None else np.asarray(weights, dtype=dtype)
        self.normal = bool(normal)
        self.lam, self.d = (dtype(0), None) if damping is None else (dtype(damping[1]), np.asarray(damping[0], dtype=dtype))

    def A(self, x):
        return np.add.reduceat(self.va * x[self.ci], self.rp[:-1]) if self.n else x.copy()

    def AT(self, x):
        y = np.zeros(self.n, dtype=self.dtype)
        np.add.at(y, self.ci, self.va * x[self.row])
        return y

    def __call__(self, x):
        x = np.asarray(x, dtype=self.dtype)
        if self.normal:
            y = self.A(self.A(x)) if self.defect == "normal_a_for_at" else self.AT(self.A(x))
            if self.d is not None:
                y = y + self.lam * (self.d * self.d if self.defect == "damping_d_squared" else self.d) * x
        else:
            y = self.A(x)
        if self.sigma != 0:
            y = y + self.sigma * (x if self.w is None or self.defect == "shift_without_weights" else self.w * x)
        return y


# ------------------------------------------------------------------------------------------------------------- the reference
DEFECTS = ("givens_not_applied_to_g", "update_k_minus_1", "restart_reuses_recurrence", "x0_ignored_in_r0", "x0_not_added",
           "tol_is_max", "left_not_on_b", "shift_without_weights", "damping_d_squared", "normal_a_for_at",
           "dot_drops_last_entry", "subdiagonal_float32")


def gmres(op, b, x0=None, atol=0.0, rtol=1e-8, restart=30, itmax=300, fixed_iters=0, Ml=None, Mr=None, snapshots=(),
          dtype=LD, defect=None):
    """Restarted GMRES(m) on the callable `op` in `dtype` (np.longdouble: THE reference; np.float64 with `defect`: one of the
    planted defects of tests/test_gmres_reference.py). Ml, Mr: callables y = P⁻¹ x in `dtype`. Returns a namespace with x,
    iters, restarts, converged, failed, rnorm0, rnorm, residuals (per step, [0] = rnorm0) and snap: {count: (x, rnorm)} — the
    iterate the solve would have returned with itmax = count, for every count of `snapshots` it passed."""
    T = dtype
    b = np.asarray(b, dtype=T)
    n = b.size
    m = 30 if restart <= 0 else int(restart)
    if x0 is not None and Mr is not None:
        raise NotImplementedError("x0 with a right preconditioner")
    left = (lambda v: Ml(v)) if Ml is not None else (lambda v: v)
    right = (lambda v: Mr(v)) if Mr is not None else (lambda v: v)
    x = np.zeros(n, dtype=T) if x0 is None else np.array(x0, dtype=T)

    def residual(xx):
        if defect == "left_not_on_b":
            return b - left(op(xx))
        return left(b - op(xx))

    def dot(u, v, first=False):
        if first and defect == "dot_drops_last_entry":
            return np.dot(u[:-1], v[:-1])
        return np.dot(u, v)

    out = SimpleNamespace(x=x, iters=0, restarts=0, converged=False, failed=False, rnorm0=0.0, rnorm=0.0, residuals=[], snap={})
    if x0 is None:
        r = b.copy() if defect == "left_not_on_b" else left(b)
    elif defect == "x0_ignored_in_r0":
        r = left(b)
    else:
        r = residual(x)
    if defect == "x0_not_added":
        x = np.zeros(n, dtype=T)
    beta = np.sqrt(dot(r, r))
    out.rnorm0 = out.rnorm = beta
    out.residuals.append(beta)
    if fixed_iters > 0:
        tol, cap = T(-1), int(fixed_iters)
    else:
        tol = max(T(atol), T(rtol) * beta) if defect == "tol_is_max" else T(atol) + T(rtol) * beta
        cap = int(itmax) if itmax > 0 else 300
    while True:
        if not np.isfinite(beta):
            out.failed = True
            break
        if beta == 0 or (tol >= 0 and beta <= tol):
            out.converged = True
            break
        V = np.zeros((m + 1, n), dtype=T)
        R = np.zeros((m, m), dtype=T)
        cs, sn, g = np.zeros(m, dtype=T), np.zeros(m, dtype=T), np.zeros(m + 1, dtype=T)
        V[0] = r / beta
        g[0] = beta
        k, done = 0, False

        def iterate(kk):
            if kk == 0:
                return x.copy()
            y = np.zeros(kk, dtype=T)
            for i in range(kk - 1, -1, -1):       # back-substitution
                y[i] = (g[i] - np.dot(R[i, i + 1:kk], y[i + 1:])) / R[i, i]
            return x + right(V[:kk].T @ y)

        while k < m and out.iters < cap:
            w = left(op(right(V[k])))
            h = np.zeros(k + 2, dtype=T)
            for sweep in range(2):                # modified Gram–Schmidt, twice
                for i in range(k + 1):
                    c = dot(V[i], w, first=(i == 0))
                    h[i] += c
                    w = w - c * V[i]
            hn = np.sqrt(np.dot(w, w))
            if defect == "subdiagonal_float32":
                hn = T(np.float32(hn))
            h[k + 1] = hn
            for i in range(k):
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                h[i] = t
            d = np.hypot(h[k], h[k + 1])
            cs[k], sn[k] = (T(1), T(0)) if d == 0 else (h[k] / d, h[k + 1] / d)
            R[:k, k] = h[:k]
            R[k, k] = d
            if defect != "givens_not_applied_to_g":
                g[k + 1] = -sn[k] * g[k]
                g[k] = cs[k] * g[k]
            else:
                g[k + 1] = g[k]
            out.iters += 1
            k += 1
            out.rnorm = abs(g[k])
            out.residuals.append(out.rnorm)
            if out.iters in snapshots:
                out.snap[out.iters] = (iterate(k), out.rnorm)
            if not np.isfinite(out.rnorm) or not np.isfinite(hn):
                out.failed = done = True
                break
            if (tol >= 0 and out.rnorm <= tol) or hn == 0:
                out.converged = done = True
                break
            V[k] = w / hn
        if not out.failed:
            x = iterate(k - 1 if defect == "update_k_minus_1" and k > 1 else k)
        if done or out.iters >= cap:
            break
        out.restarts += 1
        if defect == "restart_reuses_recurrence":   # the direction of the cycle's r₀ with the recurrence norm
            r, beta = r * (out.rnorm / beta), out.rnorm
        else:
            r = residual(x)
            beta = np.sqrt(np.dot(r, r))
            out.rnorm = beta
    out.x = x
    return out


def diag_of(case):
    d = np.zeros(case.n)
    row = np.repeat(np.arange(case.n), np.diff(case.rowptr))
    on = row == case.colind
    d[row[on]] = case.vals[on]
    return d


def jacobi(case, dtype=LD):
    """y = x / diag(A) in `dtype`"""
    d = np.asarray(diag_of(case), dtype=dtype)
    return lambda v: v / d


def chebyshev(op, lmin, lmax, degree, dtype=LD):
    """oracle.reference_restatement.chebyshev_preconditioner in `dtype`: `degree` steps of the Chebyshev iteration for
    A y = v from y = 0 on [lmin, lmax]"""
    T = dtype
    theta, delta = (T(lmax) + T(lmin)) / 2, (T(lmax) - T(lmin)) / 2
    sigma1 = theta / delta

    def M(v):
        rho = 1 / sigma1
        r = np.array(v, dtype=T, copy=True)
        d = r / theta
        y = d.copy()
        for _ in range(1, degree):
            r = r - op(d)
            rho_new = 1 / (2 * sigma1 - rho)
            d = rho_new * rho * d + (2 * rho_new / delta) * r
            y = y + d
            rho = rho_new
        return y
    return M


def real_spectrum_interval(case, shift=0.0):
    """(min, max) of the real parts of the eigenvalues of a small case's matrix (+ shift·I), from numpy's float64 dense
    eigenvalues — the interval only has to be the same on the device and in the reference, not exact"""
    assert case.n <= 600
    ev = np.linalg.eigvals(to_scipy(case).toarray()).real + shift
    return float(ev.min()), float(ev.max())


@functools.lru_cache(maxsize=None)
def _fixed_run(name_key, m):
    """the reference over KMAX steps of a convdiff case with restart m, a snapshot at every count"""
    case = convdiff_n(*name_key)
    return gmres(Operator(case), case.b, restart=m, fixed_iters=KMAX, snapshots=frozenset(range(1, KMAX + 1)))


def supported_steps(n, pe, m):
    """how many steps of the case's GMRES(m) mean something: the residual BEFORE the last step is still above 1e-6·rnorm0 and
    the step is no (near) breakdown — beyond that the Krylov space is exhausted to rounding and the iterates are noise"""
    ref = _fixed_run((n, pe), m)
    k = 0
    while k < KMAX and k < len(ref.residuals) - 1 and ref.residuals[k] > 1e-6 * ref.rnorm0 and k < (n if m >= n else KMAX):
        k += 1
    return k


RESTARTS = (1, 2, 7, 30, 62, 63)
FIXED_N = (63, 65, 99, 4097)


def fixed_counts(n, pe, m):
    """fixed_iters k ∈ {1, 2, m, m+1, 2m+3}, capped at KMAX and at what the case supports"""
    cap = min(KMAX, supported_steps(n, pe, m))
    return sorted({min(k, cap) for k in (1, 2, m, m + 1, 2 * m + 3)})


def fixed_reference(n, pe, m, k):
    """the reference's view of `fixed_iters = k`: a namespace like gmres()'s"""
    ref = _fixed_run((n, pe), m)
    x, rn = ref.snap[k]
    return SimpleNamespace(x=x, iters=k, restarts=(k - 1) // m, converged=False, failed=False, rnorm0=ref.rnorm0, rnorm=rn,
                           residuals=ref.residuals[:k + 1])


# ------------------------------------------------------------------------------------------------------------- tolerances
# (n, pe, m) -> (spread of x, spread of the norms), each rounded up to a power of two: the output of `python tests/gmres_reference.py`
TABLE = {
    (63, 0.5, 1): (2.0 ** -52, 2.0 ** -52),
    (63, 0.5, 2): (2.0 ** -50, 2.0 ** -52),
    (63, 0.5, 7): (2.0 ** -48, 2.0 ** -52),
    (63, 0.5, 30): (2.0 ** -46, 2.0 ** -52),
    (63, 0.5, 62): (2.0 ** -46, 2.0 ** -52),
    (63, 0.5, 63): (2.0 ** -46, 2.0 ** -52),
    (63, 2.0, 1): (2.0 ** -51, 2.0 ** -52),
    (63, 2.0, 2): (2.0 ** -51, 2.0 ** -52),
    (63, 2.0, 7): (2.0 ** -48, 2.0 ** -52),
    (63, 2.0, 30): (2.0 ** -46, 2.0 ** -52),
    (63, 2.0, 62): (2.0 ** -46, 2.0 ** -52),
    (63, 2.0, 63): (2.0 ** -46, 2.0 ** -52),
    (65, 0.5, 1): (2.0 ** -51, 2.0 ** -53),
    (65, 0.5, 2): (2.0 ** -50, 2.0 ** -53),
    (65, 0.5, 7): (2.0 ** -47, 2.0 ** -50),
    (65, 0.5, 30): (2.0 ** -47, 2.0 ** -53),
    (65, 0.5, 62): (2.0 ** -47, 2.0 ** -53),
    (65, 0.5, 63): (2.0 ** -47, 2.0 ** -53),
    (65, 2.0, 1): (2.0 ** -52, 2.0 ** -53),
    (65, 2.0, 2): (2.0 ** -50, 2.0 ** -53),
    (65, 2.0, 7): (2.0 ** -48, 2.0 ** -51),
    (65, 2.0, 30): (2.0 ** -47, 2.0 ** -53),
    (65, 2.0, 62): (2.0 ** -47, 2.0 ** -53),
    (65, 2.0, 63): (2.0 ** -47, 2.0 ** -53),
    (99, 0.5, 1): (2.0 ** -52, 2.0 ** -52),
    (99, 0.5, 2): (2.0 ** -51, 2.0 ** -52),
    (99, 0.5, 7): (2.0 ** -46, 2.0 ** -50),
    (99, 0.5, 30): (2.0 ** -46, 2.0 ** -52),
    (99, 0.5, 62): (2.0 ** -46, 2.0 ** -52),
    (99, 0.5, 63): (2.0 ** -46, 2.0 ** -52),
    (99, 2.0, 1): (2.0 ** -51, 2.0 ** -53),
    (99, 2.0, 2): (2.0 ** -51, 2.0 ** -53),
    (99, 2.0, 7): (2.0 ** -47, 2.0 ** -52),
    (99, 2.0, 30): (2.0 ** -46, 2.0 ** -50),
    (99, 2.0, 62): (2.0 ** -46, 2.0 ** -53),
    (99, 2.0, 63): (2.0 ** -46, 2.0 ** -53),
    (4097, 0.5, 1): (2.0 ** -52, 2.0 ** -53),
    (4097, 0.5, 2): (2.0 ** -51, 2.0 ** -52),
    (4097, 0.5, 7): (2.0 ** -46, 2.0 ** -50),
    (4097, 0.5, 30): (2.0 ** -45, 2.0 ** -50),
    (4097, 0.5, 62): (2.0 ** -45, 2.0 ** -52),
    (4097, 0.5, 63): (2.0 ** -45, 2.0 ** -52),
    (4097, 2.0, 1): (2.0 ** -52, 2.0 ** -53),
    (4097, 2.0, 2): (2.0 ** -51, 2.0 ** -53),
    (4097, 2.0, 7): (2.0 ** -48, 2.0 ** -52),
    (4097, 2.0, 30): (2.0 ** -46, 2.0 ** -49),
    (4097, 2.0, 62): (2.0 ** -45, 2.0 ** -52),
    (4097, 2.0, 63): (2.0 ** -45, 2.0 ** -52),
}
# every other solve of the GPU file, by the name all_specs() gives it: tolerance stops, warm starts, preconditioner sides, shifts,
# the normal form, host callbacks, Chebyshev, the matrix-free Brusselator cases — the spread of the oracle's column and s-step forms (oracle_on_spec)
# on that very solve, rounded up like TABLE's (0.0: every formulation returned the reference's bits; the floor then holds)
GROUP_TABLE = {
    'brus-cheb1-50': (2.0 ** -46, 2.0 ** -51),
    'brus-cheb2-50': (2.0 ** -44, 2.0 ** -48),
    'brus-cheb5-50': (2.0 ** -46, 2.0 ** -49),
    'brus-normal-32': (2.0 ** -42, 2.0 ** -53),
    'brus-normal-50': (2.0 ** -49, 2.0 ** -54),
    'brus-normal-damped0.0-32': (2.0 ** -42, 2.0 ** -53),
    'brus-normal-damped0.0-50': (2.0 ** -49, 2.0 ** -54),
    'brus-normal-damped0.5-32': (2.0 ** -43, 2.0 ** -55),
    'brus-normal-damped0.5-50': (2.0 ** -49, 2.0 ** -54),
    'cheb1-63': (2.0 ** -52, 2.0 ** -54),
    'cheb1-65': (2.0 ** -51, 2.0 ** -53),
    'cheb1-99': (2.0 ** -52, 2.0 ** -55),
    'cheb1-shift-63': (2.0 ** -52, 2.0 ** -55),
    'cheb1-shift-65': (2.0 ** -52, 2.0 ** -53),
    'cheb1-shift-99': (2.0 ** -52, 2.0 ** -56),
    'cheb2-63': (2.0 ** -51, 2.0 ** -54),
    'cheb2-65': (2.0 ** -51, 2.0 ** -53),
    'cheb2-99': (2.0 ** -51, 2.0 ** -56),
    'cheb2-shift-63': (2.0 ** -51, 2.0 ** -55),
    'cheb2-shift-65': (2.0 ** -51, 2.0 ** -53),
    'cheb2-shift-99': (2.0 ** -51, 2.0 ** -56),
    'cheb5-63': (2.0 ** -51, 2.0 ** -55),
    'cheb5-65': (2.0 ** -51, 2.0 ** -53),
    'cheb5-99': (2.0 ** -51, 2.0 ** -56),
    'cheb5-shift-63': (2.0 ** -51, 2.0 ** -55),
    'cheb5-shift-65': (2.0 ** -51, 2.0 ** -53),
    'cheb5-shift-99': (2.0 ** -51, 2.0 ** -56),
    'host-3-left': (2.0 ** -50, 2.0 ** -53),
    'host-3-left+right': (2.0 ** -52, 2.0 ** -53),
    'host-3-none': (2.0 ** -51, 2.0 ** -52),
    'host-3-right': (2.0 ** -51, 2.0 ** -52),
    'host-63-left': (2.0 ** -46, 2.0 ** -49),
    'host-63-left+right': (2.0 ** -47, 2.0 ** -52),
    'host-63-none': (2.0 ** -46, 2.0 ** -48),
    'host-63-right': (2.0 ** -47, 2.0 ** -48),
    'host-65-left': (2.0 ** -49, 2.0 ** -51),
    'host-65-left+right': (2.0 ** -47, 2.0 ** -49),
    'host-65-none': (2.0 ** -48, 2.0 ** -50),
    'host-65-right': (2.0 ** -48, 2.0 ** -50),
    'line-33': (2.0 ** -51, 2.0 ** -54),
    'line-5': (2.0 ** -50, 2.0 ** -54),
    'normal-4097': (2.0 ** -50, 2.0 ** -52),
    'normal-63': (2.0 ** -48, 2.0 ** -51),
    'normal-65': (2.0 ** -50, 2.0 ** -54),
    'normal-99': (2.0 ** -50, 2.0 ** -53),
    'normal-damped0.0-4097': (2.0 ** -50, 2.0 ** -52),
    'normal-damped0.0-63': (2.0 ** -48, 2.0 ** -51),
    'normal-damped0.0-65': (2.0 ** -50, 2.0 ** -54),
    'normal-damped0.0-99': (2.0 ** -50, 2.0 ** -53),
    'normal-damped0.5-4097': (2.0 ** -50, 2.0 ** -52),
    'normal-damped0.5-63': (2.0 ** -49, 2.0 ** -52),
    'normal-damped0.5-65': (2.0 ** -50, 2.0 ** -54),
    'normal-damped0.5-99': (2.0 ** -50, 2.0 ** -53),
    'plain-63': (2.0 ** -46, 2.0 ** -48),
    'prec-both-63-k17': (2.0 ** -47, 2.0 ** -52),
    'prec-both-63-stop': (2.0 ** -51, 2.0 ** -55),
    'prec-both-65-k17': (2.0 ** -47, 2.0 ** -49),
    'prec-both-65-stop': (2.0 ** -52, 2.0 ** -54),
    'prec-both-99-k17': (2.0 ** -49, 2.0 ** -52),
    'prec-both-99-stop': (2.0 ** -52, 2.0 ** -53),
    'prec-left-63-k17': (2.0 ** -46, 2.0 ** -49),
    'prec-left-63-stop': (2.0 ** -51, 2.0 ** -54),
    'prec-left-65-k17': (2.0 ** -48, 2.0 ** -50),
    'prec-left-65-stop': (2.0 ** -52, 2.0 ** -54),
    'prec-left-99-k17': (2.0 ** -50, 2.0 ** -52),
    'prec-left-99-stop': (2.0 ** -52, 2.0 ** -53),
    'prec-right-63-k17': (2.0 ** -47, 2.0 ** -48),
    'prec-right-63-stop': (2.0 ** -51, 2.0 ** -53),
    'prec-right-65-k17': (2.0 ** -47, 2.0 ** -49),
    'prec-right-65-stop': (2.0 ** -52, 2.0 ** -53),
    'prec-right-99-k17': (2.0 ** -50, 2.0 ** -53),
    'prec-right-99-stop': (2.0 ** -52, 2.0 ** -54),
    'shift-0.25-4097': (2.0 ** -44, 2.0 ** -51),
    'shift-0.25-63': (2.0 ** -44, 2.0 ** -46),
    'shift-0.25-65': (2.0 ** -46, 2.0 ** -49),
    'shift-0.25-99': (2.0 ** -48, 2.0 ** -50),
    'shift-0.25-w-4097': (2.0 ** -44, 2.0 ** -50),
    'shift-0.25-w-63': (2.0 ** -41, 2.0 ** -48),
    'shift-0.25-w-65': (2.0 ** -47, 2.0 ** -49),
    'shift-0.25-w-99': (2.0 ** -49, 2.0 ** -52),
    'shift0.75-4097': (2.0 ** -49, 2.0 ** -52),
    'shift0.75-63': (2.0 ** -51, 2.0 ** -53),
    'shift0.75-65': (2.0 ** -50, 2.0 ** -52),
    'shift0.75-99': (2.0 ** -52, 2.0 ** -56),
    'shift0.75-w-4097': (2.0 ** -51, 2.0 ** -53),
    'shift0.75-w-63': (2.0 ** -52, 2.0 ** -55),
    'shift0.75-w-65': (2.0 ** -50, 2.0 ** -51),
    'shift0.75-w-99': (2.0 ** -52, 2.0 ** -56),
    'stop-4097-0.5-30-0': (2.0 ** -50, 2.0 ** -53),
    'stop-4097-0.5-30-1': (2.0 ** -50, 2.0 ** -53),
    'stop-4097-0.5-30-2': (2.0 ** -46, 2.0 ** -52),
    'stop-4097-0.5-30-3': (2.0 ** -48, 2.0 ** -53),
    'stop-4097-0.5-7-0': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-0.5-7-1': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-0.5-7-2': (2.0 ** -49, 2.0 ** -53),
    'stop-4097-0.5-7-3': (2.0 ** -50, 2.0 ** -53),
    'stop-4097-2.0-30-0': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-2.0-30-1': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-2.0-30-2': (2.0 ** -45, 2.0 ** -50),
    'stop-4097-2.0-30-3': (2.0 ** -47, 2.0 ** -51),
    'stop-4097-2.0-7-0': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-2.0-7-1': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-2.0-7-2': (2.0 ** -51, 2.0 ** -53),
    'stop-4097-2.0-7-3': (2.0 ** -51, 2.0 ** -53),
    'stop-63-0.5-30-0': (2.0 ** -44, 2.0 ** -55),
    'stop-63-0.5-30-1': (2.0 ** -51, 2.0 ** -55),
    'stop-63-0.5-30-2': (2.0 ** -44, 2.0 ** -51),
    'stop-63-0.5-30-3': (2.0 ** -44, 2.0 ** -52),
    'stop-63-0.5-7-0': (2.0 ** -52, 2.0 ** -54),
    'stop-63-0.5-7-1': (2.0 ** -51, 2.0 ** -54),
    'stop-63-0.5-7-2': (2.0 ** -46, 2.0 ** -48),
    'stop-63-0.5-7-3': (2.0 ** -47, 2.0 ** -52),
    'stop-63-2.0-30-0': (2.0 ** -45, 2.0 ** -53),
    'stop-63-2.0-30-1': (2.0 ** -50, 2.0 ** -52),
    'stop-63-2.0-30-2': (2.0 ** -45, 2.0 ** -50),
    'stop-63-2.0-30-3': (2.0 ** -45, 2.0 ** -53),
    'stop-63-2.0-7-0': (2.0 ** -51, 2.0 ** -53),
    'stop-63-2.0-7-1': (2.0 ** -51, 2.0 ** -53),
    'stop-63-2.0-7-2': (2.0 ** -49, 2.0 ** -52),
    'stop-63-2.0-7-3': (2.0 ** -50, 2.0 ** -52),
    'stop-99-0.5-30-0': (2.0 ** -44, 2.0 ** -56),
    'stop-99-0.5-30-1': (2.0 ** -52, 2.0 ** -56),
    'stop-99-0.5-30-2': (2.0 ** -44, 2.0 ** -51),
    'stop-99-0.5-30-3': (2.0 ** -44, 2.0 ** -54),
    'stop-99-0.5-7-0': (2.0 ** -52, 2.0 ** -54),
    'stop-99-0.5-7-1': (2.0 ** -52, 2.0 ** -55),
    'stop-99-0.5-7-2': (2.0 ** -48, 2.0 ** -53),
    'stop-99-0.5-7-3': (2.0 ** -50, 2.0 ** -55),
    'stop-99-2.0-30-0': (2.0 ** -47, 2.0 ** -49),
    'stop-99-2.0-30-1': (2.0 ** -52, 2.0 ** -53),
    'stop-99-2.0-30-2': (2.0 ** -44, 2.0 ** -53),
    'stop-99-2.0-30-3': (2.0 ** -44, 2.0 ** -53),
    'stop-99-2.0-7-0': (2.0 ** -52, 2.0 ** -53),
    'stop-99-2.0-7-1': (2.0 ** -52, 2.0 ** -53),
    'stop-99-2.0-7-2': (2.0 ** -50, 2.0 ** -53),
    'stop-99-2.0-7-3': (2.0 ** -51, 2.0 ** -53),
    'warm-63-k17': (2.0 ** -47, 2.0 ** -53),
    'warm-63-stop': (2.0 ** -51, 2.0 ** -55),
    'warm-65-k17': (2.0 ** -42, 2.0 ** -48),
    'warm-65-stop': (2.0 ** -50, 2.0 ** -53),
    'warm-99-k17': (2.0 ** -49, 2.0 ** -52),
    'warm-99-stop': (2.0 ** -52, 2.0 ** -52),
    'warm5-63': (2.0 ** -51, 2.0 ** -51),
    'warm5-65': (2.0 ** -49, 2.0 ** -48),
    'warm5-99': (2.0 ** -52, 2.0 ** -52),
    'zero-rhs-63': (2.0 ** -41, 2.0 ** -51),
}


def pow2_up(v):
    return 0.0 if v <= 0 else 2.0 ** math.ceil(math.log2(v))


def bounds(spread_x, spread_r):
    tx, tr = max(FACTOR * spread_x, FLOOR), max(FACTOR * spread_r, FLOOR)
    assert tx <= LIMIT_X and tr <= LIMIT_R, "badly conditioned for this purpose: lower pe or k, do not loosen the bound"
    return tx, tr


def fixed_bounds(n, pe, m):
    return bounds(*TABLE[(n, pe, m)])


def group_bounds(name):
    return bounds(*GROUP_TABLE[name])


def deviation(x, info, ref):
    """(relative deviation of x, deviation of rnorm and rnorm0 over rnorm0) from the reference"""
    x = np.asarray(x, dtype=LD)
    nx = np.sqrt(np.dot(ref.x, ref.x))
    dx = np.sqrt(np.dot(x - ref.x, x - ref.x)) / nx if nx > 0 else np.sqrt(np.dot(x, x))
    dr = max(abs(LD(info["rnorm"]) - ref.rnorm), abs(LD(info["rnorm0"]) - ref.rnorm0)) / ref.rnorm0
    return float(dx), float(dr)


# ------------------------------------------------------------------------------------------------------------- assertions
def as_info(r):
    """the dict GMRES.solve returns, from an oracle's GmresInfo or a namespace of gmres() above"""
    return dict(iters=int(r.iters), restarts=int(r.restarts), converged=bool(r.converged), failed=bool(r.failed),
                rnorm0=float(r.rnorm0), rnorm=float(r.rnorm))


def check_iterate(x, info, ref, tol_x, tol_r, op=None, b=None, Ml=None):
    """x, rnorm and rnorm0 against the reference's, and (op, b given) the true residual ‖Pl⁻¹(b − A x)‖ of the returned x,
    formed in long double, against the reported rnorm"""
    x = np.asarray(x, dtype=LD)
    assert x.shape == ref.x.shape and np.all(np.isfinite(x)), "x is not finite"
    nx = np.sqrt(np.dot(ref.x, ref.x))
    ex = np.sqrt(np.dot(x - ref.x, x - ref.x))
    assert ex <= tol_x * nx, f"‖x − x_ref‖ = {float(ex):.3e} > {tol_x:.1e}·‖x_ref‖ = {float(tol_x * nx):.3e}"
    r0 = ref.rnorm0
    assert abs(LD(info["rnorm"]) - ref.rnorm) <= tol_r * r0, \
        f"rnorm {info['rnorm']!r} vs {float(ref.rnorm)!r}: off by {float(abs(LD(info['rnorm']) - ref.rnorm) / r0):.3e}·rnorm0"
    assert abs(LD(info["rnorm0"]) - r0) <= tol_r * r0, f"rnorm0 {info['rnorm0']!r} vs {float(r0)!r}"
    if op is not None:
        r = np.asarray(b, dtype=LD) - op(x)
        if Ml is not None:
            r = Ml(r)
        true = np.sqrt(np.dot(r, r))
        assert abs(true - LD(info["rnorm"])) <= tol_r * r0, \
            f"true residual {float(true)!r} vs reported {info['rnorm']!r}: off by {float(abs(true - LD(info['rnorm'])) / r0):.3e}·rnorm0"


def check_counts(info, ref, exact=True, block=0, m=0):
    """converged and failed equal the reference's; iters and restarts too for the column-by-column forms (exact); the s-step
    form (exact = False) may run on by less than its block size, since its stopping test sees whole blocks, and its restarts
    follow from its iters: cycles of m columns, all but the last one completed"""
    assert bool(info["converged"]) == bool(ref.converged), f"converged {info['converged']} vs {ref.converged}"
    assert bool(info["failed"]) == bool(ref.failed), f"failed {info['failed']} vs {ref.failed}"
    if exact:
        assert info["iters"] == ref.iters, f"iters {info['iters']} vs {ref.iters}"
        assert info["restarts"] == ref.restarts, f"restarts {info['restarts']} vs {ref.restarts}"
    else:
        assert ref.iters <= info["iters"] < ref.iters + max(block, 1), f"iters {info['iters']} vs {ref.iters} (block {block})"
        assert m > 0, "the restart length is needed to derive restarts from iters"
        want = max(info["iters"] - 1, 0) // m
        assert info["restarts"] == want, f"restarts {info['restarts']} vs {want} = (iters − 1) // m, iters {info['iters']}, m {m}"


def check_exact(x, x_expected):
    x, x_expected = np.asarray(x, dtype=np.float64), np.asarray(x_expected, dtype=np.float64)
    assert np.array_equal(x, x_expected), f"x differs from the exact answer at {np.flatnonzero(x != x_expected)[:8]}"


def stop_is_decided(ref, tol, margin=1e-6):
    """the reference's residual at the stopping step and at the step before each differ from tol by more than a factor
    1 ± margin: the iteration count is then not a coin toss between two roundings"""
    res = ref.residuals
    at, before = res[ref.iters], res[ref.iters - 1] if ref.iters > 0 else None
    ok = at < tol * (1 - margin) if ref.converged else at > tol * (1 + margin)
    return bool(ok and (before is None or before > tol * (1 + margin)))


# tolerance stops: (atol/‖b‖, rtol)
STOPS = ((0.0, 1e-6), (0.0, 1e-11), (1e-3, 0.0), (1e-4, 1e-4))
STOP_N = (63, 99, 4097)
STOP_M = (7, 30)
STOP_ITMAX = 3000
BRUS_K = 17


@functools.lru_cache(maxsize=None)
def stop_reference(n, pe, m, stop):
    case = convdiff_n(n, pe)
    a, rt = stop
    atol = a * float(np.linalg.norm(case.b))
    return gmres(Operator(case), case.b, atol=atol, rtol=rt, restart=m, itmax=STOP_ITMAX), atol, rt


# ------------------------------------------------------------------------------------------------------------- one solve
def spec(case, m, k=0, atol=0.0, rtol=1e-8, itmax=300, x0=None, left=None, right=None, shift=0.0, weights=None, normal=False,
         damping=None, cheb=None, b=None):
    """One solve, as the GPU file runs it and the reference restates it. left / right: None or "jacobi" (x / diag(A));
    cheb = (degree, lmin, lmax): the Chebyshev right preconditioner on the (shifted) operator; normal: the operator AᵀA
    (+ λ·diag(d), damping = (d, λ)) with the right-hand side Aᵀ b."""
    return SimpleNamespace(case=case, m=m, k=k, atol=atol, rtol=rtol, itmax=itmax, x0=x0, left=left, right=right, shift=shift,
                           weights=weights, normal=normal, damping=damping, cheb=cheb, b=case.b if b is None else b)


def spec_parts(s, dtype=LD, defect=None):
    """(operator, right-hand side, Ml, Mr) of a spec in `dtype`"""
    op = Operator(s.case, s.shift, s.weights, s.normal, s.damping, dtype, defect)
    b = np.asarray(s.b, dtype=dtype)
    if s.normal:   # Aᵀ b, rounded to float64: the vector the device is handed
        b = np.asarray(np.asarray(Operator(s.case, dtype=dtype).AT(b), dtype=np.float64), dtype=dtype)
    Ml = jacobi(s.case, dtype) if s.left == "jacobi" else None
    Mr = jacobi(s.case, dtype) if s.right == "jacobi" else None
    if s.cheb is not None:
        assert Mr is None
        Mr = chebyshev(op, s.cheb[1], s.cheb[2], s.cheb[0], dtype)
    return op, b, Ml, Mr


def solve_spec(s, dtype=LD, defect=None, snapshots=()):
    op, b, Ml, Mr = spec_parts(s, dtype, defect)
    return gmres(op, b, x0=s.x0, atol=s.atol, rtol=s.rtol, restart=s.m, itmax=s.itmax, fixed_iters=s.k, Ml=Ml, Mr=Mr,
                 snapshots=snapshots, dtype=dtype, defect=defect)


def check_spec(x, info, s, ref, tol_x, tol_r):
    """check_iterate with the spec's own operator, right-hand side and left preconditioner for the true residual"""
    op, b, Ml, _ = spec_parts(s)
    check_iterate(x, info, ref, tol_x, tol_r, op=op, b=b, Ml=Ml)


@functools.lru_cache(maxsize=None)
def group_specs():
    """the solves of the GPU file's groups c, e, f, h on the CSR cases, by name (each with m = 7, so that restarts happen)"""
    out = {}
    for n in (63, 65, 99, 4097):
        case = convdiff_n(n, 0.5 if n != 65 else 2.0)
        x0 = rhs(n, "x0")
        small = n < 4096    # n = 4097: shifts and the normal form only
        if small:
            out[f"warm-{n}-k17"] = spec(case, 7, k=17, x0=x0)
            out[f"warm-{n}-stop"] = spec(case, 7, atol=0.0, rtol=1e-6, itmax=STOP_ITMAX, x0=x0)
            for side in ("left", "right", "both"):
                kw = dict(left="jacobi" if side != "right" else None, right="jacobi" if side != "left" else None)
                out[f"prec-{side}-{n}-k17"] = spec(case, 7, k=17, **kw)
                out[f"prec-{side}-{n}-stop"] = spec(case, 7, atol=0.0, rtol=1e-6, itmax=STOP_ITMAX, **kw)
        w, d = positive(n, "shift"), positive(n, "damping")
        for sigma in (0.75, -0.25):
            out[f"shift{sigma}-{n}"] = spec(case, 7, k=17, shift=sigma)
            out[f"shift{sigma}-w-{n}"] = spec(case, 7, k=17, shift=sigma, weights=w)
        out[f"normal-{n}"] = spec(case, 7, k=17, normal=True)
        for lam in (0.0, 0.5):
            out[f"normal-damped{lam}-{n}"] = spec(case, 7, k=17, normal=True, damping=(d, lam))
        if not small:
            continue
        lo, hi = real_spectrum_interval(case)
        for deg in (1, 2, 5):
            out[f"cheb{deg}-{n}"] = spec(case, 7, k=17, cheb=(deg, lo, hi))
            out[f"cheb{deg}-shift-{n}"] = spec(case, 7, k=17, shift=0.75, cheb=(deg, lo + 0.75, hi + 0.75))
        # a warm start from the iterate of a 5-step solve (the GPU file starts from the device's own, equal to rounding)
        x5 = np.asarray(solve_spec(spec(case, 7, k=5)).x, dtype=np.float64)
        out[f"warm5-{n}"] = spec(case, 7, k=17, x0=x5)
    c63 = convdiff_n(63, 0.5)
    out["plain-63"] = spec(c63, 7, k=17)
    # (10 steps: x_ref shrinks with every step while the rounding acts on x0 − x_ref; at 17 steps the s-step formulations' spread
    #  relative to ‖x_ref‖ would put the bound above the project's limit)
    out["zero-rhs-63"] = spec(c63, 7, k=10, x0=rhs(63, "x0"), b=np.zeros(63))
    for n in (5, 33):      # the solve after the s-step fallback on cyclic(n)
        out[f"line-{n}"] = spec(convdiff(n, 1, 0.5), n, k=3)
    for n in (3, 63, 65):  # host callbacks
        m, k = (7, 17) if n > 3 else (3, 2)
        for sides in HOST_SIDES:
            out[f"host-{n}-{'+'.join(sides) or 'none'}"] = spec(convdiff_n(n, 0.5), m, k=k, left="jacobi" if "left" in sides else None,
                                                             right="jacobi" if "right" in sides else None)
    return out


HOST_SIDES = ((), ("right",), ("left",), ("left", "right"))


def stop_name(n, pe, m, i):
    return f"stop-{n}-{pe}-{m}-{i}"


@functools.lru_cache(maxsize=None)
def stop_specs():
    """the tolerance stops of group b as specs, by name"""
    out = {}
    for n in STOP_N:
        for pe in PES:
            case = convdiff_n(n, pe)
            for m in STOP_M:
                for i, (a, rt) in enumerate(STOPS):
                    out[stop_name(n, pe, m, i)] = spec(case, m, atol=a * float(np.linalg.norm(case.b)), rtol=rt, itmax=STOP_ITMAX)
    return out


def brusselator_case(R, N):
    """the Jacobian of the oracle's Brusselator2D(N) at its initial guess as a CSR case (n = 2N²), with a seeded b and the point u"""
    prob = R.Brusselator2D(N)
    u = np.asarray(prob.u0(), dtype=np.float64)
    J = prob.jac(u).tocsr()
    J.sort_indices()
    n = J.shape[0]
    return SimpleNamespace(name=f"brusselator{N}", n=n, rowptr=J.indptr.astype(np.int32), colind=J.indices.astype(np.int32),
                           vals=np.asarray(J.data, dtype=np.float64), b=rhs(n, "brusselator", N), u=u, N=N)


def brusselator_specs(R):
    """the matrix-free solves of groups f and h: the normal form on Brusselator2D(4) and (5), Chebyshev on Brusselator2D(5)"""
    out = {}
    for N in (4, 5):
        case = brusselator_case(R, N)
        d = positive(case.n, "damping")
        out[f"brus-normal-{case.n}"] = spec(case, 7, k=BRUS_K, normal=True)
        for lam in (0.0, 0.5):
            out[f"brus-normal-damped{lam}-{case.n}"] = spec(case, 7, k=BRUS_K, normal=True, damping=(d, lam))
    case = brusselator_case(R, 5)
    lo, hi = real_spectrum_interval(case)
    for deg in (1, 2, 5):
        out[f"brus-cheb{deg}-{case.n}"] = spec(case, 7, k=BRUS_K, cheb=(deg, lo, hi))
    return out


# ------------------------------------------------------------------------------------------------------------- the table
SSTEP_RUNS = ("sstep4", "sstep15n")


def oracle_runs(R, case, m, k):
    """(name, x, info) of every float64 formulation of the oracle on `fixed_iters = k` of a plain CSR case; an s-step
    formulation that raises SStepBreakdown is left out (callers assert that one of them contributes)"""
    A = to_scipy(case)
    mv = lambda z: A @ z   # noqa: E731
    out = []
    for ortho in ("mgs", "cgs2", "dcgs2"):
        out.append((ortho,) + R.gmres(mv, case.b, restart=m, fixed_iters=k, ortho=ortho))
    out.append(("dcgs2_1r",) + R.gmres_dcgs2_1r(mv, case.b, restart=m, fixed_iters=k))
    for name, ortho in zip(SSTEP_RUNS, (("sstep", 4), ("sstep", 15, "newton", R.gershgorin_interval(A)))):
        try:
            out.append((name,) + R.gmres(mv, case.b, restart=m, fixed_iters=k, ortho=ortho))
        except R.SStepBreakdown:
            pass
    return out


def measure_row(R, n, pe, m):
    """(spread of x, spread of the norms), rounded up, and the formulations that contributed, of one row of TABLE"""
    sx = sr = 0.0
    names = set()
    for k in fixed_counts(n, pe, m):
        ref = fixed_reference(n, pe, m, k)
        for name, x, info in oracle_runs(R, convdiff_n(n, pe), m, k):
            dx, dr = deviation(x, as_info(info), ref)
            sx, sr = max(sx, dx), max(sr, dr)
            names.add(name)
    return (pow2_up(sx), pow2_up(sr)), names


def measure_table(R):
    return {(n, pe, m): measure_row(R, n, pe, m)[0] for n in FIXED_N for pe in PES for m in RESTARTS}


def oracle_column_forms(R, mv, b, **kw):
    """the oracle's column forms on one solve; the one-reduction form takes neither x0 nor preconditioners"""
    out = [(o,) + R.gmres(mv, b, ortho=o, **kw) for o in ("mgs", "cgs2", "dcgs2")]
    if kw.get("x0") is None and kw.get("M") is None and kw.get("Ml") is None:
        kw = {k: v for k, v in kw.items() if k not in ("x0", "M", "Ml")}
        out.append(("dcgs2_1r",) + R.gmres_dcgs2_1r(mv, b, **kw))
    return out


def oracle_on_spec(R, s, iters):
    """the oracle's float64 formulations on a spec, with float64 callables for the operator and the preconditioners: the column
    forms as the spec stands, and the s-step forms the device can take on it — monomial blocks of 4 (an explicit block size) and
    6 (the automatic size without spectrum bounds: callbacks, shifts, preconditioners), Newton blocks of 15 on the Gershgorin
    interval where the device has it (a plain CSR operator). The s-step forms run `iters` steps of fixed work, the reference's
    count (their stopping test sees whole blocks); one that raises SStepBreakdown is left out, as the device falls back there."""
    op, b, Ml, Mr = spec_parts(s, dtype=np.float64)
    kw = dict(restart=s.m)
    if s.x0 is not None:
        kw["x0"] = s.x0
    if Ml is not None:
        kw["Ml"] = Ml
    if s.cheb is not None:
        Mr = R.chebyshev_preconditioner(op, s.cheb[1], s.cheb[2], s.cheb[0])
    if Mr is not None:
        kw["M"] = Mr
    out = oracle_column_forms(R, op, b, atol=s.atol, rtol=s.rtol, itmax=s.itmax, fixed_iters=s.k, **kw)
    # (no s-step form where the GPU file runs none: the Chebyshev group runs mgs and dcgs2; the normal form runs with the
    #  automatic choice only, which never takes blocks there — they would square a squared condition number)
    forms = [] if (s.normal or s.cheb is not None) else [("sstep4", ("sstep", 4)), ("sstep6", ("sstep", 6))]
    if not (s.normal or s.shift or Ml is not None or Mr is not None):
        forms.append(("sstep15n", ("sstep", 15, "newton", R.gershgorin_interval(to_scipy(s.case)))))
    for name, ortho in forms:
        if iters <= 0:
            break
        try:
            out.append((name,) + R.gmres(op, b, fixed_iters=iters, ortho=ortho, **kw))
        except R.SStepBreakdown:
            pass
    return out


def all_specs(R):
    return dict(group_specs(), **stop_specs(), **brusselator_specs(R))


def measure_spec(R, s, ref=None):
    ref = solve_spec(s) if ref is None else ref
    sx = sr = 0.0
    for _name, x, info in oracle_on_spec(R, s, ref.iters):
        dx, dr = deviation(x, as_info(info), ref)
        sx, sr = max(sx, dx), max(sr, dr)
    return pow2_up(sx), pow2_up(sr)


def _p2(v):
    return "0.0" if v == 0 else f"2.0 ** {int(math.log2(v))}"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import reference_restatement as R_
    print("TABLE = {")
    for key, (sx_, sr_) in measure_table(R_).items():
        print(f"    {key!r}: ({_p2(sx_)}, {_p2(sr_)}),")
    print("}")
    print("GROUP_TABLE = {")
    for key, s_ in sorted(all_specs(R_).items()):
        sx_, sr_ = measure_spec(R_, s_)
        print(f"    {key!r}: ({_p2(sx_)}, {_p2(sr_)}),")
    print("}")
