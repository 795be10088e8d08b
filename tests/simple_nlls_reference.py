"""NumPy restatement of the least-squares ensemble kernels (csrc/nk_batch.hip, k_kernel_nlls) — SimpleGaussNewton
(lib/SimpleNonlinearSolve/src/raphson.jl:52-81 on a NonlinearLeastSquaresProblem) and SimpleTrustRegion
(trust_region.jl:60-229, default update rule) with m residuals and n ≤ m unknowns — in float32, float64 or long double,
with the residual sources, their NumPy twins, the families and the bounds that the ensemble tests use.

Every solver works on a whole ensemble at once: row b holds problem b, each row follows its own control flow through masks,
and every sum is an explicit loop in the kernels' order of operations: the column-pivoted Householder QR (column norms
recomputed at every step, first largest wins, reflector beta = −sign(alpha)‖x‖, rank threshold m·eps·|r_11|), the dogleg and
the 2-norm termination. Elementwise NumPy arithmetic rounds each operation on its own, as the kernels do under
-ffp-contract=off. Jacobians come from `Dual`, which restates the kernels' dual-number operators one for one, so a twin is
written once and serves for values and for partials. Where a residual uses only + − × ÷ and sqrt the restatement performs
the device's operations exactly; exp and cos come from different libms.

The solvers return (u, resid, retcode, iters, info). info["pass_norm"] is the residual norm that passed the termination
check and info["fail_norm"] the last one that failed it (NaN where there is none): the two norms that decided the
iteration count.

BOUNDS are the device bounds on ‖u − u_restatement‖∞ / ‖u_restatement‖∞ per problem. The yardstick is this restatement
run in long double: for every family, dtype and method the maximum deviation of the working-precision run's final u from the
long-double run's, times MARGIN = 8, rounded up to a power of two (the convention of bcr_reference.py). The factor 8 leaves
room for the device's libm and for sums the compiler may legitimately reassociate nowhere (-ffp-contract=off, no fast-math),
without letting a wrong reflector through. tests/test_simple_nlls_reference.py recomputes the maxima on every run and pins
restatement ≤ bound / 4."""
import numpy as np

SUCCESS, MAXITERS, SHRINK = 1, 2, 6
F32, F64, LD = np.float32, np.float64, np.longdouble
ABSTOL_F64 = float(np.finfo(float).eps) ** 0.8                  # eps(Float64)^(4/5) (common_defaults.jl:39-48)
ABSTOL_F32 = float(F32(np.finfo(F32).eps) ** F32(0.8))          # eps(Float32)^(4/5) = 2.8909994e-6
MARGIN = 8

# ------------------------------------------------------------------------------------------ residual sources (nk_real)
# least_squares_tests__item1.jl: θ₁·exp(θ₂x)·cos(θ₃x + θ₄) at x = −1, −0.5, 0, 0.5, 1; the targets y travel in p
EXPCOS = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) {
    const nk_real x = nk_real(-1) + nk_real(0.5) * nk_real(i);
    f[i] = u[0] * exp(u[1] * x) * cos(u[2] * x + u[3]) - p[i];
  }
}
"""

# Michaelis–Menten a·x/(b + x); p holds (x_i, y_i) pairs
MICHAELIS_MENTEN = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) f[i] = u[0] * p[2 * i] / (u[1] + p[2 * i]) - p[2 * i + 1];
}
"""

# (a + b·x)/(1 + c·x); p holds (x_i, y_i) pairs
RATIONAL = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) f[i] = (u[0] + u[1] * p[2 * i]) / (nk_real(1) + u[2] * p[2 * i]) - p[2 * i + 1];
}
"""

# (u0 + u1·x + u2·x²)² with its Jacobian supplied; p holds (x_i, y_i) pairs
POLY_SQUARED = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) {
    const nk_real x = p[2 * i];
    const T q = u[0] + u[1] * x + u[2] * (x * x);
    f[i] = q * q - p[2 * i + 1];
  }
}
__device__ void nk_jac(const nk_real *u, const nk_real *p, nk_real *J) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) {
    const nk_real x = p[2 * i];
    const nk_real q = u[0] + u[1] * x + u[2] * (x * x);
    J[i * NK_N + 0] = nk_real(2) * q;
    J[i * NK_N + 1] = nk_real(2) * q * x;
    J[i * NK_N + 2] = nk_real(2) * q * (x * x);
  }
}
"""

# n squares and m − n products of neighbours: any n, m = 2n (the shape used above n = 8)
SQUARES_AND_PRODUCTS = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] * u[i] - p[i];
  for (int i = NK_N; i < NK_M; ++i) f[i] = u[i - NK_N] * u[(i - NK_N + 1) % NK_N] - p[i];
}
"""

# (u0 + u1)·x: two identical Jacobian columns, rank 1 whatever u is; p holds (x_i, y_i) pairs
RANK_DEFICIENT = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
#pragma unroll
  for (int i = 0; i < NK_M; ++i) f[i] = (u[0] + u[1]) * p[2 * i] - p[2 * i + 1];
}
"""

# written for n outputs only: with m > n the other residuals stay zero
N_OUTPUTS_ONLY = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] * u[i] - p[i];
}
"""


# ------------------------------------------------------------------------------------------ dual numbers, as the prelude
def _col(a):
    return a[:, None] if isinstance(a, np.ndarray) and a.ndim == 1 else a


class Dual:
    """v: (nb,), d: (nb, ch): the operators of csrc/nk_batch.hip's `struct Dual`, operation for operation"""
    __array_priority__ = 100

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def _is(x):
        return isinstance(x, Dual)

    def __add__(self, b):
        return Dual(self.v + b.v, self.d + b.d) if Dual._is(b) else Dual(self.v + b, self.d)

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __sub__(self, b):
        return Dual(self.v - b.v, self.d - b.d) if Dual._is(b) else Dual(self.v - b, self.d)

    def __rsub__(self, b):          # scalar − dual: r = −a; r.v += b
        return Dual(-self.v + b, -self.d)

    def __mul__(self, b):
        if Dual._is(b):
            return Dual(self.v * b.v, self.d * _col(b.v) + _col(self.v) * b.d)
        return Dual(self.v * b, self.d * _col(b))

    __rmul__ = __mul__

    def __truediv__(self, b):
        if Dual._is(b):
            ib = self.v.dtype.type(1) / b.v
            v = self.v * ib
            return Dual(v, (self.d - _col(v) * b.d) * _col(ib))
        return self * (self.v.dtype.type(1) / b)      # a * (1 / b)

    def __rtruediv__(self, b):      # scalar / dual: Dual(b) / a
        ib = self.v.dtype.type(1) / self.v
        v = b * ib
        return Dual(v, (np.zeros_like(self.d) - _col(v) * self.d) * _col(ib))


def _chain(a, fv, dfv):
    return Dual(fv, _col(dfv) * a.d)


def exp(a):
    if Dual._is(a):
        e = np.exp(a.v)
        return _chain(a, e, e)
    return np.exp(a)


def cos(a):
    return _chain(a, np.cos(a.v), -np.sin(a.v)) if Dual._is(a) else np.cos(a)


def sqrt(a):
    if Dual._is(a):
        s = np.sqrt(a.v)
        return _chain(a, s, a.v.dtype.type(0.5) / s)
    return np.sqrt(a)


def _T(u):
    return (u[0].v if Dual._is(u[0]) else u[0]).dtype.type


# ------------------------------------------------------------------------------------------ twins: u is a list of n columns
# (arrays or Duals), p the (nb, nparams) parameters; each returns the list of m residual columns
def expcos_f(u, p):
    T = _T(u)
    out = []
    for i in range(5):
        x = T(-1) + T(0.5) * T(i)
        out.append(u[0] * exp(u[1] * x) * cos(u[2] * x + u[3]) - p[:, i])
    return out


def michaelis_menten_f(u, p):
    return [u[0] * p[:, 2 * i] / (u[1] + p[:, 2 * i]) - p[:, 2 * i + 1] for i in range(p.shape[1] // 2)]


def rational_f(u, p):
    T = _T(u)
    return [(u[0] + u[1] * p[:, 2 * i]) / (T(1) + u[2] * p[:, 2 * i]) - p[:, 2 * i + 1] for i in range(p.shape[1] // 2)]


def poly_squared_f(u, p):
    out = []
    for i in range(p.shape[1] // 2):
        x = p[:, 2 * i]
        q = u[0] + u[1] * x + u[2] * (x * x)
        out.append(q * q - p[:, 2 * i + 1])
    return out


def poly_squared_jac(x, p):
    """nk_jac of POLY_SQUARED: (nb, m, 3)"""
    T = x.dtype.type
    m = p.shape[1] // 2
    J = np.empty((x.shape[0], m, 3), dtype=T)
    for i in range(m):
        xi = p[:, 2 * i]
        q = x[:, 0] + x[:, 1] * xi + x[:, 2] * (xi * xi)
        J[:, i, 0] = T(2) * q
        J[:, i, 1] = T(2) * q * xi
        J[:, i, 2] = T(2) * q * (xi * xi)
    return J


def squares_and_products_f(u, p):
    n = len(u)
    return [u[i] * u[i] - p[:, i] for i in range(n)] + [u[i] * u[(i + 1) % n] - p[:, n + i] for i in range(n)]


def rank_deficient_f(u, p):
    return [(u[0] + u[1]) * p[:, 2 * i] - p[:, 2 * i + 1] for i in range(p.shape[1] // 2)]


# ------------------------------------------------------------------------------------------ shared pieces
def _setup(u0, p, dtype, abstol):
    T = np.dtype(dtype).type
    p = np.asarray(p, dtype=T)
    if p.ndim == 1:
        p = p[None, :]
    u0 = np.asarray(u0, dtype=T)
    x = np.array(np.broadcast_to(u0, (p.shape[0], u0.shape[-1])), dtype=T)
    if abstol is None or abstol <= 0:
        # eps(T)^(4/5); the long-double yardstick stops where Float64 does, so that the two runs are comparable
        tol = T(ABSTOL_F32) if T is F32 else T(ABSTOL_F64)
    else:
        tol = T(F32(abstol)) if T is F32 else T(abstol)
    return T, x, p, tol


def _eval(f, x, p, m, T):
    out = f([x[:, i] for i in range(x.shape[1])], p)
    assert len(out) == m, (len(out), m)
    return np.stack([np.broadcast_to(np.asarray(c, dtype=T), x.shape[:1]) for c in out], axis=1).astype(T, copy=False)


def _dual_jac(f, x, p, m, T):
    """AutoForwardDiff as nk_jacobian: one seed per unknown (the chunking above n = 8 does not change any value)"""
    nb, n = x.shape
    eye = np.eye(n, dtype=T)
    u = [Dual(x[:, i], np.broadcast_to(eye[i], (nb, n)).copy()) for i in range(n)]
    out = f(u, p)
    J = np.zeros((nb, m, n), dtype=T)
    for i, c in enumerate(out):
        if Dual._is(c):
            J[:, i, :] = c.d
    return J


def _norm2(v, T):
    s = np.zeros(v.shape[0], dtype=T)
    for i in range(v.shape[1]):
        s = s + v[:, i] * v[:, i]
    return np.sqrt(s)


def _upd(mask, new, old):
    return np.where(mask.reshape(mask.shape + (1,) * (old.ndim - 1)), new, old)


# ------------------------------------------------------------------------------------------ pivoted Householder QR
def qr_factor(J):
    """nk_qr_factor: returns (QR, tau, piv); QR holds R in its upper triangle and the reflector vectors below the diagonal"""
    A = np.array(J, copy=True)
    T = A.dtype.type
    nb, m, n = A.shape
    rows = np.arange(nb)
    tau = np.zeros((nb, n), dtype=T)
    piv = np.zeros((nb, n), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(n):
            pv = np.full(nb, k, dtype=np.int64)
            best = None
            for j in range(k, n):
                s = np.zeros(nb, dtype=T)
                for i in range(k, m):
                    s = s + A[:, i, j] * A[:, i, j]
                if j == k:
                    best = s
                else:
                    up = s > best
                    best = np.where(up, s, best)
                    pv = np.where(up, j, pv)
            piv[:, k] = pv
            ck, cp = A[:, :, k].copy(), A[rows, :, pv].copy()
            A[rows, :, pv] = ck
            A[:, :, k] = cp
            alpha = A[:, k, k].copy()
            nrm = np.sqrt(best)
            z = nrm == 0
            beta = np.where(alpha >= 0, -nrm, nrm)
            t = np.where(z, T(0), (beta - alpha) / beta)
            sc = np.where(z, T(0), T(1) / (alpha - beta))
            tau[:, k] = t
            A[:, k, k] = beta
            for i in range(k + 1, m):
                A[:, i, k] = A[:, i, k] * sc
            for j in range(k + 1, n):
                w = A[:, k, j].copy()
                for i in range(k + 1, m):
                    w = w + A[:, i, k] * A[:, i, j]
                w = w * t
                A[:, k, j] = A[:, k, j] - w
                for i in range(k + 1, m):
                    A[:, i, j] = A[:, i, j] - A[:, i, k] * w
    return A, tau, piv


def qr_solve(fac, f):
    """nk_qr_solve: argmin ‖J dx − f‖₂ from the factorisation; columns with |r_kk| ≤ m·eps·|r_11| get 0"""
    A, tau, piv = fac
    T = A.dtype.type
    nb, m, n = A.shape
    rows = np.arange(nb)
    c = np.array(f, copy=True)
    dx = np.zeros((nb, n), dtype=T)
    with np.errstate(all="ignore"):
        for k in range(n):
            w = c[:, k].copy()
            for i in range(k + 1, m):
                w = w + A[:, i, k] * c[:, i]
            w = w * tau[:, k]
            c[:, k] = c[:, k] - w
            for i in range(k + 1, m):
                c[:, i] = c[:, i] - A[:, i, k] * w
        thr = (T(m) * T(np.finfo(T).eps)) * np.abs(A[:, 0, 0])
        for k in range(n - 1, -1, -1):
            s = c[:, k].copy()
            for j in range(k + 1, n):
                s = s - A[:, k, j] * dx[:, j]
            dx[:, k] = np.where(np.abs(A[:, k, k]) <= thr, T(0), s / A[:, k, k])
        for k in range(n - 1, -1, -1):
            pv = piv[:, k]
            a, b = dx[:, k].copy(), dx[rows, pv].copy()
            dx[rows, pv] = a
            dx[:, k] = b
    return dx


def _check_shape(n, m):
    if not 1 <= n <= m <= 64:
        raise ValueError(f"m = {m} residuals for n = {n} unknowns: n <= m <= 64 is required")


def _info(nb, T):
    return {"pass_norm": np.full(nb, np.nan, dtype=T), "fail_norm": np.full(nb, np.nan, dtype=T)}


# ------------------------------------------------------------------------------------------ SimpleGaussNewton
def simple_gauss_newton(f, u0, p, m, abstol=None, maxiters=1000, jac=None, dtype=np.float64):
    """iszero(f(u0)) ⇒ Success after 0 iterations; per iteration δ = J \\ f, u −= δ, ‖f‖₂ ≤ abstol on the residual of the
    previous iterate, then f and J at the new u. iters: the iteration whose check passed, or maxiters."""
    T, x, p, tol = _setup(u0, p, dtype, abstol)
    nb, n = x.shape
    _check_shape(n, m)
    jacf = (lambda xx: np.asarray(jac(xx, p), dtype=T)) if jac is not None else (lambda xx: _dual_jac(f, xx, p, m, T))
    rc = np.full(nb, MAXITERS, dtype=np.int32)
    iters = np.full(nb, maxiters, dtype=np.int32)
    info = _info(nb, T)
    with np.errstate(all="ignore"):
        fx = _eval(f, x, p, m, T)
        act = np.any(fx != 0, axis=1)
        rc[~act], iters[~act] = SUCCESS, 0
        J = jacf(x)
        for it in range(1, maxiters + 1):
            if not act.any():
                break
            dx = qr_solve(qr_factor(J), fx)
            x = _upd(act, x - dx, x)
            nrm = _norm2(fx, T)
            ok = act & (nrm <= tol)
            rc[ok], iters[ok] = SUCCESS, it
            info["pass_norm"][ok] = nrm[ok]
            act &= ~ok
            info["fail_norm"][act] = nrm[act]
            fx = _upd(act, _eval(f, x, p, m, T), fx)
            J = _upd(act, jacf(x), J)
    return x, fx, rc, iters, info


# ------------------------------------------------------------------------------------------ SimpleTrustRegion
def _normal_forms(J, fx, T):
    nb, m, n = J.shape
    H = np.zeros((nb, n, n), dtype=T)
    g = np.zeros((nb, n), dtype=T)
    for i in range(n):
        for j in range(n):
            s = np.zeros(nb, dtype=T)
            for k in range(m):
                s = s + J[:, k, i] * J[:, k, j]
            H[:, i, j] = s
        s = np.zeros(nb, dtype=T)
        for k in range(m):
            s = s + J[:, k, i] * fx[:, k]
        g[:, i] = s
    return H, g


def simple_trust_region(f, u0, p, m, abstol=None, maxiters=1000, step_threshold=1e-4, shrink_threshold=0.25,
                        expand_threshold=0.75, shrink_factor=0.25, expand_factor=2.0, max_shrink_times=32, jac=None,
                        dtype=np.float64):
    """A check before the loop, no iszero shortcut; H = JᵀJ, g = Jᵀf from the unfactored J; dogleg with δN = −(J \\ f);
    r = (f_{k+1} − f_k)/(δ·g + δ·Hδ/2); a rejected trial point leaves its residual in fx (trust_region.jl:146), and the
    next dogleg solves against it with the unchanged factorisation."""
    T, x, p, tol = _setup(u0, p, dtype, abstol)
    nb, n = x.shape
    _check_shape(n, m)
    jacf = (lambda xx: np.asarray(jac(xx, p), dtype=T)) if jac is not None else (lambda xx: _dual_jac(f, xx, p, m, T))
    as_t = (lambda v: T(F32(v))) if T is F32 else T
    eta1, eta2, eta3, t1, t2 = (as_t(v) for v in (step_threshold, shrink_threshold, expand_threshold, shrink_factor,
                                                    expand_factor))
    rc = np.full(nb, MAXITERS, dtype=np.int32)
    iters = np.full(nb, maxiters, dtype=np.int32)
    info = _info(nb, T)
    with np.errstate(all="ignore"):
        xo = x.copy()
        fx = _eval(f, x, p, m, T)
        norm_fx = _norm2(fx, T)
        J = jacf(x)
        xmax, xmin = x[:, 0].copy(), x[:, 0].copy()
        for i in range(1, n):
            xmax = np.where(x[:, i] > xmax, x[:, i], xmax)
            xmin = np.where(x[:, i] < xmin, x[:, i], xmin)
        spread = xmax - xmin
        dmax = np.where(norm_fx > spread, norm_fx, spread)
        delta = dmax / T(11)
        fk = T(0.5) * norm_fx * norm_fx
        H, g = _normal_forms(J, fx, T)
        fac = qr_factor(J)
        act = ~(norm_fx <= tol)
        rc[~act], iters[~act] = SUCCESS, 0
        info["pass_norm"][~act] = norm_fx[~act]
        info["fail_norm"][act] = norm_fx[act]
        shrink = np.zeros(nb, dtype=np.int64)
        for it in range(1, maxiters + 1):
            if not act.any():
                break
            dN = -qr_solve(fac, fx)
            inside = _norm2(dN, T) <= delta
            dsd = -g
            nsd = _norm2(dsd, T)
            cauchy = nsd >= delta
            dl_c = dsd * (delta / nsd)[:, None]
            dNN, dSN, dSS = (np.zeros(nb, dtype=T) for _ in range(3))
            for i in range(n):
                q = dN[:, i] - dsd[:, i]
                dNN = dNN + q * q
                dSN = dSN + dsd[:, i] * q
                dSS = dSS + dsd[:, i] * dsd[:, i]
            fact = dSN * dSN - dNN * (dSS - delta * delta)
            tu = (-dSN + np.sqrt(fact)) / dNN
            dl_b = dsd + tu[:, None] * (dN - dsd)
            dl = np.where(inside[:, None], dN, np.where(cauchy[:, None], dl_c, dl_b))
            x = _upd(act, xo + dl, x)
            fx = _upd(act, _eval(f, x, p, m, T), fx)
            nf = _norm2(fx, T)
            fk1 = nf * nf / T(2)
            dg, dHd = np.zeros(nb, dtype=T), np.zeros(nb, dtype=T)
            for i in range(n):
                s = np.zeros(nb, dtype=T)
                for k in range(n):
                    s = s + H[:, i, k] * dl[:, k]
                dHd = dHd + dl[:, i] * s
                dg = dg + dl[:, i] * g[:, i]
            r = (fk1 - fk) / (dg + dHd / T(2))
            keep = r >= eta2
            shrink = np.where(act & keep, 0, shrink)
            sh = act & ~keep
            delta = np.where(sh, t1 * delta, delta)
            shrink = shrink + sh
            out = sh & (shrink > max_shrink_times)
            rc[out], iters[out] = SHRINK, it
            act &= ~out
            acc = act & (r >= eta1)
            ok = acc & (nf <= tol)
            rc[ok], iters[ok] = SUCCESS, it
            info["pass_norm"][ok] = nf[ok]
            act &= ~ok
            acc &= ~ok
            info["fail_norm"][acc] = nf[acc]
            xo = _upd(acc, x, xo)
            Jn = jacf(x)
            grow = acc & (r > eta3)
            delta = np.where(grow, np.where(t2 * delta < dmax, t2 * delta, dmax), delta)
            fk = np.where(acc, fk1, fk)
            Hn, gn = _normal_forms(Jn, fx, T)
            facn = qr_factor(Jn)
            H, g = _upd(acc, Hn, H), _upd(acc, gn, g)
            fac = tuple(_upd(acc, a, b) for a, b in zip(facn, fac))
    return x, fx, rc, iters, info


SOLVERS = {"SimpleGaussNewton": simple_gauss_newton, "SimpleTrustRegion": simple_trust_region}


# ------------------------------------------------------------------------------------------ families
class Family:
    """source, twin, shape and one committed ensemble (u0 per problem, p) in float64; `transcendental` families may leave
    threshold-straddling problems out of the iteration-count comparison, the others may not"""

    def __init__(self, name, source, f, n, m, u0, p, jac=None, maxiters=1000, transcendental=False, zero_residual=True,
                 abstol32=None):
        self.name, self.source, self.f, self.n, self.m, self.u0, self.p = name, source, f, n, m, u0, p
        self.jac, self.maxiters, self.transcendental, self.zero_residual = jac, maxiters, transcendental, zero_residual
        self.abstol32 = abstol32     # Float32 abstol where the default eps^(4/5) lies below the residual's rounding floor
        self.nparams = p.shape[1]

    def abstol(self, dtype):
        return self.abstol32 if np.dtype(dtype) == np.float32 else None

    def run(self, method, dtype, use_jac=None, **kw):
        jac = self.jac if (use_jac if use_jac is not None else self.jac is not None) else None
        kw.setdefault("maxiters", self.maxiters)
        kw.setdefault("abstol", self.abstol(dtype))
        return SOLVERS[method](self.f, self.u0, self.p, self.m, jac=jac, dtype=dtype, **kw)


EXPCOS_THETA = np.array([1.0, 0.1, 2.0, 0.5])


def _xy(x, y):
    p = np.empty((x.shape[0], 2 * x.shape[1]))
    p[:, 0::2], p[:, 1::2] = x, y
    return p


def _plain(f, u, p):
    return np.stack(f([u[:, i] for i in range(u.shape[1])], p), axis=1)


def expcos_reference_case():
    """the reference's own case: θ_true = (1, 0.1, 2, 0.5), start θ_true + 0.1"""
    y = _plain(expcos_f, EXPCOS_THETA[None, :], np.zeros((1, 5)))
    return Family("expcos_reference", EXPCOS, expcos_f, 4, 5, EXPCOS_THETA[None, :] + 0.1, y, transcendental=True)


def expcos_family(nb=2000, seed=1):
    """θ_true scaled by ±20 %, starts perturbed by up to ±0.4"""
    rng = np.random.default_rng(seed)
    th = EXPCOS_THETA * rng.uniform(0.8, 1.2, (nb, 4))
    y = _plain(expcos_f, th, np.zeros((nb, 5)))
    return Family("expcos", EXPCOS, expcos_f, 4, 5, th + rng.uniform(-0.4, 0.4, (nb, 4)), y, transcendental=True)


def michaelis_menten_family(m, nb=500, noise=0.0, maxiters=1000):
    rng = np.random.default_rng(100 + m)
    ab = np.stack([rng.uniform(1.0, 3.0, nb), rng.uniform(0.5, 2.0, nb)], axis=1)
    x = np.sort(rng.uniform(0.2, 6.0, (nb, m)), axis=1)
    y = ab[:, :1] * x / (ab[:, 1:] + x)
    if noise:
        y = y + noise * rng.standard_normal((nb, m))
    u0 = ab * rng.uniform(0.9, 1.1, (nb, 2))
    name = f"michaelis_menten_{m}" + ("_noisy" if noise else "")
    return Family(name, MICHAELIS_MENTEN, michaelis_menten_f, 2, m, u0, _xy(x, y), maxiters=maxiters, zero_residual=not noise)


def rational_family(m=8, nb=500):
    rng = np.random.default_rng(7)
    abc = np.stack([rng.uniform(0.5, 2.0, nb), rng.uniform(0.5, 2.0, nb), rng.uniform(0.1, 0.5, nb)], axis=1)
    x = np.sort(rng.uniform(0.0, 4.0, (nb, m)), axis=1)
    y = (abc[:, :1] + abc[:, 1:2] * x) / (1.0 + abc[:, 2:] * x)
    return Family("rational", RATIONAL, rational_f, 3, m, abc * rng.uniform(0.97, 1.03, (nb, 3)), _xy(x, y))


def poly_squared_family(m=6, nb=500):
    rng = np.random.default_rng(8)
    c = np.stack([rng.uniform(1.0, 2.0, nb), rng.uniform(0.3, 1.0, nb), rng.uniform(0.1, 0.5, nb)], axis=1)
    x = np.sort(rng.uniform(0.0, 2.0, (nb, m)), axis=1)
    q = c[:, :1] + c[:, 1:2] * x + c[:, 2:] * x * x
    return Family("poly_squared", POLY_SQUARED, poly_squared_f, 3, m, c * rng.uniform(0.9, 1.1, (nb, 3)), _xy(x, q * q),
                  jac=poly_squared_jac, abstol32=1e-4)   # q² − y cannot go below ulp(y) ≈ 1e-6 per residual in Float32


def squares_and_products_family(n, nb=200):
    rng = np.random.default_rng(200 + n)
    ut = rng.uniform(0.8, 2.0, (nb, n))
    p = _plain(squares_and_products_f, ut, np.zeros((nb, 2 * n)))
    return Family(f"squares_and_products_{n}", SQUARES_AND_PRODUCTS, squares_and_products_f, n, 2 * n,
                  ut * rng.uniform(0.9, 1.1, (nb, n)), p)


def rank_deficient_family(m=8, nb=64):
    rng = np.random.default_rng(9)
    x = np.sort(rng.uniform(0.5, 3.0, (nb, m)), axis=1)
    y = 1.7 * x + 0.05 * rng.standard_normal((nb, m))
    return Family("rank_deficient", RANK_DEFICIENT, rank_deficient_f, 2, m, rng.uniform(0.2, 1.0, (nb, 2)), _xy(x, y),
                  maxiters=50, zero_residual=False)


def calibrated_families():
    """every family the device tests hold against BOUNDS"""
    return [expcos_reference_case(), expcos_family(), michaelis_menten_family(8), michaelis_menten_family(16),
            michaelis_menten_family(64, nb=200), rational_family(), poly_squared_family(), squares_and_products_family(4),
            squares_and_products_family(12), michaelis_menten_family(16, noise=0.02, maxiters=20)]


def rel_dev(u, ref):
    """‖u − ref‖∞ / ‖ref‖∞ per problem, in long double"""
    u, ref = np.asarray(u, dtype=LD), np.asarray(ref, dtype=LD)
    return np.max(np.abs(u - ref), axis=1) / np.max(np.abs(ref), axis=1)


def bound_from(maximum):
    """MARGIN × the measured maximum, rounded up to a power of two"""
    return float(2.0 ** np.ceil(np.log2(MARGIN * float(maximum))))


# (family, dtype name, method): device bound on rel_dev(device u, restatement u). The comment carries the restatement's own
# maximum against the long-double run, from which the bound follows by bound_from.
BOUNDS = {
    ("expcos_reference", "float64", "SimpleGaussNewton"): 8.881784197001252e-16,   # 5.561e-17
    ("expcos_reference", "float32", "SimpleGaussNewton"): 2.384185791015625e-07,   # 2.310e-08
    ("expcos_reference", "float64", "SimpleTrustRegion"): 4.440892098500626e-16,   # 4.554e-17
    ("expcos_reference", "float32", "SimpleTrustRegion"): 9.5367431640625e-07,   # 7.153e-08
    ("expcos", "float64", "SimpleGaussNewton"): 3.552713678800501e-15,   # 3.026e-16
    ("expcos", "float32", "SimpleGaussNewton"): 1.9073486328125e-06,   # 1.978e-07
    ("expcos", "float64", "SimpleTrustRegion"): 3.552713678800501e-15,   # 3.741e-16
    ("expcos", "float32", "SimpleTrustRegion"): 3.0517578125e-05,   # 2.946e-06
    ("michaelis_menten_8", "float64", "SimpleGaussNewton"): 7.105427357601002e-15,   # 7.947e-16
    ("michaelis_menten_8", "float32", "SimpleGaussNewton"): 7.62939453125e-06,   # 5.340e-07
    ("michaelis_menten_8", "float64", "SimpleTrustRegion"): 1.4210854715202004e-14,   # 9.733e-16
    ("michaelis_menten_8", "float32", "SimpleTrustRegion"): 0.0001220703125,   # 9.681e-06
    ("michaelis_menten_16", "float64", "SimpleGaussNewton"): 7.105427357601002e-15,   # 5.936e-16
    ("michaelis_menten_16", "float32", "SimpleGaussNewton"): 3.814697265625e-06,   # 2.822e-07
    ("michaelis_menten_16", "float64", "SimpleTrustRegion"): 7.105427357601002e-15,   # 6.105e-16
    ("michaelis_menten_16", "float32", "SimpleTrustRegion"): 6.103515625e-05,   # 4.841e-06
    ("michaelis_menten_64", "float64", "SimpleGaussNewton"): 3.552713678800501e-15,   # 2.948e-16
    ("michaelis_menten_64", "float32", "SimpleGaussNewton"): 1.9073486328125e-06,   # 1.966e-07
    ("michaelis_menten_64", "float64", "SimpleTrustRegion"): 3.552713678800501e-15,   # 2.530e-16
    ("michaelis_menten_64", "float32", "SimpleTrustRegion"): 1.52587890625e-05,   # 1.636e-06
    ("rational", "float64", "SimpleGaussNewton"): 3.637978807091713e-12,   # 3.408e-13
    ("rational", "float32", "SimpleGaussNewton"): 0.0009765625,   # 8.644e-05
    ("rational", "float64", "SimpleTrustRegion"): 3.637978807091713e-12,   # 2.385e-13
    ("rational", "float32", "SimpleTrustRegion"): 0.001953125,   # 2.192e-04
    ("poly_squared", "float64", "SimpleGaussNewton"): 2.2737367544323206e-13,   # 2.280e-14
    ("poly_squared", "float32", "SimpleGaussNewton"): 0.00048828125,   # 3.926e-05
    ("poly_squared", "float64", "SimpleTrustRegion"): 4.547473508864641e-13,   # 4.342e-14
    ("poly_squared", "float32", "SimpleTrustRegion"): 0.000244140625,   # 1.772e-05
    ("squares_and_products_4", "float64", "SimpleGaussNewton"): 4.440892098500626e-16,   # 4.622e-17
    ("squares_and_products_4", "float32", "SimpleGaussNewton"): 9.5367431640625e-07,   # 6.453e-08
    ("squares_and_products_4", "float64", "SimpleTrustRegion"): 1.7763568394002505e-15,   # 1.334e-16
    ("squares_and_products_4", "float32", "SimpleTrustRegion"): 7.62939453125e-06,   # 4.844e-07
    ("squares_and_products_12", "float64", "SimpleGaussNewton"): 4.440892098500626e-16,   # 5.255e-17
    ("squares_and_products_12", "float32", "SimpleGaussNewton"): 9.5367431640625e-07,   # 6.055e-08
    ("squares_and_products_12", "float64", "SimpleTrustRegion"): 8.881784197001252e-16,   # 9.957e-17
    ("squares_and_products_12", "float32", "SimpleTrustRegion"): 3.814697265625e-06,   # 4.402e-07
    ("michaelis_menten_16_noisy", "float64", "SimpleGaussNewton"): 7.105427357601002e-15,   # 5.265e-16
    ("michaelis_menten_16_noisy", "float32", "SimpleGaussNewton"): 3.814697265625e-06,   # 3.340e-07
    ("michaelis_menten_16_noisy", "float64", "SimpleTrustRegion"): 1.1920928955078125e-07,   # 8.107e-09
    ("michaelis_menten_16_noisy", "float32", "SimpleTrustRegion"): 0.001953125,   # 1.872e-04
}
