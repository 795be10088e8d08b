"""Float32 residual sources for the ensemble tests (the tutorial's element type, nonlinear_solve_gpus.md:146-160), and a
float32 NumPy restatement of SimpleNewtonRaphson / SimpleTrustRegion to check them against.

The sources follow the Float32 contract (`const nk_real *p`, nk_real = float) and are float-clean: every literal is taken
in nk_real, so that the value path never widens to double. The restatement keeps every operation in float32. Its linear
solve is an explicit Gaussian elimination with partial pivoting in float32, the kernel's order of operations:
np.linalg.solve would compute a float32 system in double and round the result."""
import numpy as np

F32 = np.float32
ABSTOL_F32 = float(F32(np.finfo(F32).eps) ** F32(0.8))   # eps(Float32)^(4/5) = 2.8909994e-6 (common_defaults.jl:53)
SUCCESS, MAXITERS, SHRINK_EXCEEDED = 1, 2, 6

# f(u, p) = u .* u .- p (nonlinear_solve_gpus.md:47-62): compiles in both precisions
QUADRATIC = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] * u[i] - p[i];
}
"""

# p2_f of the tutorial (nonlinear_solve_gpus.md:120-127), as it is stated there
P2 = """
template <typename T> __device__ void nk_f(const T *x, const nk_real *p, T *out) {
  out[0] = x[0] + p[0] * x[1];
  out[1] = sqrt(p[1]) * (x[2] - x[3]);
  out[2] = (x[1] - p[2] * x[2]) * (x[1] - p[2] * x[2]);
  out[3] = sqrt(p[3]) * (x[0] - x[3]) * (x[0] - x[3]);
}
"""

# the coupled transcendental system of ensemble_sources.TRIG_WITH_JAC, with its analytic Jacobian, in nk_real
TRIG_WITH_JAC = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  f[0] = exp(u[0]) + u[1] * u[2] - p[0];
  f[1] = sin(u[1]) + u[0] * u[0] - p[1];
  f[2] = u[2] * u[2] * u[2] + tanh(u[0]) - p[2];
}
__device__ void nk_jac(const nk_real *u, const nk_real *p, nk_real *J) {
  J[0] = exp(u[0]);              J[1] = u[2];        J[2] = u[1];
  J[3] = nk_real(2) * u[0];      J[4] = cos(u[1]);   J[5] = nk_real(0);
  const nk_real t = tanh(u[0]);
  J[6] = nk_real(1) - t * t;     J[7] = nk_real(0);  J[8] = nk_real(3) * u[2] * u[2];
}
"""

# a dense coupled residual (every unknown in every equation)
DENSE_COUPLED = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  T s = u[0];
  for (int i = 1; i < NK_N; ++i) s = s + u[i];
  for (int i = 0; i < NK_N; ++i)
    f[i] = u[i] * u[i] - p[i] + (nk_real(0.1) / NK_N) * s + nk_real(0.05) * u[(i + 1) % NK_N] * u[i];
}
"""

# the Float64 contract: a Float32 build must refuse it and name the contract
DOUBLE_CONTRACT = """
template <typename T> __device__ void nk_f(const T *u, const double *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] * u[i] - p[i];
}
"""


# ------------------------------------------------------------------------------------------ float32 twins of the sources
def quadratic_f(u, p):
    return u * u - p


def quadratic_jac(u, p):
    return np.diag(F32(2) * u)


def p2_f(x, p):
    s1, s3 = np.sqrt(p[1]), np.sqrt(p[3])
    return np.array([x[0] + p[0] * x[1], s1 * (x[2] - x[3]), (x[1] - p[2] * x[2]) * (x[1] - p[2] * x[2]),
                     s3 * (x[0] - x[3]) * (x[0] - x[3])], dtype=F32)


def p2_jac(x, p):
    s1, s3 = np.sqrt(p[1]), np.sqrt(p[3])
    d = x[1] - p[2] * x[2]
    e = x[0] - x[3]
    two, z, one = F32(2), F32(0), F32(1)
    return np.array([[one, p[0], z, z], [z, z, s1, -s1], [z, two * d, -two * p[2] * d, z],
                     [two * s3 * e, z, z, -two * s3 * e]], dtype=F32)


def trig_f(u, p):
    return np.array([np.exp(u[0]) + u[1] * u[2] - p[0], np.sin(u[1]) + u[0] * u[0] - p[1],
                     u[2] * u[2] * u[2] + np.tanh(u[0]) - p[2]], dtype=F32)


def trig_jac(u, p):
    t = np.tanh(u[0])
    z = F32(0)
    return np.array([[np.exp(u[0]), u[2], u[1]], [F32(2) * u[0], np.cos(u[1]), z],
                     [F32(1) - t * t, z, F32(3) * u[2] * u[2]]], dtype=F32)


def dense_f(u, p):
    n = u.shape[0]
    s = u[0]
    for i in range(1, n):
        s = s + u[i]
    return u * u - p + (F32(0.1) / F32(n)) * s + F32(0.05) * np.roll(u, -1) * u


def dense_jac(u, p):
    n = u.shape[0]
    J = np.full((n, n), F32(0.1) / F32(n), dtype=F32)
    J[np.arange(n), np.arange(n)] += F32(2) * u + F32(0.05) * np.roll(u, -1)
    J[np.arange(n), (np.arange(n) + 1) % n] += F32(0.05) * u
    return J


# ------------------------------------------------------------------------------------------ float32 restatement
def lu_solve_f32(A, b):
    """A \\ b by Gaussian elimination with partial pivoting, every operation in float32 (first maximum wins)."""
    A = np.array(A, dtype=F32)
    b = np.array(b, dtype=F32)
    n = b.shape[0]
    with np.errstate(all="ignore"):
        for c in range(n):
            piv = c + int(np.argmax(np.abs(A[c:, c])))
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
                b[[c, piv]] = b[[piv, c]]
            inv = F32(1) / A[c, c]
            for r in range(c + 1, n):
                l = A[r, c] * inv
                A[r, c + 1:] -= l * A[c, c + 1:]
                b[r] -= l * b[c]
        dx = np.zeros(n, dtype=F32)
        for r in range(n - 1, -1, -1):
            s = b[r]
            for k in range(r + 1, n):
                s = s - A[r, k] * dx[k]
            dx[r] = s / A[r, r]
    return dx


def _absmax_ok(fx, abstol):
    return (not np.any(np.isnan(fx))) and float(np.max(np.abs(fx))) <= abstol


def simple_newton_raphson_f32(f, jac, u0, p, abstol=None, maxiters=1000):
    """oracle.reference_restatement.simple_newton_raphson with T = Float32 (raphson.jl:39-83): the same loop, every value
    and the default abstol in float32. Returns (x, fx, retcode, iterations)."""
    tol = float(F32(ABSTOL_F32 if abstol is None else abstol))
    p = np.asarray(p, dtype=F32)
    x = np.array(u0, dtype=F32)
    with np.errstate(all="ignore"):
        fx = np.asarray(f(x, p), dtype=F32)
        if not np.any(fx):
            return x, fx, SUCCESS, 0
        J = np.asarray(jac(x, p), dtype=F32)
        for it in range(1, maxiters + 1):
            x = x - lu_solve_f32(J, fx)
            if _absmax_ok(fx, tol):
                return x, fx, SUCCESS, it
            fx = np.asarray(f(x, p), dtype=F32)
            J = np.asarray(jac(x, p), dtype=F32)
    return x, fx, MAXITERS, maxiters


def _norm2(v):
    s = F32(0)
    for a in v:
        s = s + a * a
    return np.sqrt(s)


def _dot(a, b):
    s = F32(0)
    for x, y in zip(a, b):
        s = s + x * y
    return s


def _matvec(M, v):
    return np.array([_dot(row, v) for row in M], dtype=F32)


def simple_trust_region_f32(f, jac, u0, p, abstol=None, maxiters=1000, step_threshold=1e-4, shrink_threshold=0.25,
                            expand_threshold=0.75, shrink_factor=0.25, expand_factor=2.0, max_shrink_times=32):
    """oracle.reference_restatement.simple_trust_region with T = Float32 (trust_region.jl:57-229, `η₁ = T(step_threshold)`
    and so on): every constant, sum and norm in float32, summed in the kernel's order. Returns (x, fx, retcode, iterations)."""
    tol = float(F32(ABSTOL_F32 if abstol is None else abstol))
    e1, e2, e3, t1, t2 = (F32(v) for v in (step_threshold, shrink_threshold, expand_threshold, shrink_factor, expand_factor))
    p = np.asarray(p, dtype=F32)
    x = np.array(u0, dtype=F32)
    xo = x.copy()
    with np.errstate(all="ignore"):
        fx = np.asarray(f(x, p), dtype=F32)
        norm_fx = _norm2(fx)
        J = np.asarray(jac(x, p), dtype=F32)
        dmax = max(norm_fx, np.max(x) - np.min(x))
        delta = dmax / F32(11)
        fk = F32(0.5) * norm_fx * norm_fx
        g = _matvec(J.T, fx)
        shrink = 0
        if _absmax_ok(fx, tol):
            return x, fx, SUCCESS, 0
        for it in range(1, maxiters + 1):
            dN = -lu_solve_f32(J, fx)
            if _norm2(dN) <= delta:
                dl = dN
            else:
                dsd = -g
                nsd = _norm2(dsd)
                if nsd >= delta:
                    dl = dsd * (delta / nsd)
                else:
                    q = dN - dsd
                    dNN, dSN, dSS = _dot(q, q), _dot(dsd, q), _dot(dsd, dsd)
                    fact = dSN * dSN - dNN * (dSS - delta * delta)
                    tau = (-dSN + np.sqrt(fact)) / dNN
                    dl = dsd + tau * (dN - dsd)
            x = xo + dl
            fx = np.asarray(f(x, p), dtype=F32)
            nf = _norm2(fx)
            fk1 = nf * nf / F32(2)
            r = (fk1 - fk) / (_dot(dl, g) + _dot(dl, _matvec(J.T, _matvec(J, dl))) / F32(2))
            if r >= e2:
                shrink = 0
            else:
                delta = t1 * delta
                shrink += 1
                if shrink > max_shrink_times:
                    return x, fx, SHRINK_EXCEEDED, it
            if r >= e1:
                if _absmax_ok(fx, tol):
                    return x, fx, SUCCESS, it
                xo = x.copy()
                J = np.asarray(jac(x, p), dtype=F32)
                if r > e3:
                    delta = min(t2 * delta, dmax)
                fk = fk1
                g = _matvec(J.T, fx)
    return x, fx, MAXITERS, maxiters


def ensemble_f32(solver, f, jac, u0, P, **kw):
    """the restatement over an ensemble: (x, fx, retcode, iterations) stacked over the systems"""
    u0 = np.asarray(u0, dtype=F32)
    out = [solver(f, jac, u0 if u0.ndim == 1 else u0[b], P[b], **kw) for b in range(P.shape[0])]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))

