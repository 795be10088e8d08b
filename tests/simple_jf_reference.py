"""NumPy restatement of the Jacobian-free ensemble methods of lib/SimpleNonlinearSolve — SimpleBroyden (broyden.jl:31-108,
linesearch = nothing), SimpleKlement (klement.jl:9-56) and SimpleDFSane (dfsane.jl:66-172, η_k = f₁/k²) — in float64 or
float32, with the residual sources and NumPy twins that the ensemble tests use.

Every solver works on a whole ensemble at once: row b holds the state of system b, each row follows its own control flow
through masks, and every sum is an explicit loop in the kernels' order of operations (csrc/nk_batch.hip, k_kernel_jf).
Elementwise NumPy arithmetic rounds each operation on its own, as the kernels do under -ffp-contract=off, and a float32 row
stays in float32 throughout. The solvers return (u, resid, retcode, iters, info); info records the rare branches per system:
Klement's resets of J, DFSane's inner line-search passes and line searches cut short by maxiters, and DFSane's first trial
point."""
import numpy as np

SUCCESS, MAXITERS = 1, 2
F32 = np.float32
ABSTOL_F64 = float(np.finfo(float).eps) ** 0.8                  # eps(Float64)^(4/5) (common_defaults.jl:39-48)
ABSTOL_F32 = float(F32(np.finfo(F32).eps) ** F32(0.8))          # eps(Float32)^(4/5) = 2.8909994e-6

# ------------------------------------------------------------------------------------------ residual sources (nk_real)
# All compile in both precisions. Those built from + − × ÷ and sqrt alone are reproduced bit for bit by their twins.
QUADRATIC = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] * u[i] - p[i];
}
"""

# p2_f of the tutorial (nonlinear_solve_gpus.md:120-127)
P2 = """
template <typename T> __device__ void nk_f(const T *x, const nk_real *p, T *out) {
  out[0] = x[0] + p[0] * x[1];
  out[1] = sqrt(p[1]) * (x[2] - x[3]);
  out[2] = (x[1] - p[2] * x[2]) * (x[1] - p[2] * x[2]);
  out[3] = sqrt(p[3]) * (x[0] - x[3]) * (x[0] - x[3]);
}
"""

# every unknown in every equation
DENSE_COUPLED = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  T s = u[0];
  for (int i = 1; i < NK_N; ++i) s = s + u[i];
  for (int i = 0; i < NK_N; ++i)
    f[i] = u[i] * u[i] - p[i] + (nk_real(0.1) / NK_N) * s + nk_real(0.05) * u[(i + 1) % NK_N] * u[i];
}
"""

# newton_fails of the reference's tests (setup_rootfindtestsnippet.jl:12-28), componentwise over NK_N unknowns, minus p
NEWTON_FAILS = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) {
    const T a = nk_real(0.21640425613334457) + nk_real(216.40425613334457) / (nk_real(1) + nk_real(0.0006250000000000001) * (u[i] * u[i]));
    const T b = nk_real(0.21640425613334457) + nk_real(216.40425613334457) / (nk_real(1) + a * a);
    f[i] = nk_real(0.010000000000000002) + nk_real(10.000000000000002) / (nk_real(1) + b * b) - nk_real(0.0011552453009332421) * u[i] - p[i];
  }
}
"""

# flat (f = −1) left of 0, u² − p right of it: on the flat part Klement's J collapses to exactly 0 and is reset to ones
FLAT_THEN_QUADRATIC = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  for (int i = 0; i < NK_N; ++i) f[i] = u[i] < nk_real(0) ? T(nk_real(-1)) : u[i] * u[i] - p[i];
}
"""

# a coupled transcendental system (libm on the device, NumPy's on the host: the roots agree, the trajectories need not)
TRIG = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  f[0] = exp(u[0]) + u[1] * u[2] - p[0];
  f[1] = sin(u[1]) + u[0] * u[0] - p[1];
  f[2] = u[2] * u[2] * u[2] + tanh(u[0]) - p[2];
}
"""


# ------------------------------------------------------------------------------------------ twins: one row per system
def quadratic_f(u, p):
    return u * u - p


def p2_f(x, p):
    out = np.empty_like(x)
    out[:, 0] = x[:, 0] + p[:, 0] * x[:, 1]
    out[:, 1] = np.sqrt(p[:, 1]) * (x[:, 2] - x[:, 3])
    d = x[:, 1] - p[:, 2] * x[:, 2]
    out[:, 2] = d * d
    e = x[:, 0] - x[:, 3]
    out[:, 3] = np.sqrt(p[:, 3]) * e * e
    return out


def dense_f(u, p):
    T = u.dtype.type
    n = u.shape[1]
    s = u[:, 0].copy()
    for i in range(1, n):
        s = s + u[:, i]
    c = T(0.1) / T(n)
    return u * u - p + (c * s)[:, None] + T(0.05) * np.roll(u, -1, axis=1) * u


def newton_fails_f(u, p):
    T = u.dtype.type
    a = T(0.21640425613334457) + T(216.40425613334457) / (T(1) + T(0.0006250000000000001) * (u * u))
    b = T(0.21640425613334457) + T(216.40425613334457) / (T(1) + a * a)
    return T(0.010000000000000002) + T(10.000000000000002) / (T(1) + b * b) - T(0.0011552453009332421) * u - p


def flat_then_quadratic_f(u, p):
    T = u.dtype.type
    return np.where(u < T(0), T(-1), u * u - p).astype(T, copy=False)


def trig_f(u, p):
    return np.stack([np.exp(u[:, 0]) + u[:, 1] * u[:, 2] - p[:, 0], np.sin(u[:, 1]) + u[:, 0] * u[:, 0] - p[:, 1],
                     u[:, 2] * u[:, 2] * u[:, 2] + np.tanh(u[:, 0]) - p[:, 2]], axis=1).astype(u.dtype, copy=False)


# ------------------------------------------------------------------------------------------ shared pieces
def _setup(u0, p, dtype, abstol):
    T = np.dtype(dtype).type
    p = np.asarray(p, dtype=T)
    if p.ndim == 1:
        p = p[None, :]
    u0 = np.asarray(u0, dtype=T)
    if u0.ndim == 0:
        u0 = u0[None]
    x = np.array(np.broadcast_to(u0, (p.shape[0], u0.shape[-1])), dtype=T)
    tol = (ABSTOL_F32 if T is F32 else ABSTOL_F64) if abstol is None or abstol <= 0 else abstol
    return T, x, p, float(T(tol))


def _eval(f, x, p, T):
    return np.asarray(f(x, p), dtype=T).reshape(x.shape)


def _norm2(v, T):
    s = np.zeros(v.shape[0], dtype=T)
    for i in range(v.shape[1]):
        s = s + v[:, i] * v[:, i]
    return np.sqrt(s)


def _absmax_ok(fx, tol):
    """AbsNormTerminationMode(maximum∘abs); NaN never terminates"""
    return ~np.isnan(fx).any(axis=1) & (np.abs(fx).max(axis=1) <= tol)


def _jl_max(a, b):
    """Julia's max on floats: NaN propagates"""
    return np.where(np.isnan(a), a, np.where((b > a) | np.isnan(b), b, a))


def _jl_clamp(x, lo, hi):
    """Julia's clamp: x > hi ? hi : x < lo ? lo : x (NaN stays NaN)"""
    return np.where(x > hi, hi, np.where(x < lo, lo, x))


def _jl_sign(x):
    one = x.dtype.type(1)
    return np.where(x > 0, one, np.where(x < 0, -one, x))


def _upd(mask, new, old):
    return np.where(mask.reshape(mask.shape + (1,) * (old.ndim - 1)), new, old)


# ------------------------------------------------------------------------------------------ SimpleBroyden
def simple_broyden(f, u0, p, abstol=None, maxiters=1000, alpha=None, dtype=np.float64):
    """iszero(f(u0)) ⇒ Success after 0 steps; J⁻¹ = init_α·I; per iteration δx = −J⁻¹f_prev, x += δx, f, check,
    J⁻¹ += ((δx − J⁻¹δf)/(δx·J⁻¹δf)) (J⁻¹ᵀδx)ᵀ. iters: the iteration that passed the check, or maxiters."""
    T, x, p, tol = _setup(u0, p, dtype, abstol)
    nb, n = x.shape
    rc = np.full(nb, MAXITERS, dtype=np.int32)
    iters = np.full(nb, maxiters, dtype=np.int32)
    with np.errstate(all="ignore"):
        fx = _eval(f, x, p, T)
        act = np.any(fx != 0, axis=1)
        rc[~act], iters[~act] = SUCCESS, 0
        if alpha is None or alpha <= 0:
            # Julia compares fx_norm ≥ 1.0e-5 in Float64: for a float32 norm, ≥ the smallest float32 ≥ 1e-5
            thresh = np.nextafter(F32(1e-5), F32(1)) if T is F32 else T(1e-5)
            fn, xn = _norm2(fx, T), _norm2(x, T)
            init_a = np.where(fn >= thresh, _jl_max(xn, T(1)) / (T(2) * fn), T(1)).astype(T)
        else:
            init_a = np.full(nb, T(1.0 / alpha), dtype=T)     # inv(alpha), taken in double
        Ji = np.zeros((nb, n, n), dtype=T)
        for i in range(n):
            Ji[:, i, i] = init_a
        fprev = fx.copy()
        for it in range(1, maxiters + 1):
            if not act.any():
                break
            s = np.zeros((nb, n), dtype=T)
            for k in range(n):
                s = s + Ji[:, :, k] * fprev[:, k:k + 1]
            dx = -s
            x = _upd(act, x + dx, x)
            fx = _upd(act, _eval(f, x, p, T), fx)
            ok = act & _absmax_ok(fx, tol)
            rc[ok], iters[ok] = SUCCESS, it
            act &= ~ok
            df = fx - fprev
            t = np.zeros((nb, n), dtype=T)
            for k in range(n):
                t = t + Ji[:, :, k] * df[:, k:k + 1]
            d = np.zeros(nb, dtype=T)
            for i in range(n):
                d = d + dx[:, i] * t[:, i]
            xJ = np.zeros((nb, n), dtype=T)
            for i in range(n):
                xJ = xJ + Ji[:, i, :] * dx[:, i:i + 1]
            w = (dx - t) / d[:, None]
            Ji = _upd(act, Ji + w[:, :, None] * xJ[:, None, :], Ji)
            fprev = _upd(act, fx, fprev)
    return x, fx, rc, iters, {}


# ------------------------------------------------------------------------------------------ SimpleKlement
def simple_klement(f, u0, p, abstol=None, maxiters=1000, dtype=np.float64):
    """J = ones, reset to ones whenever any entry is 0; δx = f_prev ./ J, x −= δx, f, check,
    J += (f − f_prev − J·δ)/(δ²J² or 1e-5 where that is 0)·δ·J² with δ = −δx. iters as for Broyden."""
    T, x, p, tol = _setup(u0, p, dtype, abstol)
    nb, n = x.shape
    rc = np.full(nb, MAXITERS, dtype=np.int32)
    iters = np.full(nb, maxiters, dtype=np.int32)
    resets = np.zeros(nb, dtype=np.int64)
    with np.errstate(all="ignore"):
        fx = _eval(f, x, p, T)
        fprev = fx.copy()
        J = np.ones((nb, n), dtype=T)
        act = np.ones(nb, dtype=bool)
        for it in range(1, maxiters + 1):
            if not act.any():
                break
            z = act & np.any(J == 0, axis=1)
            resets += z
            J = _upd(z, np.ones_like(J), J)
            dx = fprev / J
            x = _upd(act, x - dx, x)
            fx = _upd(act, _eval(f, x, p, T), fx)
            ok = act & _absmax_ok(fx, tol)
            rc[ok], iters[ok] = SUCCESS, it
            act &= ~ok
            d = -dx
            j2 = J * J
            d2 = (d * d) * j2
            den = np.where(d2 == 0, T(1.0e-5), d2)
            J = _upd(act, J + (((fx - fprev) - J * d) / den) * d * j2, J)
            fprev = _upd(act, fx, fprev)
    return x, fx, rc, iters, {"resets": resets}


# ------------------------------------------------------------------------------------------ SimpleDFSane
def simple_dfsane(f, u0, p, abstol=None, maxiters=1000, sigma_min=1e-10, sigma_max=1e10, sigma_1=1.0, M=10, gamma=1e-4,
                  tau_min=0.1, tau_max=0.5, n_exp=2, dtype=np.float64):
    """The reference's counter k counts outer iterations and inner line-search passes; both loops run while k < maxiters
    (the last trial point is then taken and checked), and the merit value goes to slot mod1(k, M) after the inner
    increments. iters = min(k + 1, maxiters) on Success (the iteration that passed the check), maxiters otherwise.
    Unlike the C ABI, any σ₁ is taken as given (0 and NaN included)."""
    assert 1 <= M <= 32 and n_exp in (1, 2)
    T, x, p, tol = _setup(u0, p, dtype, abstol)
    nb, n = x.shape
    smin, smax, gam, tmin, tmax = (T(v) for v in (sigma_min, sigma_max, gamma, tau_min, tau_max))
    rc = np.full(nb, MAXITERS, dtype=np.int32)
    iters = np.full(nb, maxiters, dtype=np.int32)
    info = {"inner_passes": np.zeros(nb, dtype=np.int64), "exhausted": np.zeros(nb, dtype=np.int64), "first_trial": None}

    def merit(fv):
        s = _norm2(fv, T)
        return s if n_exp == 1 else s * s

    with np.errstate(all="ignore"):
        fx = _eval(f, x, p, T)
        fn = merit(fx)
        f1 = fn.copy()
        hist = np.repeat(fn[:, None], M, axis=1)
        fp = fx.copy()
        xc = x.copy()
        sk = np.full(nb, T(sigma_1), dtype=T)
        k = np.zeros(nb, dtype=np.int64)
        act = k < maxiters
        while act.any():
            sk = _upd(act, _jl_sign(sk) * _jl_clamp(np.abs(sk), smin, smax), sk)
            ms = -sk
            k1 = k + 1
            eta = f1 / (k1 * k1).astype(T)
            fbe = np.max(hist, axis=1) + eta                  # maximum propagates NaN
            ap = np.ones(nb, dtype=T)
            am = np.ones(nb, dtype=T)
            xc = _upd(act, x + ap[:, None] * (ms[:, None] * fp), xc)
            fx = _upd(act, _eval(f, xc, p, T), fx)
            if info["first_trial"] is None:
                info["first_trial"] = xc.copy()
            fnew = merit(fx)
            inn = act.copy()
            while True:
                inn &= k < maxiters
                inn &= ~(fnew <= fbe - gam * (ap * ap) * fn)
                if not inn.any():
                    break
                atp = (ap * ap) * fn / (fnew + (T(2) * ap - T(1)) * fn)
                xc = _upd(inn, x - am[:, None] * (ms[:, None] * fp), xc)
                fx = _upd(inn, _eval(f, xc, p, T), fx)
                fnew = _upd(inn, merit(fx), fnew)
                go = inn & ~(fnew <= fbe - gam * (am * am) * fn)
                atm = (am * am) * fn / (fnew + (T(2) * am - T(1)) * fn)
                ap = _upd(go, _jl_clamp(atp, tmin * ap, tmax * ap), ap)
                am = _upd(go, _jl_clamp(atm, tmin * am, tmax * am), am)
                xc = _upd(go, x + ap[:, None] * (ms[:, None] * fp), xc)
                fx = _upd(go, _eval(f, xc, p, T), fx)
                fnew = _upd(go, merit(fx), fnew)
                k += go
                info["inner_passes"] += go
                inn = go
            info["exhausted"] += act & (k >= maxiters)
            ok = act & _absmax_ok(fx, tol)
            x = _upd(ok, xc, x)
            rc[ok] = SUCCESS
            iters[ok] = np.minimum(k[ok] + 1, maxiters)
            act &= ~ok
            sxx = np.zeros(nb, dtype=T)
            sxf = np.zeros(nb, dtype=T)
            for i in range(n):
                dxi, dfi = xc[:, i] - x[:, i], fx[:, i] - fp[:, i]
                sxx = sxx + dxi * dxi
                sxf = sxf + dxi * dfi
            sk = _upd(act, sxx / sxf, sk)
            x = _upd(act, xc, x)
            fp = _upd(act, fx, fp)
            fn = _upd(act, fnew, fn)
            rows = np.flatnonzero(act)
            hist[rows, (k[rows] + M - 1) % M] = fnew[rows]     # mod1(k, M), 0-based
            k += act
            act &= k < maxiters
    return x, fx, rc, iters, info


SOLVERS = {"SimpleBroyden": simple_broyden, "SimpleKlement": simple_klement, "SimpleDFSane": simple_dfsane}
