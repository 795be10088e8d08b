"""NumPy restatement of LimitedMemoryBroyden without a line search (lib/NonlinearSolveQuasiNewton: lbroyden.jl,
initialization.jl:139-298, broyden.jl:129-147, reset_conditions.jl:1-87, solve.jl:296-486; the initial scaling of
NonlinearSolveBase/src/utils.jl:307-314), sequential and literal: three operator products per step (J⁻¹·fu, J⁻¹·dfu, J⁻ᵀ·du),
each written as the reference writes it (coefficients first, then the combination, then the a·x term).

    J⁻¹ = a·I + U Vᵀ over the first min(idx, threshold) columns, a = 1/α,
    α = `alpha`, or 2‖fu‖₂ / max(‖u‖₂, 1), or 1 when ‖fu‖₂ < 1e-5.
    step:   [reset test, every step but the first]  δu = −(J⁻¹ fu);  u += δu;  fu = f(u);  termination check;
    update: dfu = fu − fu_prev;  w = J⁻¹ dfu;  z = J⁻ᵀ δu;  denom = δu·w (1e-5 if exactly 0);
            U[:, mod1(idx+1, threshold)] = (δu − w)/denom;  V[:, same] = z;  idx += 1.

The reset test is NoChangeInStateReset(nsteps = 3) with its own copy of the last residual it looked at: the early return of
its `du` branch leaves that copy one step old, which the restatement keeps. A reset sets idx = 0 and recomputes a from the
current (u, fu); the reset that brings the count to `max_resets` ends the solve with ConvergenceFailure instead of being applied.

`dtype` is the arithmetic (float64 or np.longdouble). The thresholds that steer the control flow — the reset tolerance
eps^(3/4), the 1e-5 of the α rule, abstol — are Float64's in either arithmetic: the long-double run is the same trajectory in
wider arithmetic, and the per-step distance between the two runs is the algorithm's sensitivity to rounding. The termination
check is the part of AbsNormSafeBestTerminationMode(maximum∘abs) a short solve can reach: non-finite → Unstable,
max|fu| ≤ abstol → Success. One divergence from the reference, shared with the library: reinit! there leaves the reset test's
residual copy at the previous solve's value; here a solve always starts with the copy at f(u0).

Step counts at abstol = eps^(4/5) (tests/test_lbroyden_reference.py pins them):

    case                                        threshold  steps  retcode             resets asked for at step
    Quadratic n = 64, u0 = 1, p = 2                 10        6   Success             —
    Quadratic n = 64, u0 = 1, p = 2                  3       11   Success             —   (columns 0 1 2 0 1 2 0 1 2 0: the index wraps)
    Quadratic n = 1000, u0 = linspace(1, 3)         10       12   Success             11  (decided within a factor 2.1 of the tolerance)
    Quadratic n = 1000, u0 = linspace(1, 2.375)     10       15   Success             14  (a factor 10 away: the shared spread case)
    stall n = 64 (constant residuals 0 and 1)       10       10   ConvergenceFailure  4, 7, 10 (the third is not applied)
    Bratu 8² … 64², u0 = 0, threshold 3, 10, 30      —   5 … 100  Unstable; 8² with threshold 30: ConvergenceFailure at step 42
                                                                   (resets at 32, 37, 42) — the method does not solve it

Per-step distance float64 ↔ long double (gaps(name): max|Δu| and max|Δfu| after every step) and the bounds the GPU tests take
from it (bounds(name), never from the device): 16 × the gap of that step, plus a floor of 4 eps × the size of the numbers that
were rounded — max(1, ‖u‖∞) for u; ‖fu‖∞ + 4‖u‖∞ + ‖u‖∞² + 2 for fu, the terms that cancel in the residuals used here. The
table holds the maximum over the steps of each case, measured with x87 long double (64-bit significand):

    case                      max gap u   max gap fu   max bound u  max bound fu
    quadratic64_t10            1.10e-16    2.63e-16      3.02e-15      1.28e-14
    quadratic64_t3             1.51e-16    4.49e-16      3.67e-15      1.58e-14
    quadratic1000_spread       5.23e-16    1.45e-15      9.71e-15      3.17e-14
    quadratic4099_spread       6.30e-16    1.44e-15      1.14e-14      3.22e-14
    bratu16_t10                7.41e-15    3.62e-14      1.20e-13      6.04e-13
    quadratic64_alpha_t1       1.32e-16    3.80e-16      3.37e-15      1.47e-14
    quadratic64_clamped        1.17e-16    3.54e-16      3.13e-15      1.42e-14
    quadratic65539             1.10e-16    2.57e-16      3.02e-15      1.27e-14
    quadratic262145            2.80e-16    6.99e-16      5.74e-15      1.98e-14
    stall64                    1.06e-11    1.46e-11      1.70e-10      2.44e-10
"""
import numpy as np

SUCCESS, MAXITERS, UNSTABLE, CONVERGENCE_FAILURE = "Success", "MaxIters", "Unstable", "ConvergenceFailure"
EPS = float(np.finfo(np.float64).eps)
ABSTOL = EPS ** 0.8                      # eps(Float64)^(4/5)
RESET_TOL = EPS ** 0.75                  # eps(Float64)^(3/4) (reset_conditions.jl:34; the docstring's sqrt(eps) is not the code)


# ------------------------------------------------------------------------------------------ problems (dtype-generic)
def quadratic(p=2.0):
    """quadratic_f(u, p) = u .* u .- p"""
    def f(u):
        return u * u - u.dtype.type(p)
    return f


def bratu(ns, lam=6.0):
    """5-point Bratu, h²-scaled: F_k = (4u_k − u_W − u_E − u_S − u_N) − h²λ exp(u_k), lexicographic k = j·ns + i."""
    def f(u):
        T = u.dtype.type
        g = u.reshape(ns, ns)
        s = T(4) * g
        s[:, 1:] = s[:, 1:] - g[:, :-1]
        s[:, :-1] = s[:, :-1] - g[:, 1:]
        s[1:, :] = s[1:, :] - g[:-1, :]
        s[:-1, :] = s[:-1, :] - g[1:, :]
        h = T(1) / T(ns + 1)
        return (s - (h * h * T(lam)) * np.exp(g)).reshape(-1)
    return f


def stall(p=2.0):
    """u² − p in every component but the last two, whose residuals are the constants 0 and 1. The constant 1 keeps the solve
    from converging. The constant 0 makes that component of δu and of dfu exactly 0 at every reset test, so every third test
    asks for a reset and the third reset ends the solve. (One constant non-zero component alone does not do it: its dfu is 0
    but its δu is not, and a reset test whose `du` flag is false zeroes both counters, reset_conditions.jl:65-68.)"""
    def f(u):
        r = u * u - u.dtype.type(p)
        r[-1] = u.dtype.type(1)
        r[-2] = u.dtype.type(0)
        return r
    return f


# ------------------------------------------------------------------------------------------ pieces of the algorithm
def initial_alpha(alpha, u, fu):
    """Utils.initial_jacobian_scaling_alpha (utils.jl:307-314) with internalnorm = L2: α, not its inverse."""
    T = u.dtype.type
    if alpha is not None:
        return T(alpha)
    fn = np.sqrt(np.dot(fu, fu))
    if fn < 1.0e-5:
        return T(1)
    return (T(2) * fn) / max(np.sqrt(np.dot(u, u)), T(1))


def mod1(i, m):
    return (i - 1) % m + 1


class LowRank:
    """BroydenLowRankJacobian: a·I + U Vᵀ over the first min(idx, threshold) columns (initialization.jl:209-296)."""

    def __init__(self, n, threshold, dtype):
        self.U = np.zeros((n, threshold), dtype)
        self.V = np.zeros((n, threshold), dtype)
        self.idx = 0
        self.a = dtype(1)

    def ncols(self):
        return min(self.idx, self.U.shape[1])

    def mul(self, x):                       # mul!(y, J, x)
        if self.idx == 0:
            return self.a * x
        m = self.ncols()
        c = np.array([np.dot(self.V[:, j], x) for j in range(m)], x.dtype)
        y = np.zeros_like(x)
        for j in range(m):
            y = y + self.U[:, j] * c[j]
        return y + self.a * x

    def tmul(self, x):                      # mul!(y, x, J): J⁻ᵀ x
        if self.idx == 0:
            return self.a * x
        m = self.ncols()
        c = np.array([np.dot(self.U[:, j], x) for j in range(m)], x.dtype)
        y = np.zeros_like(x)
        for j in range(m):
            y = y + self.V[:, j] * c[j]
        return y + self.a * x

    def rank1(self, ucol, vcol):            # mul!(J, u, vᵀ, true, true)
        j = mod1(self.idx + 1, self.U.shape[1]) - 1
        self.U[:, j] = ucol
        self.V[:, j] = vcol
        self.idx += 1
        return j


class NoChangeInStateReset:
    """reset_conditions.jl:39-87 with nsteps = 3, check_du = check_dfu = true."""

    def __init__(self, fu, tol, nsteps=3):
        self.ref = fu.copy()
        self.tol, self.nsteps = tol, nsteps
        self.since_du = self.since_dfu = 0
        self.last = None                    # what the last call looked at: (_closest(du), _closest(dfu), flag du, flag dfu); the dfu entries are None if the du branch returned early

    @staticmethod
    def _closest(x, tol):
        """How far the flag any(|x_i| ≤ tol) is from flipping under a perturbation of x, as a ratio ≥ 1: the flag is decided
        by min|x_i| alone, so this is min|x_i|/tol when the flag is false and tol/min|x_i| when it is true (inf for an
        exact zero). Entries near tol do not matter while a smaller one holds the flag."""
        m = float(np.min(np.abs(np.asarray(x, np.float64))))
        if m == 0.0:
            return float("inf")
        return max(m / tol, tol / m)

    def __call__(self, fu, du):
        fdu = bool(np.any(np.abs(du) <= self.tol))
        self.last = (self._closest(du, self.tol), None, fdu, None)
        if fdu:
            self.since_du += 1
            if self.since_du >= self.nsteps:
                self.since_du = self.since_dfu = 0
                return True                 # (self.ref stays where it was: the early return skips the dfu bookkeeping)
        else:
            self.since_du = self.since_dfu = 0
        dfu = fu - self.ref
        fdfu = bool(np.any(np.abs(dfu) <= self.tol))
        self.last = (self.last[0], self._closest(dfu, self.tol), fdu, fdfu)
        if fdfu:
            self.since_dfu += 1
            if self.since_dfu >= self.nsteps:
                self.since_dfu = self.since_du = 0
                self.ref = fu.copy()
                return True
        else:
            self.since_dfu = self.since_du = 0
        self.ref = fu.copy()
        return False


class Result:
    def __init__(self):
        self.u = self.fu = None
        self.retcode = None
        self.nsteps = 0
        self.nresets = 0
        self.reset_steps = []               # steps (1-based) at which a reset was asked for, the terminating one included
        self.us, self.fus = [], []          # after every step that moved u
        self.cols = []                      # 0-based column written by every update
        self.alphas = []                    # (step, a) every time a was (re)computed
        self.margins = []                   # (step,) + NoChangeInStateReset.last per reset test


def solve(f, u0, dtype=np.float64, threshold=10, max_resets=3, reset_tolerance=None, alpha=None, abstol=None,
          maxiters=1000, stop_after=None):
    """Runs until the termination check, the reset count or maxiters stops it (or `stop_after` steps were taken)."""
    T = np.dtype(dtype).type
    u = np.asarray(u0, dtype).copy()
    fu = f(u)
    threshold = min(int(threshold), int(maxiters))          # initialization.jl:180
    tol = RESET_TOL if reset_tolerance is None else float(reset_tolerance)
    abstol = ABSTOL if abstol is None else float(abstol)
    J = LowRank(u.size, threshold, T)
    reset = NoChangeInStateReset(fu, tol)
    du = np.zeros_like(u)
    R = Result()
    while R.retcode is None and R.nsteps < maxiters and (stop_after is None or R.nsteps < stop_after):
        step = R.nsteps + 1
        R.nsteps = step
        if step == 1:
            J.idx, J.a = 0, T(1) / initial_alpha(alpha, u, fu)
            R.alphas.append((step, J.a))
        else:
            asked = reset(fu, du)
            R.margins.append((step,) + reset.last)
            if asked:
                R.nresets += 1
                R.reset_steps.append(step)
                if R.nresets >= max_resets:
                    R.retcode = CONVERGENCE_FAILURE
                    break
                J.idx, J.a = 0, T(1) / initial_alpha(alpha, u, fu)
                R.alphas.append((step, J.a))
        du = -J.mul(fu)
        u = u + du
        fu_prev, fu = fu, f(u)
        R.us.append(u.copy())
        R.fus.append(fu.copy())
        obj = np.max(np.abs(fu))
        if not np.isfinite(obj):
            R.retcode = UNSTABLE
            break
        if obj <= abstol:
            R.retcode = SUCCESS
            break
        dfu = fu - fu_prev                                   # GoodBroydenUpdateRule (broyden.jl:129-147)
        w = J.mul(dfu)
        z = J.tmul(du)
        denom = np.dot(du, w)
        if denom == 0:
            denom = T(1.0e-5)
        R.cols.append(J.rank1((du - w) / denom, z))
    if R.retcode is None:
        R.retcode = MAXITERS if R.nsteps >= maxiters else None
    R.u, R.fu = u, fu
    return R


# ------------------------------------------------------------------------------------------ the cases the tests share
def spread_start(n=1000):
    """linspace(1, 2.375): the reset at step 14 and every reset test before it are decided by a min|δu_i| / min|dfu_i| at
    least a factor 10 away from the tolerance. (linspace(1, 3) resets at step 11 with a factor 2.)"""
    return np.linspace(1.0, 2.375, n)


CASES = {
    # name: (residual, u0, keyword arguments of solve, steps compared on the device)
    "quadratic64_t10": (quadratic(2.0), np.ones(64), dict(threshold=10), None),
    "quadratic64_t3": (quadratic(2.0), np.ones(64), dict(threshold=3), None),
    "quadratic1000_spread": (quadratic(2.0), spread_start(1000), dict(threshold=10), None),
    "quadratic4099_spread": (quadratic(2.0), spread_start(4099), dict(threshold=10), None),   # 5 workgroups, an odd tail
    "bratu16_t10": (bratu(16, 6.0), np.zeros(256), dict(threshold=10), 6),     # (diverges later: six steps are compared)
    "quadratic64_alpha_t1": (quadratic(2.0), np.ones(64), dict(threshold=1, alpha=2.5), None),
    "quadratic64_clamped": (quadratic(2.0), np.ones(64), dict(threshold=32, alpha=2.5, maxiters=4), None),
    "quadratic65539": (quadratic(2.0), np.ones(65539), dict(threshold=10), None),
    "quadratic262145": (quadratic(2.0), np.ones(2 ** 18 + 1), dict(threshold=10), None),
    "stall64": (stall(2.0), np.ones(64), dict(threshold=10), None),
}

_cache = {}


def run(name, dtype=np.float64):
    """the case's trajectory in the given arithmetic, computed once"""
    key = (name, np.dtype(dtype).name)
    if key not in _cache:
        f, u0, kw, upto = CASES[name]
        _cache[key] = solve(f, u0, dtype=dtype, stop_after=upto, **kw)
    return _cache[key]


def gaps(name):
    """per step: (max|u64 − u80|, max|fu64 − fu80|) between the float64 and the long-double run of a case"""
    a, b = run(name, np.float64), run(name, np.longdouble)
    assert len(a.us) == len(b.us) and a.reset_steps == b.reset_steps, (name, len(a.us), len(b.us))
    return [(float(np.max(np.abs(x - y))), float(np.max(np.abs(fx - fy))))
            for x, y, fx, fy in zip(a.us, b.us, a.fus, b.fus)]


MARGIN, FLOOR_ULPS = 16.0, 4.0


def bounds(name):
    """per step: (bound on max|Δu|, bound on max|Δfu|) for a device trajectory against run(name): MARGIN × the measured
    float64 ↔ long-double gap (the device sums in another order and forms w as J⁻¹fu_new + δu) plus a floor of FLOOR_ULPS
    units of eps at the size of the numbers that were rounded: ‖u‖∞ (at least 1) for u; for fu, ‖fu‖∞ plus the size of the
    terms that cancel in it, which for every residual here is bounded by 4‖u‖∞ + ‖u‖∞² + 2."""
    a = run(name, np.float64)
    out = []
    for (gu, gf), u, fu in zip(gaps(name), a.us, a.fus):
        su = max(1.0, float(np.max(np.abs(u))))
        sf = float(np.max(np.abs(fu))) + 4.0 * su + su * su + 2.0
        out.append((MARGIN * gu + FLOOR_ULPS * EPS * su, MARGIN * gf + FLOOR_ULPS * EPS * sf))
    return out
