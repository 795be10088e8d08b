"""NumPy restatement of DFSane at full size — GeneralizedDFSane (lib/NonlinearSolveSpectralMethods/src/solve.jl:127-259) with the
RobustNonMonotone line search as the reference states it in-tree (lib/SimpleNonlinearSolve/src/dfsane.jl:114-144) — sequential
and literal: d = −σ f, the trial points u ± α d, axpy!(α, d, u), δu = u − u_cache and δf = fu − fu_cache elementwise, the two
dots ⟨δu,δu⟩ and ⟨δu,δf⟩, the copies into the caches. (The device never forms δu or δf: csrc/nk_qn.hip.)

    start:  σ = sigma_1, or ⟨u,u⟩/⟨u,f⟩ replaced by clamp(1/‖f‖₂, 1, 1e5) when !(σ_min ≤ |σ| ≤ σ_max);
            f₁ = ‖f(u0)‖₂^n_exp; history = M × f₁; k = 0.
    step:   k += 1; η = f₁/k²; f̄ = max(history); α₊ = α₋ = 1; trial at u + α₊ d; then
              loop: accept +α₊ if ‖f_t‖^n_exp ≤ f̄ + η − γ α₊² ‖f‖^n_exp;
                    α_t₊ = α₊² ‖f‖ⁿ / (‖f_t‖ⁿ + (2α₊ − 1)‖f‖ⁿ); trial at u − α₋ d; accept −α₋ by the same test with α₋;
                    α_t₋ likewise; α± = clamp(α_t±, τ_min α±, τ_max α±); trial at u + α₊ d; inner += 1;
                    inner = max_inner_iterations: the search has failed (that last trial is not looked at).
            u += α d; fu = f(u); termination check; σ = ⟨δu,δu⟩/⟨δu,δf⟩ with the same bounds test (on the new ‖f‖₂);
            caches; history[mod1(k, M)] = ‖fu‖₂^n_exp.
    Fixed by this project, not by the reference text: k counts outer steps only; the inner counter is the
    search's own; every trial is ONE residual evaluation (nf += 1; the accepted trial is not evaluated a second time).
    A NaN trial norm fails both tests, makes α_t NaN, clamp keeps NaN, and the search runs to its cap: no early exit.

`dtype` is the arithmetic (float64 or np.longdouble); the parameters are Float64's in either. Every sum is sequential
(np.cumsum), as tests/simple_jf_reference.py sums, so that a run whose steps are all accepted at the first trial repeats
SimpleDFSane's float64 trajectory bit for bit (tests/test_dfsane_reference.py). The termination check is the part of
AbsNormSafeBestTerminationMode(maximum∘abs) a short solve can reach: non-finite → Unstable, max|fu| ≤ abstol → Success.

Every comparison a run makes is recorded in Result.decisions as (step, kind, outcome, relative margin): the two acceptance
tests ("accept+", "accept-"), the two branches of each clamp ("clamp+>hi", "clamp+<lo", "clamp->hi", "clamp-<lo") and the two
halves of the σ-bounds test ("sigma>=min", "sigma<=max"). The margin of a ≤ b is |a − b| / max(|a|, |b|); a comparison with
a NaN operand cannot be flipped by a rounding and has margin inf. The shared cases are chosen so that the float64 and the
long-double run take the same decisions and every margin is at least 2⁻²⁰.

Bounds for a device trajectory (bounds(name), never from the device): MARGIN = 16 × the gap between the float64 and the
long-double run at that step, plus a floor of FLOOR_ULPS = 4 units of eps at the size of the numbers that were rounded —
max(1, ‖u‖∞) for u; ‖fu‖∞ + 4‖u‖∞ + ‖u‖∞² + 2 for fu (the terms that cancel in the residuals used here). For the scalars the
getter reports (scalar_bounds(name)) the floor is eps × (log₂ n + 4) — a blocked tree sum — × FLOOR_ULPS × the condition of
the sum: for σ the condition of ⟨δu,δf⟩, Σ|δu_i δf_i| / |Σ δu_i δf_i|; for a history entry additionally the fu floor carried
into Σf², 2‖f‖₁ × floor; for α the two merits' relative floors × the condition of α_t's denominator.
"""
import numpy as np

SUCCESS, MAXITERS, UNSTABLE, LINESEARCH_FAILED = "Success", "MaxIters", "Unstable", "InternalLineSearchFailed"
EPS = float(np.finfo(np.float64).eps)
ABSTOL = EPS ** 0.8


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


def root_domain():
    """f_i = sqrt(u_i) + 1 (even i), sqrt(u_i) − 3 (odd i): defined for u ≥ 0 only. From u0 = 0.01 the plus trial takes the
    even components below 0 and the minus trial the odd ones: every trial of the first line search returns NaN."""
    def f(u):
        T = u.dtype.type
        with np.errstate(invalid="ignore"):
            r = np.sqrt(u)
        r[0::2] = r[0::2] + T(1)
        r[1::2] = r[1::2] - T(3)
        return r
    return f


# ------------------------------------------------------------------------------------------ pieces of the algorithm
def seq_dot(a, b):
    """Σ a_i b_i, summed in index order from the first product"""
    return np.cumsum(a * b)[-1]


def mod1(i, m):
    return (i - 1) % m + 1


def jl_clamp(x, lo, hi):
    """Julia's clamp: x > hi ? hi : x < lo ? lo : x (NaN stays NaN)"""
    return hi if x > hi else (lo if x < lo else x)


def jl_maximum(v):
    """maximum(history): NaN propagates"""
    return v.dtype.type(np.nan) if np.isnan(v).any() else np.max(v)


def margin(a, b):
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return float("inf")
    m = max(abs(a), abs(b))
    return float("inf") if m == 0.0 else abs(a - b) / m


class Result:
    def __init__(self):
        self.u = self.fu = None
        self.retcode = None
        self.nsteps = 0
        self.nf = 0                          # residual evaluations of the line searches (the one at the start is not counted)
        self.sigma0 = None
        self.us, self.fus = [], []           # after every step that moved u
        self.sigmas, self.alphas, self.trials, self.histories = [], [], [], []   # after every step: σ for the next one, signed α
        self.sigma_cond, self.alpha_floor = [], []
        self.decisions = []                  # (step, kind, outcome, relative margin)
        self.sigma_replaced = []             # steps after which the bounds test replaced σ (0: at the start)


def solve(f, u0, dtype=np.float64, sigma_min=1e-10, sigma_max=1e10, sigma_1=None, M=10, gamma=1e-4, tau_min=0.1,
          tau_max=0.5, n_exp=2, max_inner_iterations=100, abstol=None, maxiters=1000, stop_after=None):
    assert 1 <= M <= 32 and n_exp in (1, 2)
    T = np.dtype(dtype).type
    smin, smax, gam, tmin, tmax = (T(v) for v in (sigma_min, sigma_max, gamma, tau_min, tau_max))
    abstol = ABSTOL if abstol is None else float(abstol)
    R = Result()

    def cmp_le(step, kind, a, b):
        out = bool(a <= b)
        R.decisions.append((step, kind, out, margin(a, b)))
        return out

    def clamp(step, side, x, lo, hi):
        hi_hit = bool(x > hi)
        R.decisions.append((step, "clamp%s>hi" % side, hi_hit, margin(x, hi)))
        if hi_hit:
            return hi
        lo_hit = bool(x < lo)
        R.decisions.append((step, "clamp%s<lo" % side, lo_hit, margin(x, lo)))
        return lo if lo_hit else x

    def merit(fv):
        nrm = np.sqrt(seq_dot(fv, fv))
        return nrm if n_exp == 1 else nrm * nrm

    def bounded(step, sigma, fv):
        ok = cmp_le(step, "sigma>=min", smin, abs(sigma)) and cmp_le(step, "sigma<=max", abs(sigma), smax)
        if ok:
            return sigma
        R.sigma_replaced.append(step)
        return jl_clamp(T(1) / np.sqrt(seq_dot(fv, fv)), T(1), T(1.0e5))

    with np.errstate(all="ignore"):
        u = np.asarray(u0, dtype).copy()
        fu = f(u)
        u_cache, fu_cache = u.copy(), fu.copy()
        sigma = T(sigma_1) if sigma_1 is not None else bounded(0, seq_dot(u, u) / seq_dot(u, fu), fu)
        R.sigma0 = sigma
        fn = merit(fu)
        f1 = fn
        hist = np.full(M, f1, dtype)
        k = 0
        while R.retcode is None and R.nsteps < maxiters and (stop_after is None or R.nsteps < stop_after):
            k += 1
            R.nsteps = k
            eta = f1 / T(k * k)
            fbar = jl_maximum(hist)
            d = -sigma * fu
            ap = am = T(1)
            alpha, ntr, afloor = None, 1, 0.0
            ft = f(u + ap * d)
            fnew = merit(ft)
            inner = 0
            while True:
                if cmp_le(k, "accept+", fnew, (fbar + eta) - gam * (ap * ap) * fn):
                    alpha = ap
                    break
                atp = (ap * ap) * fn / (fnew + (T(2) * ap - T(1)) * fn)
                kp = float((fnew + abs(T(2) * ap - T(1)) * fn) / abs(fnew + (T(2) * ap - T(1)) * fn))
                ft = f(u - am * d)
                fnew = merit(ft)
                ntr += 1
                if cmp_le(k, "accept-", fnew, (fbar + eta) - gam * (am * am) * fn):
                    alpha = -am
                    break
                atm = (am * am) * fn / (fnew + (T(2) * am - T(1)) * fn)
                km = float((fnew + abs(T(2) * am - T(1)) * fn) / abs(fnew + (T(2) * am - T(1)) * fn))
                ap = clamp(k, "+", atp, tmin * ap, tmax * ap)
                am = clamp(k, "-", atm, tmin * am, tmax * am)
                afloor = max(kp, km)
                ft = f(u + ap * d)
                fnew = merit(ft)
                ntr += 1
                inner += 1
                if inner >= max_inner_iterations:
                    break
            R.nf += ntr
            R.trials.append(ntr)
            if alpha is None:
                R.retcode = LINESEARCH_FAILED
                R.alphas.append(T(np.nan))
                break
            u = u + alpha * d                                   # axpy!(α, du, u)
            fu = f(u)                                           # (the trial's values: not counted a second time)
            R.us.append(u.copy())
            R.fus.append(fu.copy())
            R.alphas.append(alpha)
            R.alpha_floor.append(afloor)
            obj = np.max(np.abs(fu))
            if not np.isfinite(obj):
                R.retcode = UNSTABLE
            elif obj <= abstol:
                R.retcode = SUCCESS
            du = u - u_cache                                    # the spectral update runs whatever the check said (solve.jl:234-250)
            dfu = fu - fu_cache
            sxf = seq_dot(du, dfu)
            R.sigma_cond.append(float(np.cumsum(np.abs(du * dfu))[-1] / abs(sxf)) if sxf != 0 else float("inf"))
            sigma = bounded(k, seq_dot(du, du) / sxf, fu)
            u_cache, fu_cache = u.copy(), fu.copy()
            fn = merit(fu)
            hist[mod1(k, M) - 1] = fn
            R.sigmas.append(sigma)
            R.histories.append(hist.copy())
    if R.retcode is None and R.nsteps >= maxiters:
        R.retcode = MAXITERS
    R.u, R.fu = u, fu
    return R


# ------------------------------------------------------------------------------------------ the cases the tests share
def spread_start(n=1000):
    return np.linspace(1.0, 2.375, n)


CASES = {
    # name: (residual, u0, keyword arguments of solve, steps compared on the device)
    "quadratic64": (quadratic(2.0), np.ones(64), dict(), None),
    "quadratic64_M3": (quadratic(2.0), np.ones(64), dict(M=3), None),
    "quadratic64_nexp1": (quadratic(2.0), np.ones(64), dict(n_exp=1), None),
    "quadratic64_sigma1": (quadratic(2.0), np.full(64, 1.3), dict(sigma_1=0.4), None),
    "quadratic64_smin": (quadratic(2.0), np.ones(64), dict(sigma_min=0.35), None),
    # (34 steps to Success; by step 10 the trajectory has amplified a rounding by 10⁵ and by step 26 by 10⁹: six steps — with
    #  both minus-side acceptances — are compared on the device, the whole solve's decisions are checked here)
    "quadratic1000_spread": (quadratic(2.0), spread_start(1000), dict(), 6),
    "quadratic4099_spread": (quadratic(2.0), spread_start(4099), dict(), 6),   # 5 workgroups, an odd tail; six steps likewise
    "bratu16_g2": (bratu(16, 6.0), np.zeros(256), dict(gamma=2.0, tau_min=0.3), 12),   # (first steps only: twelve are compared)
    "quadratic1": (quadratic(2.0), np.ones(1), dict(), None),
    "quadratic2": (quadratic(2.0), np.ones(2), dict(), None),
    "quadratic63": (quadratic(2.0), np.ones(63), dict(), None),
    "quadratic257": (quadratic(2.0), np.ones(257), dict(), None),
    "quadratic65539": (quadratic(2.0), np.ones(65539), dict(), None),
    "quadratic262145": (quadratic(2.0), np.ones(2 ** 18 + 1), dict(), None),
    "root_domain_nan": (root_domain(), np.full(64, 0.01), dict(sigma_1=1.0, max_inner_iterations=3), None),
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
    assert len(a.us) == len(b.us) and a.trials == b.trials, (name, len(a.us), len(b.us))
    return [(float(np.max(np.abs(x - y))), float(np.max(np.abs(fx - fy))))
            for x, y, fx, fy in zip(a.us, b.us, a.fus, b.fus)]


MARGIN, FLOOR_ULPS = 16.0, 4.0


def _floors(u, fu):
    su = max(1.0, float(np.max(np.abs(u))))
    sf = float(np.max(np.abs(fu))) + 4.0 * su + su * su + 2.0
    return FLOOR_ULPS * EPS * su, FLOOR_ULPS * EPS * sf


def bounds(name):
    """per step: (bound on max|Δu|, bound on max|Δfu|) for a device trajectory against run(name): MARGIN × the measured
    float64 ↔ long-double gap plus a floor of FLOOR_ULPS units of eps at the size of the numbers that were rounded: ‖u‖∞ (at
    least 1) for u; for fu, ‖fu‖∞ plus the size of the terms that cancel in it, bounded by 4‖u‖∞ + ‖u‖∞² + 2 here."""
    a = run(name, np.float64)
    out = []
    for (gu, gf), u, fu in zip(gaps(name), a.us, a.fus):
        flu, flf = _floors(u, fu)
        out.append((MARGIN * gu + flu, MARGIN * gf + flf))
    return out


def scalar_bounds(name):
    """per step: (bound on |Δσ|, bound on |Δα|, bound on max|Δhistory|) for what the getter reports after that step"""
    a, b = run(name, np.float64), run(name, np.longdouble)
    out = []
    for k, (u, fu) in enumerate(zip(a.us, a.fus)):
        n = u.size
        tree = FLOOR_ULPS * EPS * (np.log2(n) + 4.0)
        _flu, flf = _floors(u, fu)
        h64, h80 = a.histories[k], b.histories[k]
        hfloor = tree * np.abs(np.asarray(h64, np.float64)) + 2.0 * float(np.sum(np.abs(fu))) * flf   # (n_exp = 1: ‖Δf‖₂ ≤ ‖f‖₁-free √n·floor)
        if CASES[name][2].get("n_exp", 2) == 1:
            hfloor = tree * np.abs(np.asarray(h64, np.float64)) + np.sqrt(n) * flf
        if a.sigmas[k] != a.sigmas[k]:
            bs = float("inf")
        else:
            bs = MARGIN * abs(float(a.sigmas[k]) - float(b.sigmas[k])) + tree * a.sigma_cond[k] * abs(float(a.sigmas[k]))
        hrel = float(np.max(hfloor / np.maximum(np.abs(np.asarray(h64, np.float64)), 1e-300)))
        ba = MARGIN * abs(float(a.alphas[k]) - float(b.alphas[k])) + abs(float(a.alphas[k])) * a.alpha_floor[k] * 2.0 * hrel
        bh = MARGIN * np.abs(np.asarray(h64 - h80, np.float64)) + hfloor
        out.append((bs, ba, bh))
    return out
