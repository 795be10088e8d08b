"""NumPy restatement of Broyden and Klement without a line search (lib/NonlinearSolveQuasiNewton: broyden.jl:34-167,
klement.jl:29-128, initialization.jl:73-105 IdentityInitialization, reset_conditions.jl:18-120, solve.jl:296-486; the initial
scaling of NonlinearSolveBase/src/utils.jl:307-314), sequential and literal: the dense J⁻¹ is a NumPy matrix and a step makes
the three products the reference makes, J⁻¹·fu, J⁻¹·dfu and J⁻ᵀ·δu, each as a matrix-vector product of its own.

    Broyden, full:      J⁻¹ = I/α;  δu = −(J⁻¹ fu);  u += δu;  fu = f(u);  termination check;
                        dfu = fu − fu_prev;  w = J⁻¹ dfu;
                        good_broyden:  z = J⁻ᵀ δu,  denom = δu·w        bad_broyden:  z = dfu,  denom = ‖dfu‖₂²
                        J⁻¹ += ((δu − w)/denom) zᵀ                      (denom == 0 → 1e-5)
    Broyden, diagonal:  J⁻¹ = 1/α (a vector);  t = J⁻¹·dfu·δu;  denom = Σt;  J⁻¹ += (δu − t)·δu·J⁻¹/denom   (broyden.jl:149-167)
    Klement, diagonal:  J = α (a vector, not inverted);  δu = −(fu ./ J);
                        Jdu = J²·δu²;  J += ((fu − fu_prev − J·δu)/ifelse(Jdu == 0, 1e-5, Jdu))·δu·J²         (klement.jl:116-128)
    α = `alpha`, or 2‖fu‖₂ / max(‖u‖₂, 1), or 1 when ‖fu‖₂ < 1e-5 (the docstrings state the inverse; the code rules).

Reset tests, every step but the first: Broyden's is NoChangeInStateReset(nsteps = 3) with its own copy of the last residual it
looked at (lbroyden_reference.NoChangeInStateReset, the early return included); Klement's is IllConditionedJacobianReset,
any(iszero, J). A reset recomputes α from the current (u, fu); the reset that brings the count to `max_resets` ends the solve
with ConvergenceFailure and is not applied. The update rule's own residual copy is the previous residual at every step.

`dtype` is the arithmetic (float64 or np.longdouble); the thresholds that steer the control flow are Float64's in either, as in
lbroyden_reference.py, whose termination check, residuals and bound rule this module shares: a step's bound is 16 × that step's
float64 ↔ long-double gap plus 4 eps × the magnitudes rounded. Every case below has the same control flow in both arithmetics
(step count, retcode, reset steps; tests/test_broyden_reference.py pins them). Maxima over the steps of each case, x87 long
double; abstol = eps^(4/5):

    case                      steps  retcode             resets at    max gap u   max gap fu    max bound u  max bound fu
    broyden64_good               11  Success             —            4.39e-16    1.30e-15      8.28e-15      2.94e-14
    broyden64_bad                12  Success             —            4.16e-16    1.28e-15      7.92e-15      2.91e-14
    broyden64_diagonal           33  Success             9, 12, 15, 18, 21, 24, 27, 30, 33   2.17e-15    6.04e-15      3.59e-14      1.05e-13
    broyden65_good               11  Success             —            3.83e-16    1.09e-15      7.37e-15      2.60e-14
    broyden1000_good             13  Success             —            7.70e-16    1.96e-15      1.36e-14      4.11e-14
    broyden1000_bad              13  Success             —            8.40e-16    2.26e-15      1.47e-14      4.54e-14
    broyden1000_diagonal          9  Success             9            1.94e-16    6.83e-16      4.36e-15      1.95e-14
    broyden2049_good             13  Success             —            1.10e-15    3.00e-15      1.89e-14      5.73e-14
    broyden4099_diagonal          8  Success             —            1.90e-16    6.56e-16      4.29e-15      1.91e-14
    broyden64_alpha               7  Success             —            1.83e-16    5.35e-16      4.19e-15      1.72e-14
    broyden64_small_fu            2  Success             —            2.17e-16    7.24e-16      4.74e-15      2.02e-14
    broyden130_nonsym             4  (stopped)           —            3.45e-15    9.79e-15      5.66e-14      1.67e-13
    broyden_bratu16               6  (stopped)           —            2.81e-14    1.31e-13      4.51e-13      2.11e-12
    broyden_stall64              10  ConvergenceFailure  4, 7, 10     9.81e-12    1.52e-10      1.57e-10      2.45e-09
    klement64                     7  Success             —            2.48e-16    9.05e-16      5.48e-15      2.56e-14
    klement65                     7  Success             —            2.80e-16    9.32e-16      5.98e-15      2.60e-14
    klement1000                   7  Success             —            3.60e-16    1.37e-15      7.27e-15      3.31e-14
    klement4099                   7  Success             —            3.40e-16    1.31e-15      6.94e-15      3.21e-14
    klement64_alpha               6  Success             —            1.75e-16    5.27e-16      4.06e-15      1.71e-14
    klement_reset64               4  ConvergenceFailure  2, 3, 4      0.00e+00    0.00e+00      1.78e-15      1.42e-14

(the table is what `python tests/broyden_reference.py` prints). broyden130_nonsym also bounds J⁻¹ entry by entry
(matrix_bound): 16 × the entry-wise gap of the two matrices plus 4 eps × max|J⁻¹|.
"""
import numpy as np

import lbroyden_reference as LB
from lbroyden_reference import (ABSTOL, CONVERGENCE_FAILURE, EPS, FLOOR_ULPS, MARGIN, MAXITERS, RESET_TOL, SUCCESS, UNSTABLE,
                                NoChangeInStateReset, bratu, initial_alpha, quadratic, stall)

BROYDEN_MAX_N = 32768


def coupled(p=2.0, c=0.1):
    """fᵢ = uᵢ² − p + c·u₍ᵢ₊₁ mod n₎: one-sided coupling, so J⁻¹ is not symmetric and rows are not columns"""
    def f(u):
        T = u.dtype.type
        return u * u - T(p) + T(c) * np.roll(u, -1)
    return f


def klement_stall(p=2.0):
    """u² − p in every component but the last, whose residual is the constant 1: with alpha = 1 that component's J becomes
    1 + ((0 − 1·(−1))/1)·(−1)·1 = 0 at every update, so every reset test after the first step asks for a reset"""
    def f(u):
        r = u * u - u.dtype.type(p)
        r[-1] = u.dtype.type(1)
        return r
    return f


class Result(LB.Result):
    def __init__(self):
        super().__init__()
        self.J = None                       # J⁻¹ (Broyden: n×n, or the diagonal) or J (Klement) when the run ended


def solve(f, u0, dtype=np.float64, method="broyden", update_rule="good_broyden", max_resets=100, reset_tolerance=None,
          alpha=None, abstol=None, maxiters=1000, stop_after=None):
    T = np.dtype(dtype).type
    assert method in ("broyden", "klement") and update_rule in ("good_broyden", "bad_broyden", "diagonal")
    u = np.asarray(u0, dtype).copy()
    fu = f(u)
    n = u.size
    tol = RESET_TOL if reset_tolerance is None else float(reset_tolerance)
    abstol = ABSTOL if abstol is None else float(abstol)
    klement = method == "klement"
    diagonal = klement or update_rule == "diagonal"
    reset = None if klement else NoChangeInStateReset(fu, tol)
    du = np.zeros_like(u)
    J = None
    R = Result()

    def identity():
        a = initial_alpha(alpha, u, fu)
        R.alphas.append((R.nsteps, a if klement else T(1) / a))
        if klement:
            return np.ones(n, T) * a                     # J = α·1, not inverted
        if diagonal:
            return T(1) / (np.ones(n, T) * a)            # linsolve_identity!!(Diagonal): safe_inv per entry
        return np.eye(n, dtype=T) * (T(1) / a)

    while R.retcode is None and R.nsteps < maxiters and (stop_after is None or R.nsteps < stop_after):
        step = R.nsteps + 1
        R.nsteps = step
        if step == 1:
            J = identity()
        else:
            asked = bool(np.any(J == 0)) if klement else reset(fu, du)
            if not klement:
                R.margins.append((step,) + reset.last)
            if asked:
                R.nresets += 1
                R.reset_steps.append(step)
                if R.nresets >= max_resets:
                    R.retcode = CONVERGENCE_FAILURE
                    break
                J = identity()
        if klement:
            du = -(fu / J)
        elif diagonal:
            du = -(J * fu)
        else:
            du = -(J @ fu)
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
        if klement:                                           # klement.jl:116-128
            Jdu = (J * J) * (du * du)
            Jdu = np.where(Jdu == 0, T(1.0e-5), Jdu)
            J = J + ((fu - fu_prev - J * du) / Jdu) * du * (J * J)
            continue
        dfu = fu - fu_prev
        if diagonal:                                          # broyden.jl:149-167 (the rule is GoodBroydenUpdateRule)
            t = J * dfu * du
            denom = np.sum(t)
            if denom == 0:
                denom = T(1.0e-5)
            J = J + (du - t) * du * J / denom
            continue
        w = J @ dfu                                           # broyden.jl:129-147
        if update_rule == "good_broyden":
            z = J.T @ du
            denom = np.dot(du, w)
        else:
            z = dfu
            nrm = np.sqrt(np.dot(dfu, dfu))
            denom = nrm * nrm
        if denom == 0:
            denom = T(1.0e-5)
        J = J + np.outer((du - w) / denom, z)
    if R.retcode is None and R.nsteps >= maxiters:
        R.retcode = MAXITERS
    R.u, R.fu, R.J = u, fu, J
    return R


def _lin(n, hi=2.375):
    return np.linspace(1.0, hi, n)


CASES = {
    # name: (residual, u0, keyword arguments of solve, steps compared on the device). The starts are chosen so that every
    # reset test is decided at least a factor 2 away from its tolerance (`closest flag` of the table printed below).
    "broyden64_good": (quadratic(2.0), _lin(64, 1.2), dict(), None),
    "broyden64_bad": (quadratic(2.0), _lin(64, 1.2), dict(update_rule="bad_broyden"), None),
    "broyden64_diagonal": (quadratic(2.0), np.linspace(1.2, 1.6, 64), dict(update_rule="diagonal", alpha=3.0), None),
    "broyden65_good": (quadratic(2.0), _lin(65, 1.2), dict(), None),
    "broyden1000_good": (quadratic(2.0), _lin(1000), dict(), None),
    "broyden1000_bad": (quadratic(2.0), _lin(1000), dict(update_rule="bad_broyden"), None),
    "broyden1000_diagonal": (quadratic(2.0), _lin(1000, 1.2), dict(update_rule="diagonal", alpha=2.8), None),
    "broyden2049_good": (quadratic(2.0), _lin(2049), dict(), None),
    "broyden4099_diagonal": (quadratic(2.0), _lin(4099, 1.2), dict(update_rule="diagonal", alpha=2.8), None),   # 5 workgroups
    "broyden64_alpha": (quadratic(2.0), _lin(64, 1.5), dict(alpha=2.5), None),
    "broyden64_small_fu": (quadratic(2.0), np.sqrt(2.0) + 1.0e-7 * _lin(64, 2.0), dict(), None),   # ‖fu‖₂ < 1e-5: α = 1
    "broyden130_nonsym": (coupled(2.0, 0.1), _lin(130, 1.5), dict(), 4),
    "broyden_bratu16": (bratu(16, 6.0), np.zeros(256), dict(), 6),              # (does not solve it: six steps are compared)
    "broyden_stall64": (stall(2.0), np.ones(64), dict(max_resets=3), None),
    "klement64": (quadratic(2.0), _lin(64, 1.2), dict(method="klement"), None),
    "klement65": (quadratic(2.0), _lin(65, 1.2), dict(method="klement"), None),
    "klement1000": (quadratic(2.0), _lin(1000, 1.2), dict(method="klement"), None),
    "klement4099": (quadratic(2.0), _lin(4099, 1.2), dict(method="klement"), None),   # 5 workgroups in every vector kernel
    "klement64_alpha": (quadratic(2.0), _lin(64, 1.2), dict(method="klement", alpha=2.8), None),
    "klement_reset64": (klement_stall(2.0), np.ones(64), dict(method="klement", alpha=1.0, max_resets=3), None),
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
    assert (len(a.us), a.retcode, a.nsteps, a.reset_steps) == (len(b.us), b.retcode, b.nsteps, b.reset_steps), name
    return [(float(np.max(np.abs(x - y))), float(np.max(np.abs(fx - fy))))
            for x, y, fx, fy in zip(a.us, b.us, a.fus, b.fus)]


def bounds(name):
    """per step: (bound on max|Δu|, bound on max|Δfu|) for a device trajectory against run(name): the rule of
    lbroyden_reference.bounds — MARGIN × the measured gap plus FLOOR_ULPS eps at the size of the numbers rounded (for the
    coupled residual the extra term 0.1‖u‖∞ is below the 4‖u‖∞ the rule already carries)."""
    a = run(name, np.float64)
    out = []
    for (gu, gf), u, fu in zip(gaps(name), a.us, a.fus):
        su = max(1.0, float(np.max(np.abs(u))))
        sf = float(np.max(np.abs(fu))) + 4.0 * su + su * su + 2.0
        out.append((MARGIN * gu + FLOOR_ULPS * EPS * su, MARGIN * gf + FLOOR_ULPS * EPS * sf))
    return out


def matrix_bound(name):
    """entry by entry: MARGIN × |J64 − J80| + FLOOR_ULPS eps × max|J64|, for the matrix the run ended with"""
    a, b = run(name, np.float64).J, run(name, np.longdouble).J
    return MARGIN * np.abs(a - b).astype(np.float64) + FLOOR_ULPS * EPS * float(np.max(np.abs(a)))


if __name__ == "__main__":
    for name in CASES:
        r, g, b = run(name), gaps(name), bounds(name)
        print("    %-24s %6d  %-18s  %-10s %10.2e  %10.2e  %12.2e  %12.2e" % (
            name, r.nsteps, r.retcode or "(stopped)", ", ".join(map(str, r.reset_steps)) or "—",
            max(x[0] for x in g), max(x[1] for x in g), max(x[0] for x in b), max(x[1] for x in b)),
            "  closest flag: %.1f" % min([m for row in r.margins for m in row[1:3] if m is not None] or [float("inf")]))
