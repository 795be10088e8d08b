"""Cases, the reference and the assertions for ONE trust-region step (csrc/nk_solver.hip: dogleg with k_dogleg_segment, tr_solve
with k_tr_trial, tr_defaults, tr_radii and the accept/reject bookkeeping of internal_step), in plain NumPy.
tests/test_gpu_trust_region.py hands the device's steps to judge_run below; tests/test_tr_reference.py hands it the oracle's
float64 formulation (which must pass) and float64 copies of the reference with one planted defect each (which must fail),
without a GPU.

The reference is `step` in np.longdouble, a restatement of the reference project's Dogleg.solve! (descent/dogleg.jl:86-151) and
GenericTrustRegionSchemeCache solve! (trust_region.jl:396-514) with the defaults of trust_region.jl:320-384: the Newton direction
from band_lu_reference's unpivoted band LU, every product formed from the CSR arrays, every scalar in long double. It does not
use the oracle's _dogleg, _tr_solve, _tr_defaults or _tr_radii. Two things follow this project, not the reference project's text:
Bastin's retrospective ratio uses the step just taken (the reference project reads a buffer it never writes), and reinit
restores the scheme parameters p1 … p4 (there, Yuan's and Fan's mutated p1 survives reinit!).

A step is judged from the device's OWN previous iterate and radius, so nothing accumulates: the reference carries only what the
device does not show (p1 of Yuan and Fan, the shrink counter). Besides the numbers it returns a label for every decision taken
and, for every comparison with a threshold, the relative distance of the two sides (`margins`).

Problems (a torch twin for the device in the GPU file, `f` and `jac_values` here in whatever float type `u` has):
  ros(n)   chained Rosenbrock f_i = 10(u_{i+1} − u_i²), f_n = 1 − u_n from linspace(−1.2, 1, n): an upper bidiagonal Jacobian.
           n = 9, and n = 2051: three workgroups of k_tr_trial / k_dogleg_segment with a ragged last one
  nf       the seven-unknown `newton_fails` system of tests/test_gpu_lm.py with a diagonal pattern. Its Jacobian is the analytic
           derivative here, not that file's central difference: a difference quotient with h = 1e-7 carries a rounding error
           of 1e-9 that long double does not share, which alone would use up the bound
  bratu3   the built-in Bratu2D(12) from u0 ≡ 3

Cases (all_cases): 7 schemes × (ros9, nf, bratu3) × initial_trust_radius (0, 0.05, 50); the column 0 passes 0 for EVERY option,
which is how the scheme's own defaults (tr_defaults) are reached — TrustRegion(radius_update_scheme = …) alone passes the
constructor's 1/10000, 1/4, 3/4, 1/4, 2 —, the other two columns leave the constructor's values. Then ros2051 for every scheme;
Bastin with expand_threshold = −1e30 (a decrease of ‖f‖ makes the retrospective ratio negative: its expansion runs in no other
way) and with −0.004 (inside the range the ratio takes on ros9, so that the ratio's VALUE matters); max_shrink_times = 2 on ros9 from radius 50 for every scheme; max_trust_radius = 0.3 for the final clamp. Fan's cap
min(p1·p3, p4 = 1e18) is UNREACHABLE: p1 starts at 0.1 and grows by 12 per expansion, so the cap needs 18 consecutive expansions
more than any shrink gave back, K ≤ 12 steps cannot make them, and a run long enough has converged long before.

Tolerances. TABLE holds, per case, the largest deviation of the oracle's float64 formulation (oracle.reference_restatement:
_dogleg + _tr_solve with its splu solve, driven for one step from that state) from the long-double step started at the same
state, over the states of the float64 twin's trajectory (the reference run in float64 from the start), for δu = u_new − u
(∞-norm, relative), ρ (relative to max(1, |ρ|)), the new radius (relative) and ‖f_new‖∞ (relative). Each is rounded UP to a
power of two; the bound is FACTOR = 100 times that, never below 1e-13 and never above 1e-9 — a case that would pass the cap
gets fewer steps or another start (bounds() asserts). Nothing is measured on the device. Regenerate with

    python tests/tr_reference.py

which prints TABLE. Every comparison of the first K steps of every case lies at least 1e-6 (relative) from its threshold in the
float64 twin, so float64 rounding cannot flip a decision; K was lowered where a later step came closer, where the spread would
put a bound above the cap, or where the Newton solve is no longer verifiable in float64 (SOLVE_RESIDUAL); see K_OF."""
import functools
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import band_lu_reference as BL  # noqa: E402

LD = np.longdouble
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63
FLOOR, LIMIT, FACTOR = 1e-13, 1e-9, 100.0
MARGIN = 1e-6
KMAX = 12
# The library's direct solve is verified (‖J x − f‖₂ ≤ 1e-8 ‖f‖₂ after one refinement step, else a GMRES fallback and, if that fails
# too, InternalLinearSolveFailed); the first residual decides about the refinement. A state is kept only where a float64 solve
# leaves a residual FACTOR below 1e-10·‖f‖₂: the Rosenbrock chain passes through |u_i| ≈ 1e-3 … 1e-7, where the pivots −20 u_i
# make J so ill-conditioned (growth 10 / |20 u_i| per row) that no float64 solve is verified and the step is not defined
SOLVE_RESIDUAL = 1e-10 / FACTOR
ROS_LONG_START = (0.55, 0.9)     # see the module docstring: the start of ros(n) for n ≥ 100
ROS_WARM_START = (0.8, 8.0)      # "ros9w": Newton steps that are accepted while they shorten — Hei's counter counts those

SIMPLE, NLSOLVE, NOCEDAL_WRIGHT, HEI, YUAN, BASTIN, FAN = range(7)     # RadiusUpdateSchemes, the library's numbering
SCHEME_NAMES = ("simple", "nlsolve", "nocedalwright", "hei", "yuan", "bastin", "fan")

REQUIRED_LABELS = (
    "dogleg/newton", "dogleg/cauchy", "dogleg/segment",
    "simple/shrink", "simple/expand", "simple/keep",
    "nlsolve/shrink", "nlsolve/expand", "nlsolve/middle", "nlsolve/keep",
    "nocedalwright/shrink", "nocedalwright/expand", "nocedalwright/keep",
    "hei/atan", "hei/exp", "hei/counted", "hei/reset",
    "yuan/shrink", "yuan/expand", "yuan/keep",
    "fan/shrink", "fan/expand", "fan/keep",
    "bastin/reject", "bastin/retro-expand", "bastin/retro-keep",
    "clamp", "accept", "reject")
UNREACHABLE_LABELS = ("fan/cap",)   # min(p1·p3, 1e18) taking 1e18: see the module docstring


def need_longdouble():
    if not LONGDOUBLE_OK:
        import pytest
        pytest.skip("np.longdouble has fewer than 64 significand bits on this machine")


# ------------------------------------------------------------------------------------------------------------- problems
class Problem:
    """f and the CSR Jacobian of one system; `f` and `jac_values` work in the float type of `u`."""

    def __init__(self, name, u0, rowptr, colind):
        self.name, self.u0, self.n = name, np.asarray(u0, dtype=np.float64), len(u0)
        self.rowptr, self.colind = np.asarray(rowptr, dtype=np.int64), np.asarray(colind, dtype=np.int64)
        self.row = np.repeat(np.arange(self.n), np.diff(self.rowptr))

    def J(self, u):
        return Jacobian(self, self.jac_values(u))


class Jacobian:
    def __init__(self, prob, vals):
        self.p, self.vals = prob, vals

    def mv(self, v):
        return np.add.reduceat(self.vals * v[self.p.colind], self.p.rowptr[:-1])

    def tmv(self, v):
        y = np.zeros(self.p.n, dtype=self.vals.dtype)
        np.add.at(y, self.p.colind, self.vals * v[self.p.row])
        return y

    def scipy(self):
        return sp.csr_matrix((self.vals, self.p.colind, self.p.rowptr), shape=(self.p.n, self.p.n))

    def solve(self, b):
        """J x = b: the unpivoted band LU in long double; a float64 twin takes a float64 sparse LU"""
        if self.vals.dtype == LD:
            if not hasattr(self, "_F"):
                self._F = BL.lu_band(self.scipy())
            return BL.solve_band(self._F, b)
        import scipy.sparse.linalg as spla
        if not hasattr(self, "_F"):
            self._F = spla.splu(sp.csc_matrix(self.scipy()))
        return self._F.solve(np.asarray(b, dtype=np.float64))


class Ros(Problem):
    def __init__(self, n, lo=-1.2, hi=1.0, name=None):
        rp = np.concatenate([2 * np.arange(n), [2 * n - 1]])
        ci = np.concatenate([np.repeat(np.arange(n - 1), 2) + np.tile([0, 1], n - 1), [n - 1]])
        super().__init__(name or f"ros{n}", np.linspace(lo, hi, n), rp, ci)

    def f(self, u):
        out = np.empty_like(u)
        out[:-1] = 10.0 * (u[1:] - u[:-1] * u[:-1])
        out[-1] = 1.0 - u[-1]
        return out

    def jac_values(self, u):
        v = np.empty(2 * self.n - 1, dtype=u.dtype)
        v[0:-1:2] = -20.0 * u[:-1]
        v[1:-1:2] = 10.0
        v[-1] = -1.0
        return v


NF_A, NF_B, NF_P, NF_Q, NF_R, NF_C = (0.010000000000000002, 10.000000000000002, 0.21640425613334457, 216.40425613334457,
                                      0.0006250000000000001, 0.0011552453009332421)


def nf_parts(u):
    """(value, derivative) of the `newton_fails` function, entrywise; numpy arrays of any float type, or torch tensors"""
    w = 1 + NF_R * (u * u)
    h = NF_P + NF_Q / w
    dh = -NF_Q * (2 * NF_R) * u / (w * w)
    v = 1 + h * h
    g = NF_P + NF_Q / v
    dg = -NF_Q * 2 * h * dh / (v * v)
    z = 1 + g * g
    return NF_A + NF_B / z - NF_C * u, -NF_B * 2 * g * dg / (z * z) - NF_C


class NewtonFails(Problem):
    def __init__(self):
        super().__init__("nf", [-110.0, -11.0, 11.0, 22.0, 33.0, 44.0, 110.0], np.arange(8), np.arange(7))

    def f(self, u):
        return nf_parts(u)[0]

    def jac_values(self, u):
        return nf_parts(u)[1]


class Bratu3(Problem):
    NS, LAM = 12, 6.0

    def __init__(self):
        ns = self.NS
        h = 1.0 / float(ns + 1)
        s = h * h
        self.c_lap, self.c_exp = s / (h * h), s * self.LAM     # float64, the operations of the library's bratu_coefficients
        j, i = np.divmod(np.arange(ns * ns), ns)
        k = np.arange(ns * ns)
        present = np.stack([j > 0, i > 0, np.ones_like(k, dtype=bool), i < ns - 1, j < ns - 1], axis=1)
        cols = np.stack([k - ns, k - 1, k, k + 1, k + ns], axis=1)
        super().__init__("bratu3", np.full(ns * ns, 3.0), np.concatenate([[0], np.cumsum(present.sum(axis=1))]), cols[present])
        self.diag = np.flatnonzero(self.colind == self.row)

    def f(self, u):
        ns = self.NS
        x = u.reshape(ns, ns)
        acc = 4 * x
        acc[:, 1:] -= x[:, :-1]
        acc[:, :-1] -= x[:, 1:]
        acc[1:, :] -= x[:-1, :]
        acc[:-1, :] -= x[1:, :]
        return self.c_lap * acc.ravel() - self.c_exp * np.exp(u)

    def jac_values(self, u):
        v = np.full(self.colind.size, -self.c_lap, dtype=u.dtype)
        v[self.diag] = 4 * self.c_lap - self.c_exp * np.exp(u)
        return v


@functools.lru_cache(maxsize=None)
def problem(name):
    if name.startswith("ros"):
        if name == "ros9w":
            return Ros(9, *ROS_WARM_START, name=name)
        n = int(name[3:])
        return Ros(n) if n < 100 else Ros(n, *ROS_LONG_START)
    return {"nf": NewtonFails, "bratu3": Bratu3}[name]()


# ------------------------------------------------------------------------------------------------------------- the reference
ALG_DEFAULTS = dict(max_trust_radius=0.0, initial_trust_radius=0.0, step_threshold=1.0 / 10000, shrink_threshold=1.0 / 4,
                    expand_threshold=3.0 / 4, shrink_factor=1.0 / 4, expand_factor=2.0, max_shrink_times=32)
ALL_ZERO = dict(step_threshold=0.0, shrink_threshold=0.0, expand_threshold=0.0, shrink_factor=0.0, expand_factor=0.0)

DEFECTS = ("tau_other_root", "c_dcauchy_not_squared", "cauchy_duJJdu_unscaled", "rho_without_half", "nlsolve_expands_from_tr",
           "nocedalwright_shrinks_tr", "hei_halves_swapped", "hei_counts_rejections", "yuan_norm_at_old_point", "fan_exponent_1",
           "fan_uses_f_old", "bastin_jacobian_at_old_point", "no_final_clamp", "accept_greater_or_equal", "counter_never_reset",
           "rejected_step_moves_u", "stale_JTf", "nd_and_tr_swapped_in_yuan")
# defects of reinit, judged by judge_reinit: p1 as the first run left it; Yuan's radius p1·‖Jᵀf‖ with the Jacobian of the last iterate
# (the second one was found on the device by tests/test_gpu_trust_region.py and fixed in tr_radii)
REINIT_DEFECTS = ("reinit_keeps_p1", "reinit_keeps_counter", "reinit_yuan_radius_from_last_jacobian")


def alg_options(scheme, **kw):
    """the keyword arguments of TrustRegion(radius_update_scheme = scheme, …) in full"""
    bad = set(kw) - set(ALG_DEFAULTS)
    assert not bad, bad
    return dict(ALG_DEFAULTS, radius_update_scheme=scheme, **kw)


def nrm2(x):
    return np.sqrt(np.dot(x, x))


def tr_defaults(alg, T=LD):
    """thresholds, factors and p1 … p4 of a scheme (trust_region.jl:320-384): an option given as 0 means the scheme's own"""
    m = alg["radius_update_scheme"]

    def pick(key, by_scheme, otherwise):
        v = alg[key]
        return T(by_scheme.get(m, otherwise) if v == 0 else v)

    d = SimpleNamespace(scheme=m)
    d.step_thr = pick("step_threshold", {HEI: 0.0, YUAN: 1.0 / 1000, BASTIN: 1.0 / 20}, 1.0 / 10000)
    d.shrink_thr = pick("shrink_threshold", {HEI: 0.0, NLSOLVE: 1.0 / 20, BASTIN: 1.0 / 20}, 1.0 / 4)
    d.expand_thr = pick("expand_threshold", {NLSOLVE: 9.0 / 10, HEI: 0.0, BASTIN: 9.0 / 10}, 3.0 / 4)
    d.shrink_f = pick("shrink_factor", {NLSOLVE: 1.0 / 2, HEI: 0.0, BASTIN: 1.0 / 20}, 1.0 / 4)
    d.expand_f = pick("expand_factor", {}, 2.0)
    p = {NLSOLVE: (1.0 / 2, 0.0, 0.0, 0.0), HEI: (5.0, 1.0 / 10, 15.0 / 100, 15.0 / 100), YUAN: (2.0, 1.0 / 6, 6.0, 0.0),
         FAN: (1.0 / 10, 1.0 / 4, 12.0, 1.0e18), BASTIN: (5.0 / 2, 1.0 / 4, 0.0, 0.0)}.get(m, (0.0, 0.0, 0.0, 0.0))
    d.p1, d.p2, d.p3, d.p4 = (T(x) for x in p)
    d.max_shrink_times = int(alg["max_shrink_times"]) if alg["max_shrink_times"] > 0 else 32
    return d


def tr_radii(alg, d, prob, u):
    """(max_trust_radius, initial_trust_radius) at u (trust_region.jl:204-258,330-346), Yuan's override p1·‖Jᵀf‖ included"""
    T = u.dtype.type
    m = alg["radius_update_scheme"]
    fu = prob.f(u)
    u_norm, f_norm = nrm2(u), nrm2(fu)
    if alg["max_trust_radius"] != 0:
        mtr = T(alg["max_trust_radius"])
    elif m in (SIMPLE, NOCEDAL_WRIGHT):
        mtr = max(f_norm, np.max(u) - np.min(u))
    else:
        mtr = T(np.inf)
    if m == YUAN:
        itr = d.p1 * nrm2(prob.J(u).tmv(fu))
    elif alg["initial_trust_radius"] != 0:
        itr = T(alg["initial_trust_radius"])
    elif m == NLSOLVE:
        itr = u_norm if u_norm > 0 else T(1)
    elif m in (HEI, BASTIN):
        itr = T(1)
    elif m == FAN:
        itr = f_norm ** T(0.99) / 10
    else:
        itr = mtr / 11
    return mtr, itr


def _dist(a, b):
    """relative distance of the two sides of a comparison of positive quantities"""
    s = max(abs(a), abs(b))
    return float(abs(a - b) / s) if s > 0 else 0.0


def _dist_rho(rho, thr):
    """ρ is a ratio of order one whose numerator ‖f_new‖² − ‖f‖² cancels: its distance from a threshold is taken relative to
    max(1, |threshold|), so a ρ of 1e-9 is NOT far from a threshold of 0"""
    return float(abs(rho - thr) / max(abs(thr), 1))


def step(prob, d, max_tr, u, tr, p1, counter, defect=None, stale=None):
    """One trust-region step from (u, tr) with the scheme's hidden state (p1, counter), in the float type of u.
    d: tr_defaults(...). Returns a namespace: du, rho, accepted, tr (new), p1 (new), counter (new), exceeded, u_trial, u_new and
    f_new (after the accept/reject), fnorm_inf, step_norm2 (‖δu‖₂ of the proposed step), labels, margins [(name, distance)].
    defect: one of DEFECTS, for the float64 copies of the CPU file; stale: the previous step's Jᵀf for the defect that needs it."""
    T = u.dtype.type
    tr, p1 = T(tr), T(p1)
    m = d.scheme
    labels, margins = [], []

    def cmp(name, dist):
        margins.append((name, dist))

    f = prob.f(u)
    J = prob.J(u)
    # ---- the dogleg (dogleg.jl:86-151)
    newton = -J.solve(f)
    duJJdu = None
    JTf = J.tmv(f)
    n_newton = nrm2(newton)
    cmp("newton<=tr", _dist(n_newton, tr))
    if n_newton <= tr:
        du = newton.copy()
        labels.append("dogleg/newton")
    else:
        cauchy = -JTf
        l_grad = nrm2(cauchy)
        Jc = J.mv(cauchy)
        dJJd = np.dot(Jc, Jc)
        d_cauchy = l_grad ** 3 / dJJd
        cmp("d_cauchy>=tr", _dist(d_cauchy, tr))
        if d_cauchy >= tr:
            lam = tr / l_grad
            du = lam * cauchy
            duJJdu = dJJd if defect == "cauchy_duJJdu_unscaled" else lam * lam * dJJd
            labels.append("dogleg/cauchy")
        else:
            c1 = (d_cauchy / l_grad) * cauchy
            c2 = newton - c1
            a, b = np.dot(c2, c2), 2 * np.dot(c1, c2)
            c = (d_cauchy if defect == "c_dcauchy_not_squared" else d_cauchy * d_cauchy) - tr * tr
            aux = max(T(0), b * b - 4 * a * c)
            tau = ((-b - np.sqrt(aux)) if defect == "tau_other_root" else (-b + np.sqrt(aux))) / (2 * a)
            du = c1 + tau * c2
            labels.append("dogleg/segment")
    # ---- the trial point and ρ (trust_region.jl:396-419)
    u_trial = u + du
    f_trial = prob.f(u_trial)
    if duJJdu is None:
        Jdu = J.mv(du)
        duJJdu = np.dot(Jdu, Jdu)
    if defect == "stale_JTf" and stale is not None:
        JTf = stale
    num = (np.dot(f_trial, f_trial) - np.dot(f, f)) / 2
    denom = np.dot(du, JTf) + (duJJdu if defect == "rho_without_half" else duJJdu / 2)
    rho = num / denom
    cmp("rho>step_thr", _dist_rho(rho, d.step_thr))
    accepted = bool(rho >= d.step_thr) if defect == "accept_greater_or_equal" else bool(rho > d.step_thr)
    nd = nrm2(du)
    tr_old = tr

    def shrunk():
        return counter + 1

    def reset():
        return counter if defect == "counter_never_reset" else 0

    # ---- the radius (trust_region.jl:421-509)
    if m == SIMPLE:
        cmp("rho<shrink_thr", _dist_rho(rho, d.shrink_thr))
        if rho < d.shrink_thr:
            tr, counter = tr * d.shrink_f, shrunk()
            labels.append("simple/shrink")
        else:
            counter = reset()
            cmp("rho>expand_thr", _dist_rho(rho, d.expand_thr))
            if rho > d.expand_thr and rho > d.step_thr:
                tr = d.expand_f * tr
                labels.append("simple/expand")
            else:
                labels.append("simple/keep")
    elif m == NLSOLVE:
        cmp("rho<shrink_thr", _dist_rho(rho, d.shrink_thr))
        if rho < d.shrink_thr:
            tr, counter = tr * d.shrink_f, shrunk()
            labels.append("nlsolve/shrink")
        else:
            counter = reset()
            cmp("rho>=expand_thr", _dist_rho(rho, d.expand_thr))
            if rho >= d.expand_thr:
                tr = d.expand_f * (tr if defect == "nlsolve_expands_from_tr" else nd)
                labels.append("nlsolve/expand")
            else:
                cmp("rho>=p1", _dist_rho(rho, d.p1))
                if rho >= d.p1:
                    tr = max(tr, d.expand_f * nd)
                    labels.append("nlsolve/middle")
                else:
                    labels.append("nlsolve/keep")
    elif m == NOCEDAL_WRIGHT:
        cmp("rho<shrink_thr", _dist_rho(rho, d.shrink_thr))
        if rho < d.shrink_thr:
            tr, counter = d.shrink_f * (tr if defect == "nocedalwright_shrinks_tr" else nd), shrunk()
            labels.append("nocedalwright/shrink")
        else:
            counter = reset()
            cmp("rho>expand_thr", _dist_rho(rho, d.expand_thr))
            at_edge = False
            if rho > d.expand_thr:
                gap, width = abs(nd - tr), T(1.0e-6) * tr
                cmp("|nd-tr|<1e-6tr", _dist(gap, width))
                at_edge = gap < width
            if at_edge:
                tr = d.expand_f * tr
                labels.append("nocedalwright/expand")
            else:
                labels.append("nocedalwright/keep")
    elif m == HEI:
        c2, M, g1, g2, beta = d.shrink_thr, d.p1, d.p3, d.p4, d.p2
        cmp("rho>=c2", _dist_rho(rho, c2))
        upper = (rho >= c2) != (defect == "hei_halves_swapped")
        if upper:
            rf = (2 * (M - 1 - g2) * np.arctan(rho - c2) + (1 + g2)) / T(np.pi)
            labels.append("hei/atan")
        else:
            rf = (1 - g1 - beta) * (np.exp(rho - c2) + beta / (1 - g1 - beta))
            labels.append("hei/exp")
        tr_new = rf * nd
        cmp("tr_new<tr", _dist(tr_new, tr))
        if defect == "hei_counts_rejections":
            count = not accepted
        else:
            count = tr_new < tr
        if count:
            counter = shrunk()
        else:
            counter = reset()
        labels.append("hei/counted" if tr_new < tr else "hei/reset")
        tr = tr_new
    elif m == YUAN:
        cmp("rho<shrink_thr", _dist_rho(rho, d.shrink_thr))
        if rho < d.shrink_thr:
            p1, counter = d.p2 * p1, shrunk()
            labels.append("yuan/shrink")
        else:
            cmp("rho>=expand_thr", _dist_rho(rho, d.expand_thr))
            grow = False
            if rho >= d.expand_thr:
                lhs, rhs = (2 * tr, nd) if defect == "nd_and_tr_swapped_in_yuan" else (2 * nd, tr)
                cmp("2nd>tr", _dist(lhs, rhs))
                grow = lhs > rhs
            if grow:
                p1 = d.p3 * p1
                labels.append("yuan/expand")
            else:
                labels.append("yuan/keep")
            counter = reset()
        g = JTf if defect == "yuan_norm_at_old_point" else prob.J(u_trial).tmv(f_trial)
        tr = p1 * nrm2(g)
    elif m == FAN:
        cmp("rho<shrink_thr", _dist_rho(rho, d.shrink_thr))
        if rho < d.shrink_thr:
            p1, counter = p1 * d.p2, shrunk()
            labels.append("fan/shrink")
        else:
            counter = reset()
            cmp("rho>expand_thr", _dist_rho(rho, d.expand_thr))
            if rho > d.expand_thr:
                cmp("p1*p3<p4", _dist(p1 * d.p3, d.p4))
                if p1 * d.p3 > d.p4:
                    labels.append("fan/cap")
                p1 = min(p1 * d.p3, d.p4)
                labels.append("fan/expand")
            else:
                labels.append("fan/keep")
        fn = nrm2(f if defect == "fan_uses_f_old" else f_trial)
        tr = p1 * (fn if defect == "fan_exponent_1" else fn ** T(0.99))
    elif m == BASTIN:
        if rho > d.step_thr:      # (the same comparison as the acceptance: its distance is recorded above)
            Jt = J if defect == "bastin_jacobian_at_old_point" else prob.J(u_trial)
            g = Jt.tmv(f_trial)
            gg = Jt.tmv(Jt.mv(du))
            rho2 = num / (np.dot(g, g) + np.dot(gg, gg) / 2)
            cmp("rho2>=expand_thr", _dist_rho(rho2, d.expand_thr))
            if rho2 >= d.expand_thr:
                tr = d.p1 * nd
                labels.append("bastin/retro-expand")
            else:
                labels.append("bastin/retro-keep")
            counter = reset()
        else:
            tr, counter = tr * d.p2, shrunk()
            labels.append("bastin/reject")
    else:
        raise ValueError(m)
    if not (tr == tr_old and tr == max_tr):   # (a radius carried over unchanged at the cap involves no arithmetic)
        cmp("tr<=max_tr", _dist(tr, max_tr) if np.isfinite(max_tr) else 1.0)
    if tr > max_tr:
        labels.append("clamp")
        if defect != "no_final_clamp":
            tr = max_tr
    labels.append("accept" if accepted else "reject")
    moved = accepted or defect == "rejected_step_moves_u"
    u_new, f_new = (u_trial, f_trial) if moved else (u, f)
    return SimpleNamespace(du=du, rho=rho, accepted=accepted, tr=tr, p1=p1, counter=counter, exceeded=counter > d.max_shrink_times,
                           u_trial=u_trial, u_new=u_new, f_new=f_new, fnorm_inf=np.max(np.abs(f_new)),
                           step_norm2=nd, labels=tuple(labels), margins=margins, JTf=JTf)


# ------------------------------------------------------------------------------------------------------------- cases
def case(name, prob, scheme, K=KMAX, **alg_kw):
    return SimpleNamespace(name=name, prob=prob, scheme=scheme, alg=alg_options(scheme, **alg_kw), K=K)


# the number of steps of a case where it is not KMAX: the step after it has a comparison closer than MARGIN to its threshold in
# the float64 twin, or a quantity whose float64 spread would put the bound above LIMIT (python tests/tr_reference.py reports both)
K_OF = {
    "simple-ros9-r0": 7, "simple-ros9-r0.05": 9, "simple-ros2051": 6, "nlsolve-ros9-r0.05": 7,
    "nlsolve-ros9-r50": 11, "nlsolve-nf-r0": 8, "nlsolve-ros2051": 6, "nocedalwright-ros9-r0": 7,
    "nocedalwright-ros9-r0.05": 9, "nocedalwright-ros2051": 6, "hei-ros9-r0": 4, "hei-ros9-r0.05": 7,
    "hei-ros9-r50": 7, "hei-ros2051": 6, "bastin-ros9-r0": 6, "bastin-ros9-r50": 10,
    "fan-ros9-r0": 7, "fan-ros2051": 6, "bastin-ros9-retro": 3, "yuan-ros9w": 5,
    "simple-ros9-clamp": 5,
}


@functools.lru_cache(maxsize=None)
def all_cases():
    out = {}

    def add(name, prob, scheme, **kw):
        out[name] = case(name, prob, scheme, K=K_OF.get(name, KMAX), **kw)

    for scheme, sname in enumerate(SCHEME_NAMES):
        for prob in ("ros9", "nf", "bratu3"):
            add(f"{sname}-{prob}-r0", prob, scheme, **ALL_ZERO)                       # every option the scheme's default
            for r in (0.05, 50.0):
                add(f"{sname}-{prob}-r{r:g}", prob, scheme, initial_trust_radius=r)   # the constructor's options
        add(f"{sname}-ros2051", "ros2051", scheme, initial_trust_radius=0.0)
        if scheme == HEI:    # (from ros9 at radius 50 Hei's counter reaches 2 and is reset; it counts shorter radii, not rejections)
            add(f"{sname}-ros9w-shrink2", "ros9w", scheme, max_shrink_times=2)
        else:
            add(f"{sname}-ros9-shrink2", "ros9", scheme, initial_trust_radius=50.0, max_shrink_times=2)
    add("bastin-ros9-retro", "ros9", BASTIN, expand_threshold=-1.0e30)
    # (a threshold inside the range the retrospective ratio takes here, −0.009 … −0.0006: both of its branches, and a ratio
    #  formed with the Jacobian of the OLD point, −0.0011 at the first step, decides differently)
    #  max_shrink_times = 2 with rejections that alternate with acceptances: a counter that is never reset passes 2, this one not
    add("bastin-ros9-retro-mid", "ros9", BASTIN, expand_threshold=-0.004, max_shrink_times=2)
    # Newton steps with ρ ≥ expand_threshold that are shorter than half the radius: the second operand of Yuan's expansion test
    add("yuan-ros9w", "ros9w", YUAN)
    add("simple-ros9-clamp", "ros9", SIMPLE, max_trust_radius=0.3, initial_trust_radius=0.2)
    return out


class Twin:
    """The reference driven as a solver: the float64 twin (defect = None) and the planted defects of the CPU file. It shows
    what the device shows — u, fu, the radius, a trace row per step, the retcode — and keeps p1 and the counter to itself."""

    def __init__(self, c, dtype=np.float64, defect=None):
        self.c, self.prob, self.defect = c, problem(c.prob), defect
        self.d = tr_defaults(c.alg, dtype)
        self._u = np.asarray(self.prob.u0, dtype=dtype)
        self.max_tr, self.tr = tr_radii(c.alg, self.d, self.prob, self._u)
        self.p1, self.counter, self.stopped, self.stale = self.d.p1, 0, False, None
        self.steps = []

    def u(self):
        return np.asarray(self._u, dtype=np.float64)

    def fu(self):
        return np.asarray(self.prob.f(self._u), dtype=np.float64)

    def radius(self):
        return float(self.tr)

    def retcode(self):
        return "ShrinkThresholdExceeded" if self.stopped else "Default"

    def reinit(self):
        last = self._u
        self._u = np.asarray(self.prob.u0, dtype=last.dtype)
        self.max_tr, self.tr = tr_radii(self.c.alg, self.d, self.prob, self._u)
        if self.defect == "reinit_yuan_radius_from_last_jacobian" and self.d.scheme == YUAN:
            self.tr = self.d.p1 * nrm2(self.prob.J(last).tmv(self.prob.f(self._u)))
        if self.defect != "reinit_keeps_p1":
            self.p1 = self.d.p1
        elif self.d.scheme == YUAN:
            self.tr = self.p1 * nrm2(self.prob.J(self._u).tmv(self.prob.f(self._u)))
        if self.defect != "reinit_keeps_counter":
            self.counter = 0
        self.stopped, self.stale, self.steps = False, None, []

    def step(self):
        s = step(self.prob, self.d, self.max_tr, self._u, self.tr, self.p1, self.counter, self.defect, self.stale)
        self._u, self.tr, self.p1, self.counter, self.stopped, self.stale = s.u_new, s.tr, s.p1, s.counter, s.exceeded, s.JTf
        self.steps.append(s)
        return dict(rho=float(s.rho), accepted=s.accepted, trust_region=float(s.tr), step_norm2=float(s.step_norm2),
                    fnorm_inf=float(s.fnorm_inf))


@functools.lru_cache(maxsize=None)
def twin_run(name, K=None):
    """the float64 twin's K steps of a case (it stops where the shrink counter passes max_shrink_times): (states, steps) with
    states[k] = (u, tr, p1, counter) before step k"""
    c = all_cases()[name]
    t = Twin(c)
    states = []
    for _ in range(c.K if K is None else K):
        states.append((t._u.copy(), t.tr, t.p1, t.counter))
        t.step()
        if t.stopped:
            break
    return states, t.steps


# ------------------------------------------------------------------------------------------------------------- tolerances
QUANTITIES = ("du", "rho", "radius", "fnorm")
# case -> the spread of (δu, ρ, radius, ‖f_new‖∞), each rounded up to a power of two: the output of `python tests/tr_reference.py`
TABLE = {
    'simple-ros9-r0': (2.0 ** -49, 2.0 ** -49, 0.0, 2.0 ** -50),
    'simple-ros9-r0.05': (2.0 ** -48, 2.0 ** -48, 0.0, 2.0 ** -52),
    'simple-ros9-r50': (2.0 ** -50, 2.0 ** -49, 0.0, 2.0 ** -50),
    'simple-nf-r0': (2.0 ** -49, 2.0 ** -46, 0.0, 2.0 ** -51),
    'simple-nf-r0.05': (2.0 ** -42, 2.0 ** -40, 0.0, 2.0 ** -51),
    'simple-nf-r50': (2.0 ** -45, 2.0 ** -43, 0.0, 2.0 ** -51),
    'simple-bratu3-r0': (2.0 ** -45, 2.0 ** -48, 0.0, 2.0 ** -48),
    'simple-bratu3-r0.05': (2.0 ** -46, 2.0 ** -46, 0.0, 2.0 ** -48),
    'simple-bratu3-r50': (2.0 ** -46, 2.0 ** -45, 2.0 ** -53, 2.0 ** -49),
    'simple-ros2051': (2.0 ** -44, 2.0 ** -51, 0.0, 2.0 ** -38),
    'simple-ros9-shrink2': (0.0, 2.0 ** -49, 0.0, 2.0 ** -56),
    'nlsolve-ros9-r0': (2.0 ** -51, 2.0 ** -49, 2.0 ** -52, 2.0 ** -50),
    'nlsolve-ros9-r0.05': (2.0 ** -48, 2.0 ** -48, 2.0 ** -51, 2.0 ** -53),
    'nlsolve-ros9-r50': (2.0 ** -49, 2.0 ** -49, 2.0 ** -51, 2.0 ** -51),
    'nlsolve-nf-r0': (2.0 ** -44, 2.0 ** -50, 2.0 ** -46, 2.0 ** -40),
    'nlsolve-nf-r0.05': (2.0 ** -42, 2.0 ** -40, 2.0 ** -52, 2.0 ** -51),
    'nlsolve-nf-r50': (2.0 ** -50, 2.0 ** -48, 2.0 ** -52, 2.0 ** -52),
    'nlsolve-bratu3-r0': (2.0 ** -47, 2.0 ** -45, 2.0 ** -61, 2.0 ** -45),
    'nlsolve-bratu3-r0.05': (2.0 ** -46, 2.0 ** -46, 2.0 ** -52, 2.0 ** -50),
    'nlsolve-bratu3-r50': (2.0 ** -46, 2.0 ** -45, 2.0 ** -51, 2.0 ** -49),
    'nlsolve-ros2051': (2.0 ** -48, 2.0 ** -50, 2.0 ** -52, 2.0 ** -48),
    'nlsolve-ros9-shrink2': (0.0, 2.0 ** -49, 0.0, 2.0 ** -56),
    'nocedalwright-ros9-r0': (2.0 ** -50, 2.0 ** -47, 2.0 ** -51, 2.0 ** -50),
    'nocedalwright-ros9-r0.05': (2.0 ** -48, 2.0 ** -48, 2.0 ** -52, 2.0 ** -52),
    'nocedalwright-ros9-r50': (2.0 ** -50, 2.0 ** -48, 2.0 ** -51, 2.0 ** -53),
    'nocedalwright-nf-r0': (2.0 ** -49, 2.0 ** -46, 2.0 ** -51, 2.0 ** -51),
    'nocedalwright-nf-r0.05': (2.0 ** -42, 2.0 ** -40, 0.0, 2.0 ** -51),
    'nocedalwright-nf-r50': (2.0 ** -45, 2.0 ** -43, 2.0 ** -52, 2.0 ** -51),
    'nocedalwright-bratu3-r0': (2.0 ** -45, 2.0 ** -48, 2.0 ** -51, 2.0 ** -48),
    'nocedalwright-bratu3-r0.05': (2.0 ** -46, 2.0 ** -46, 0.0, 2.0 ** -48),
    'nocedalwright-bratu3-r50': (2.0 ** -47, 2.0 ** -45, 2.0 ** -49, 2.0 ** -49),
    'nocedalwright-ros2051': (2.0 ** -44, 2.0 ** -50, 2.0 ** -53, 2.0 ** -37),
    'nocedalwright-ros9-shrink2': (0.0, 2.0 ** -49, 2.0 ** -51, 2.0 ** -56),
    'hei-ros9-r0': (2.0 ** -49, 2.0 ** -49, 2.0 ** -50, 2.0 ** -52),
    'hei-ros9-r0.05': (2.0 ** -48, 2.0 ** -48, 2.0 ** -49, 2.0 ** -52),
    'hei-ros9-r50': (2.0 ** -51, 2.0 ** -49, 2.0 ** -50, 2.0 ** -52),
    'hei-nf-r0': (2.0 ** -47, 2.0 ** -43, 2.0 ** -44, 2.0 ** -52),
    'hei-nf-r0.05': (2.0 ** -42, 2.0 ** -40, 2.0 ** -41, 2.0 ** -52),
    'hei-nf-r50': (2.0 ** -49, 2.0 ** -49, 2.0 ** -49, 2.0 ** -50),
    'hei-bratu3-r0': (2.0 ** -48, 2.0 ** -48, 2.0 ** -48, 2.0 ** -49),
    'hei-bratu3-r0.05': (2.0 ** -46, 2.0 ** -45, 2.0 ** -46, 2.0 ** -48),
    'hei-bratu3-r50': (2.0 ** -47, 2.0 ** -45, 2.0 ** -48, 2.0 ** -50),
    'hei-ros2051': (2.0 ** -47, 2.0 ** -49, 2.0 ** -49, 2.0 ** -42),
    'hei-ros9w-shrink2': (2.0 ** -47, 2.0 ** -50, 2.0 ** -49, 2.0 ** -45),
    'yuan-ros9-r0': (2.0 ** -41, 2.0 ** -42, 2.0 ** -49, 2.0 ** -52),
    'yuan-ros9-r0.05': (2.0 ** -41, 2.0 ** -42, 2.0 ** -49, 2.0 ** -52),
    'yuan-ros9-r50': (2.0 ** -41, 2.0 ** -42, 2.0 ** -49, 2.0 ** -52),
    'yuan-nf-r0': (2.0 ** -46, 2.0 ** -44, 2.0 ** -49, 2.0 ** -49),
    'yuan-nf-r0.05': (2.0 ** -46, 2.0 ** -44, 2.0 ** -49, 2.0 ** -49),
    'yuan-nf-r50': (2.0 ** -46, 2.0 ** -44, 2.0 ** -49, 2.0 ** -49),
    'yuan-bratu3-r0': (2.0 ** -48, 2.0 ** -45, 2.0 ** -45, 2.0 ** -50),
    'yuan-bratu3-r0.05': (2.0 ** -48, 2.0 ** -45, 2.0 ** -45, 2.0 ** -50),
    'yuan-bratu3-r50': (2.0 ** -48, 2.0 ** -45, 2.0 ** -45, 2.0 ** -50),
    'yuan-ros2051': (2.0 ** -49, 2.0 ** -47, 2.0 ** -51, 2.0 ** -51),
    'yuan-ros9-shrink2': (0.0, 2.0 ** -49, 2.0 ** -49, 2.0 ** -56),
    'bastin-ros9-r0': (2.0 ** -51, 2.0 ** -49, 0.0, 2.0 ** -51),
    'bastin-ros9-r0.05': (2.0 ** -48, 2.0 ** -47, 0.0, 2.0 ** -51),
    'bastin-ros9-r50': (2.0 ** -48, 2.0 ** -48, 0.0, 2.0 ** -51),
    'bastin-nf-r0': (2.0 ** -46, 2.0 ** -42, 0.0, 2.0 ** -52),
    'bastin-nf-r0.05': (2.0 ** -42, 2.0 ** -37, 0.0, 2.0 ** -52),
    'bastin-nf-r50': (2.0 ** -50, 2.0 ** -46, 0.0, 2.0 ** -52),
    'bastin-bratu3-r0': (2.0 ** -48, 2.0 ** -48, 0.0, 2.0 ** -48),
    'bastin-bratu3-r0.05': (2.0 ** -46, 2.0 ** -43, 0.0, 2.0 ** -51),
    'bastin-bratu3-r50': (2.0 ** -46, 2.0 ** -45, 0.0, 2.0 ** -48),
    'bastin-ros2051': (2.0 ** -48, 2.0 ** -48, 0.0, 2.0 ** -49),
    'bastin-ros9-shrink2': (0.0, 2.0 ** -49, 0.0, 2.0 ** -56),
    'fan-ros9-r0': (2.0 ** -49, 2.0 ** -49, 2.0 ** -51, 2.0 ** -51),
    'fan-ros9-r0.05': (2.0 ** -48, 2.0 ** -49, 2.0 ** -51, 2.0 ** -52),
    'fan-ros9-r50': (2.0 ** -50, 2.0 ** -47, 2.0 ** -50, 2.0 ** -51),
    'fan-nf-r0': (2.0 ** -48, 2.0 ** -45, 2.0 ** -51, 2.0 ** -51),
    'fan-nf-r0.05': (2.0 ** -42, 2.0 ** -41, 2.0 ** -51, 2.0 ** -50),
    'fan-nf-r50': (2.0 ** -49, 2.0 ** -47, 2.0 ** -51, 2.0 ** -51),
    'fan-bratu3-r0': (2.0 ** -46, 2.0 ** -46, 2.0 ** -49, 2.0 ** -48),
    'fan-bratu3-r0.05': (2.0 ** -46, 2.0 ** -47, 2.0 ** -49, 2.0 ** -50),
    'fan-bratu3-r50': (2.0 ** -48, 2.0 ** -45, 2.0 ** -46, 2.0 ** -50),
    'fan-ros2051': (2.0 ** -47, 2.0 ** -51, 2.0 ** -47, 2.0 ** -43),
    'fan-ros9-shrink2': (0.0, 2.0 ** -49, 2.0 ** -50, 2.0 ** -56),
    'bastin-ros9-retro': (2.0 ** -51, 2.0 ** -51, 2.0 ** -63, 2.0 ** -51),
    'bastin-ros9-retro-mid': (2.0 ** -51, 2.0 ** -49, 2.0 ** -52, 2.0 ** -51),
    'yuan-ros9w': (2.0 ** -48, 2.0 ** -51, 2.0 ** -48, 2.0 ** -45),
    'simple-ros9-clamp': (2.0 ** -51, 2.0 ** -50, 0.0, 2.0 ** -52),
}


def pow2_up(v):
    return 0.0 if v <= 0 else 2.0 ** math.ceil(math.log2(v)) if np.isfinite(v) else float("inf")


def bounds(name):
    out = tuple(max(FACTOR * s, FLOOR) for s in TABLE[name])
    assert max(out) <= LIMIT, f"{name}: badly conditioned for this purpose — fewer steps or another start, do not loosen the bound"
    return out


def deviations(obs, ref, u_prev):
    """(δu, ρ, radius, ‖f_new‖∞) of an observed step against the reference's; obs: a namespace or dict with u_new, rho,
    radius, fnorm_inf. δu is u_new − u_prev on both sides (relative, ∞-norm; 0 against 0 on a rejected step)."""
    g = (lambda k: obs[k]) if isinstance(obs, dict) else (lambda k: getattr(obs, k))
    up = np.asarray(u_prev, dtype=LD)
    du, du_ref = np.asarray(g("u_new"), dtype=LD) - up, ref.u_new - up
    scale = np.max(np.abs(du_ref))
    e_du = float(np.max(np.abs(du - du_ref)) / scale) if scale > 0 else float(np.max(np.abs(du)))
    e_rho = float(abs(LD(g("rho")) - ref.rho) / max(abs(ref.rho), 1))
    e_tr = float(abs(LD(g("radius")) - ref.tr) / ref.tr)
    e_f = float(abs(LD(g("fnorm_inf")) - ref.fnorm_inf) / ref.fnorm_inf)
    return e_du, e_rho, e_tr, e_f


def oracle_problem(R, prob):
    if prob.name == "bratu3":
        return R.Bratu2D(Bratu3.NS, Bratu3.LAM)
    return R.FunctionProblem(lambda u: prob.f(u), prob.u0, jac=lambda u: prob.J(u).scipy())


def oracle_alg(R, c):
    kw = {k: v for k, v in c.alg.items()}
    return R.TrustRegion(**kw)


def oracle_init(R, c, u0=None):
    prob = problem(c.prob)
    return R.init(oracle_problem(R, prob), oracle_alg(R, c), u0=prob.u0.copy() if u0 is None else u0, abstol=1e-200,
                  reltol=1e-200, store_trace=True)


@functools.lru_cache(maxsize=None)
def _oracle_max_tr(R, name):
    return oracle_init(R, all_cases()[name]).max_trust_radius


def oracle_step(R, c, u, tr, p1, counter):
    """the oracle's float64 formulation (its _dogleg and _tr_solve, with its splu solve) driven for ONE step from a state"""
    o = R.init(oracle_problem(R, problem(c.prob)), oracle_alg(R, c), u0=np.asarray(u, dtype=np.float64), abstol=1e-200,
               reltol=1e-200, store_trace=True)
    o.trust_region, o.p1, o.shrink_counter = float(tr), float(p1), int(counter)
    o.max_trust_radius = _oracle_max_tr(R, c.name)     # (fixed at u0, not at the state the step starts from)
    o.step()
    row = o.trace[-1]
    return SimpleNamespace(u_new=o.u.copy(), rho=row["rho"], radius=row["trust_region"], fnorm_inf=row["fnorm_inf"],
                           accepted=row["accepted"], counter=o.shrink_counter, p1=o.p1,
                           exceeded=o.retcode == R.SHRINK_EXCEEDED)


def reference_at(c, state, max_tr=None):
    """the long-double step from a float64 state (u, tr, p1, counter)"""
    prob = problem(c.prob)
    d = tr_defaults(c.alg)
    if max_tr is None:
        max_tr = tr_radii(c.alg, d, prob, np.asarray(prob.u0, dtype=LD))[0]
    u, tr, p1, counter = state
    return step(prob, d, max_tr, np.asarray(u, dtype=LD), LD(tr), LD(p1), counter)


def solve_residual(prob, u):
    """‖J x − f‖₂ / ‖f‖₂ of the float64 Newton solve at u"""
    u = np.asarray(u, dtype=np.float64)
    J, f = prob.J(u), prob.f(u)
    return float(nrm2(J.mv(J.solve(f)) - f) / nrm2(f))


def measure_steps(R, name, K=None):
    """per step of the float64 twin: (the four deviations of the oracle's one-step result from the long-double step at that
    state, the smallest margin of the twin's comparisons with its name)"""
    c = all_cases()[name]
    states, steps = twin_run(name, K)
    out = []
    for st, s in zip(states, steps):
        try:
            devs = deviations(oracle_step(R, c, *st), reference_at(c, st), st[0])
        except (ArithmeticError, IndexError):     # a step from a converged state (0 / 0), or a failed float64 solve: not a step to keep
            devs = (float("inf"),) * 4
        if not solve_residual(problem(c.prob), st[0]) <= SOLVE_RESIDUAL:
            devs = (float("inf"),) * 4
        out.append((devs, min(((dist, nm) for nm, dist in s.margins), default=(1.0, ""))))
    return out


def measure_case(R, name):
    """(the four spreads rounded up, the smallest margin over the twin's steps with its name and step, the labels visited)"""
    per = measure_steps(R, name)
    spread = [max(p[0][i] for p in per) for i in range(4)]
    worst = min((p[1] + (k,) for k, p in enumerate(per)), default=(1.0, "", 0))
    return tuple(pow2_up(s) for s in spread), worst, {lab for s in twin_run(name)[1] for lab in s.labels}


def supported_steps(R, name):
    """the largest K ≤ KMAX for which every step keeps its margin and every bound stays under LIMIT"""
    k = 0
    for devs, (dist, _nm) in measure_steps(R, name, KMAX):   # (a run that stops at ShrinkThresholdExceeded supports what it ran)
        if not dist >= MARGIN or not max(pow2_up(v) for v in devs) * FACTOR <= LIMIT:
            break
        k += 1
    return k


def measure_table(R):
    return {name: measure_case(R, name)[0] for name in all_cases()}


# ------------------------------------------------------------------------------------------------------------- the protocol
class Worst:
    """the largest deviation seen per quantity, for reports"""

    def __init__(self):
        self.dev = dict.fromkeys(QUANTITIES, 0.0)

    def add(self, devs):
        for q, v in zip(QUANTITIES, devs):
            self.dev[q] = max(self.dev[q], v)


def judge_run(c, dev, worst=None, log=print):
    """K steps of a solver object `dev` (u(), fu(), radius(), retcode(), step() -> the new trace row) on case c, each step judged
    against the long-double step from dev's own previous u and radius. Returns the labels of every step."""
    prob = problem(c.prob)
    d = tr_defaults(c.alg)
    tol = dict(zip(QUANTITIES, bounds(c.name)))
    max_tr, tr0 = tr_radii(c.alg, d, prob, np.asarray(prob.u0, dtype=LD))
    assert np.array_equal(dev.u(), prob.u0), "the solver does not start at u0"
    e0 = float(abs(LD(dev.radius()) - tr0) / tr0)
    log(f"{c.name}: initial radius {dev.radius()!r} vs {float(tr0)!r} (off by {e0:.2e}, bound {tol['radius']:.1e})")
    assert e0 <= tol["radius"], f"{c.name}: initial radius {dev.radius()!r} vs {float(tr0)!r}"
    twin_labels = [s.labels for s in twin_run(c.name)[1]]
    p1, counter = d.p1, 0
    labels = []
    for k in range(c.K):
        u_prev, fu_prev, tr_prev = dev.u(), dev.fu(), dev.radius()
        row = dev.step()
        ref = step(prob, d, max_tr, np.asarray(u_prev, dtype=LD), LD(tr_prev), p1, counter)
        u_new, fu_new = dev.u(), dev.fu()
        obs = dict(u_new=u_new, rho=row["rho"], radius=row["trust_region"], fnorm_inf=row["fnorm_inf"])
        devs = deviations(obs, ref, u_prev)
        log(f"{c.name} step {k}: {' '.join(ref.labels)}; rho {row['rho']!r}; deviation " +
            ", ".join(f"{q} {v:.2e}/{tol[q]:.1e}" for q, v in zip(QUANTITIES, devs)))
        what = f"{c.name} step {k}"
        assert all(np.isfinite(v) for v in devs), f"{what}: a non-finite quantity: {obs}"
        assert bool(row["accepted"]) == ref.accepted, f"{what}: accepted {row['accepted']} vs {ref.accepted} (rho {float(ref.rho)!r})"
        for q, v in zip(QUANTITIES, devs):
            assert v <= tol[q], f"{what}: {q} deviates by {v:.3e} > {tol[q]:.1e}"
        if worst is not None:
            worst.add(devs)
        assert dev.radius() == row["trust_region"], f"{what}: the radius {dev.radius()!r} is not the trace's {row['trust_region']!r}"
        e = float(abs(LD(np.max(np.abs(fu_new))) - ref.fnorm_inf) / ref.fnorm_inf)
        assert e <= tol["fnorm"], f"{what}: ‖fu‖∞ of the stored residual deviates by {e:.3e}"
        # the trace's step_norm2 is ‖δu‖₂ of the step the dogleg PROPOSED, taken or not (the reference project's trace records
        # norm(get_du(cache)) after every step!): on a rejected step it is the one view of δu the solver gives
        e = float(abs(LD(row["step_norm2"]) - ref.step_norm2) / ref.step_norm2)
        assert e <= tol["du"], f"{what}: step_norm2 {row['step_norm2']!r} vs {float(ref.step_norm2)!r} (off by {e:.3e})"
        if not ref.accepted:
            assert np.array_equal(u_new, u_prev), f"{what}: a rejected step moved u"
            assert np.array_equal(fu_new, fu_prev), f"{what}: a rejected step changed fu"
        assert k < len(twin_labels) and ref.labels == twin_labels[k], \
            f"{what}: decisions {ref.labels} vs the float64 twin's {twin_labels[k] if k < len(twin_labels) else None}"
        labels.append(ref.labels)
        p1, counter = ref.p1, ref.counter
        stopped = dev.retcode() == "ShrinkThresholdExceeded"
        assert stopped == ref.exceeded, f"{what}: retcode {dev.retcode()} with the reference's counter at {counter} " \
                                        f"(max_shrink_times {d.max_shrink_times})"
        if stopped:
            break
    return labels


REINIT_CASES = ("yuan-ros9-r0", "yuan-bratu3-r50", "fan-ros9-r50", "fan-nf-r0", "bastin-ros9-retro-mid", "simple-ros9-shrink2")


def judge_reinit(c, dev):
    """K steps, reinit at the same start, K steps again: the second run repeats the first bit for bit — the radius, p1 (Yuan and Fan
    change it as they go) and the shrink counter are restored. dev: judge_run's interface and reinit()."""
    def run():
        rows = []
        for _ in range(c.K):
            if dev.retcode() == "ShrinkThresholdExceeded":
                break
            r = dev.step()
            rows.append((r["rho"], r["accepted"], r["trust_region"], r["step_norm2"], r["fnorm_inf"]))
        return rows, dev.u(), dev.retcode()

    r0 = dev.radius()
    first = run()
    assert len({r[2] for r in first[0]}) > 1, "the radius never changed: the case shows nothing"
    dev.reinit()
    assert np.array_equal(dev.u(), problem(c.prob).u0) and dev.retcode() == "Default"
    assert dev.radius() == r0, f"{c.name}: the radius after reinit is {dev.radius()!r}, the initial one was {r0!r}"
    second = run()
    assert second[0] == first[0], f"{c.name}: the second run differs from step {[a == b for a, b in zip(*[first[0], second[0]])].index(False)}" \
        if len(second[0]) == len(first[0]) else f"{c.name}: {len(first[0])} steps, then {len(second[0])}"
    assert np.array_equal(first[1], second[1]) and first[2] == second[2]


def _p2(v):
    return "0.0" if v == 0 else f"2.0 ** {int(math.log2(v))}" if np.isfinite(v) else "float('inf')"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import reference_restatement as R_
    seen = set()
    print("TABLE = {")
    for name_ in all_cases():
        sp_, worst_, labs_ = measure_case(R_, name_)
        seen |= labs_
        flag = "" if worst_[0] >= MARGIN and max(sp_) * FACTOR <= LIMIT and supported_steps(R_, name_) >= len(twin_run(name_)[1]) else \
            f"   # !! margin {worst_[0]:.1e} ({worst_[1]}, step {worst_[2]}), largest bound {max(sp_) * FACTOR:.1e}"
        print(f"    {name_!r}: ({', '.join(_p2(s) for s in sp_)}),{flag}")
    print("}")
    print("# labels not visited:", sorted(set(REQUIRED_LABELS) - seen))
    print("# K_OF as the margins and the cap allow:",
          {n_: k_ for n_ in all_cases() for k_ in [supported_steps(R_, n_)] if k_ < len(twin_run(n_, KMAX)[1])})
