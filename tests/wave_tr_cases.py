"""Shared inputs of the per-wavefront SimpleTrustRegion tests (nk_batch_trust_region_wave, 8 < n ≤ 64): the residual
sources, their NumPy twins, the case list, the oracle's results (computed once per case and size), a second restatement of
trust_region.jl:57-229 that can count its branches, round differently and carry planted defects, and the one assertion helper
that the CPU tests and the GPU tests both use.

The base family is the suite's dense coupled residual f_i = u_i² − p_i + (0.1/n) Σu + 0.05 u_{i+1} u_i from rough starts."""
import functools
import json
import math
import os

import numpy as np

import ensemble_f32 as E32
from oracle import reference_restatement as R

NS = (9, 16, 33, 64)
NB = 130            # not a multiple of the 4 systems per workgroup
MAXITERS = 300
ABSTOL = float(np.finfo(float).eps) ** 0.8

DENSE_COUPLED = E32.DENSE_COUPLED   # the nk_real contract: compiles in both precisions

# the same residual times 0.1: ‖f(u0)‖₂, and with it Δmax and the gradient, shrink against the Newton step, which stays, so that
# all three dogleg branches are taken
DENSE_COUPLED_SCALED = """
template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f) {
  T s = u[0];
  for (int i = 1; i < NK_N; ++i) s = s + u[i];
  for (int i = 0; i < NK_N; ++i)
    f[i] = nk_real(0.1) * (u[i] * u[i] - p[i] + (nk_real(0.1) / NK_N) * s + nk_real(0.05) * u[(i + 1) % NK_N] * u[i]);
}
"""


def dense_f(u, p):
    n = u.shape[0]
    return u * u - p + (0.1 / n) * u.sum() + 0.05 * np.roll(u, -1) * u


def dense_jac(u, p):
    n = u.shape[0]
    J = np.diag(2.0 * u + 0.05 * np.roll(u, -1)) + (0.1 / n) * np.ones((n, n))
    J[np.arange(n), (np.arange(n) + 1) % n] += 0.05 * u
    return J


def scaled_f(u, p):
    return 0.1 * dense_f(u, p)


def scaled_jac(u, p):
    return 0.1 * dense_jac(u, p)


# name → (source, f, jac, solver keywords, kind of start)
#   rough    the base family from rough starts: hundreds of rejected trials, shrinks and expansions per n; the Newton and the
#            clipped-gradient branch (the segment branch almost never)
#   scaled   the residual times 0.1: all three dogleg branches more than 150 times at every n
#   shrink0  rough with max_shrink_times = 0: every system that ever shrinks ends in ShrinkThresholdExceeded
#   capped   the scaled residual from flat starts near 0.3, where the Newton step is some sixteen times Δmax = ‖f(u0)‖₂: the
#            radius doubles up to Δmax and stays there, step after step. The case that tells a missing clip at Δmax (the other
#            three do not: their radius never gets near Δmax while the Newton step is still outside it)
CASES = {
    "rough": (DENSE_COUPLED, dense_f, dense_jac, {}, "rough"),
    "scaled": (DENSE_COUPLED_SCALED, scaled_f, scaled_jac, {}, "rough"),
    "shrink0": (DENSE_COUPLED, dense_f, dense_jac, {"max_shrink_times": 0}, "rough"),
    "capped": (DENSE_COUPLED_SCALED, scaled_f, scaled_jac, {}, "flat"),
}


def inputs(n, nb=NB, start="rough"):
    """(P, u0) of size n: parameters in [1, 4); rough starts far from the roots (some components negative), or flat ones"""
    rng = np.random.default_rng(n)
    P = rng.uniform(1.0, 4.0, (nb, n))
    if start == "rough":
        u0 = rng.uniform(0.5, 2.0, (nb, n)) + 1.5 * rng.standard_normal((nb, n))
    else:
        u0 = 0.3 + 0.02 * rng.standard_normal((nb, n))
    return P, u0


def stack(out):
    """[(x, fx, retcode, iterations), …] → the four arrays"""
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int64))


def oracle_solve(f, jac, u0, P, **kw):
    u0 = np.asarray(u0, dtype=float)
    return stack([R.simple_trust_region(f, jac, u0 if u0.ndim == 1 else u0[b], P[b], **kw) for b in range(P.shape[0])])


@functools.lru_cache(maxsize=None)
def oracle(case, n):
    """oracle.reference_restatement.simple_trust_region over the case's ensemble: (u, resid, retcode, iterations); read-only"""
    _, f, jac, kw, start = CASES[case]
    P, u0 = inputs(n, start=start)
    out = oracle_solve(f, jac, u0, P, maxiters=MAXITERS, **kw)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ the second restatement
BRANCHES = ("newton", "clipped", "segment", "rejected", "shrink", "expand")
DEFECTS = ("jac_at_rejected", "fx_restored", "unclipped_expand")


def _sum_reversed(v):
    s = 0.0
    for a in v[::-1]:
        s += a
    return float(s)


def restatement(f, jac, u0, p, abstol=None, maxiters=1000, step_threshold=1e-4, shrink_threshold=0.25, expand_threshold=0.75,
                shrink_factor=0.25, expand_factor=2.0, max_shrink_times=32, rerounded=False, defect=None, census=None):
    """trust_region.jl:57-229 once more. As called by default it performs the oracle's floating-point operations one for one
    (the tests hold it to the oracle's bits), so `census` — a dict that gets BRANCHES counts added — counts the oracle's own
    branches. `rerounded=True` rounds the way a per-wavefront kernel may: the linear solve on the columns in reversed order,
    sums of squares and dot products from the last entry to the first, and ‖Jδ‖² for δᵀ(Jᵀ(Jδ)). `defect` plants one of DEFECTS:
    J re-evaluated at a rejected trial point; fx put back to the accepted point's residual after a rejection; expansion not
    clipped at Δmax. Returns (x, fx, retcode, iterations)."""
    assert defect is None or defect in DEFECTS
    if abstol is None:
        abstol = ABSTOL
    count = (lambda k: census.__setitem__(k, census.get(k, 0) + 1)) if census is not None else (lambda k: None)
    if rerounded:
        norm = lambda v: math.sqrt(_sum_reversed(v * v))
        dot = lambda a, b: _sum_reversed(a * b)
    else:
        norm = lambda v: float(np.linalg.norm(v))
        dot = lambda a, b: float(a @ b)

    def solve(J, b):
        try:
            return np.linalg.solve(J[:, ::-1], b)[::-1] if rerounded else np.linalg.solve(J, b)
        except np.linalg.LinAlgError:
            return np.full_like(b, np.nan)

    def done(fv):
        return (not np.any(np.isnan(fv))) and np.max(np.abs(fv)) <= abstol

    x = np.array(u0, dtype=float)
    xo = x.copy()
    fx = np.asarray(f(x, p), dtype=float)
    norm_fx = float(np.linalg.norm(fx))
    J = np.asarray(jac(x, p), dtype=float)
    dmax = max(norm_fx, float(np.max(x) - np.min(x)))
    delta = dmax / 11.0
    fk = 0.5 * norm_fx ** 2
    g = J.T @ fx
    fo = fx
    shrink = 0
    if done(fx):
        return x, fx, R.SUCCESS, 0
    with np.errstate(all="ignore"):
        for it in range(1, maxiters + 1):
            dN = -solve(J, fx)
            if norm(dN) <= delta:
                dl = dN
                count("newton")
            else:
                dsd = -g
                nsd = norm(dsd)
                if nsd >= delta:
                    dl = dsd * (delta / nsd)
                    count("clipped")
                else:
                    q = dN - dsd
                    dNN, dSN, dSS = dot(q, q), dot(dsd, q), dot(dsd, dsd)
                    tau = (-dSN + math.sqrt(dSN * dSN - dNN * (dSS - delta * delta))) / dNN
                    dl = dsd + tau * q
                    count("segment")
            x = xo + dl
            fx = np.asarray(f(x, p), dtype=float)
            fk1 = float(np.linalg.norm(fx)) ** 2 / 2.0
            Jd = J @ dl
            dHd = dot(Jd, Jd) if rerounded else float(dl @ (J.T @ Jd))
            r = (fk1 - fk) / (dot(dl, g) + dHd / 2.0)
            if r >= shrink_threshold:
                shrink = 0
            else:
                delta = shrink_factor * delta
                shrink += 1
                count("shrink")
                if shrink > max_shrink_times:
                    return x, fx, R.SHRINK_EXCEEDED, it
            if r >= step_threshold:
                if done(fx):
                    return x, fx, R.SUCCESS, it
                xo = x.copy()
                fo = fx
                J = np.asarray(jac(x, p), dtype=float)
                if r > expand_threshold:
                    delta = expand_factor * delta if defect == "unclipped_expand" else min(expand_factor * delta, dmax)
                    count("expand")
                fk = fk1
                g = J.T @ fx
            else:
                count("rejected")
                if defect == "jac_at_rejected":
                    J = np.asarray(jac(x, p), dtype=float)
                if defect == "fx_restored":
                    fx = fo
    return x, fx, R.MAXITERS, maxiters


def restatement_solve(case, n, **kw):
    _, f, jac, ckw, start = CASES[case]
    P, u0 = inputs(n, start=start)
    return stack([restatement(f, jac, u0[b], P[b], maxiters=MAXITERS, **ckw, **kw) for b in range(P.shape[0])])


# ------------------------------------------------------------------------------------------ Float32: the `rough` case
# ensemble_f32.simple_trust_region_f32 runs its elimination in Python, 17 s for the 130 systems of n = 64, so its retcodes and
# step counts are recorded in tests/golden/wave_tr_f32_steps.json (written by `PYTHONPATH=. python tests/wave_tr_cases.py`); test_wave_tr_cases.py
# recomputes a sample of them at every size.
F32_NS = (16, 64)
F32_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_tr_f32_steps.json")


def f32_inputs(n):
    P, u0 = inputs(n)
    return P.astype(np.float32), u0.astype(np.float32)


def f32_reference_compute(n, systems=None):
    """(retcode, iterations) of ensemble_f32.simple_trust_region_f32 on `rough` in Float32, for all or the listed systems"""
    P, u0 = f32_inputs(n)
    idx = range(P.shape[0]) if systems is None else systems
    out = [E32.simple_trust_region_f32(E32.dense_f, E32.dense_jac, u0[b], P[b], maxiters=MAXITERS) for b in idx]
    return np.array([o[2] for o in out], dtype=np.int64), np.array([o[3] for o in out], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def f32_reference(n):
    """the recorded (retcode, iterations) of size n"""
    with open(F32_GOLDEN) as fh:
        rec = json.load(fh)[str(n)]
    return np.array(rec["retcode"], dtype=np.int64), np.array(rec["iters"], dtype=np.int64)


# ------------------------------------------------------------------------------------------ the assertion both sides share
MIN_SAME = 0.97     # the cap of the per-thread kernel's test (test_gpu_ensemble.py): paths may split at a rounding-level tie
U_TOL = 1e-10


def check_against_oracle(u, resid, retcode, iters, ref, min_same=MIN_SAME, u_tol=U_TOL, abstol=ABSTOL):
    """A Float64 result against the oracle's `ref` = (u, resid, retcode, iterations): every retcode equal; retcode and step
    count both equal on at least `min_same` of the systems; on those |u − u_ref|∞ < u_tol (NaN counts as a miss unless the
    oracle has it too); every Success within abstol. Returns the share that took the oracle's number of steps."""
    uo, _, rco, ito = ref
    u, resid, retcode, iters = np.asarray(u), np.asarray(resid), np.asarray(retcode), np.asarray(iters)
    assert u.shape == uo.shape and retcode.shape == rco.shape
    bad = np.flatnonzero(retcode != rco)
    assert bad.size == 0, f"retcodes differ on systems {bad[:10].tolist()}: {retcode[bad[:10]].tolist()} vs {rco[bad[:10]].tolist()}"
    same = iters == ito
    share = float(same.mean())
    assert share >= min_same, f"only {share:.3f} of the systems took the oracle's number of steps"
    err = np.abs(u[same] - uo[same])
    err = np.where(np.isnan(u[same]) & np.isnan(uo[same]), 0.0, err)
    assert not np.isnan(err).any() and (err.size == 0 or float(err.max()) < u_tol), float(np.nanmax(err)) if err.size else 0.0
    ok = retcode == R.SUCCESS
    if ok.any():
        worst = float(np.max(np.abs(resid[ok])))
        assert worst <= abstol, worst
    return share


if __name__ == "__main__":   # writes the Float32 record
    rec = {}
    for n_ in F32_NS:
        rc_, it_ = f32_reference_compute(n_)
        rec[str(n_)] = {"retcode": rc_.tolist(), "iters": it_.tolist()}
    with open(F32_GOLDEN, "w") as fh:
        json.dump(rec, fh)
        fh.write("\n")
