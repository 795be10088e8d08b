"""Cases, data, references and assertions for the exported vector kernels (csrc/nk_blas.hip: nk_dot, nk_nrm2, nk_norm_inf,
nk_axpy, nk_multidot, nk_multiaxpy, nk_fused_axpy_dot, nk_vec_axpby, nk_vec_fill), in plain NumPy. tests/test_gpu_blas.py hands
the device's results to the check_* functions below; tests/test_blas_reference.py hands them emulated and deliberately wrong
results, without a GPU.

Two kinds of data.

exact   every entry of x, y, w, V, a, b is a nonzero integer in ±[1, 8], every entry of h and s one in ±[1, 4]. Every partial
        sum, in any order, with or without FMA contraction, is then an integer below 2⁵³ (cap() gives each case's worst case,
        the largest being the fused pass's Σ w_new² ≤ n·4104²), so the reference is an int64 evaluation and the device has to
        return its bits; nrm2 has to return math.sqrt of the exact integer. Every term is nonzero: one dropped, doubled or
        misplaced element changes the result.
real    magnitudes uniform in [0.5, 2) with random signs (h, s, a, b too). The reference is evaluated in np.longdouble (64
        significand bits are required: need_real()). The tolerances are the any-order rounding bounds with u = 2⁻⁵³ — a sum
        of n products rounded once each and added in any order, in any tree, is within ((1+u)ⁿ − 1)·Σ|terms| of the exact sum;
        the factor 1.01 covers the second-order terms, n·u < 2⁻³⁰ at every size used:

            dot, each multidot h_j     1.01·(n+1)·u·Σ|x_i y_i|
            nrm2                       (0.505·(n+1)·u + u)·√Σx_i²                (half the relative error of Σx², and the root's)
            multiaxpy w_i              1.01·(nv+2)·u·(|w_i| + Σ_j|h_j V_ji|)
            fused w_i                  the same with nv+3 (the coefficient h_j s_j is rounded too)
            ‖w‖² (both)                1.01·(n+1)·u·Σw_i²                         against the device's own w
            fused h2_j                 1.01·(n+2)·u·|s_j|·Σ_i|V_ji w_i|           against the device's own w
            axpby, axpy y_i            2.02·u·(|a x_i| + |b y_i|)

        With magnitudes in [0.5, 2) every bound stays far below the smallest single term, 0.25 (the worst is 4n²u = 2⁻⁷ at
        n = 2²²), so these cases catch a single dropped element too. norm_inf has to be max|x_i| exactly. Nothing here is
        fitted to what a kernel returns.

Guards. Every device vector lives inside a larger allocation: PRE = 2 doubles of a NaN with a payload of its own in front (the
vector still starts on a 16-byte boundary), POST of them behind, and the ldv − n padding of every column of V holds it too.
A read past n poisons a result; a write past n changes a guard (check_guards, check_basis compare bits). Only 16-byte-aligned
vectors and even ldv are passed: that is the documented requirement (include/mi355x_nk.h).

The sizes come from nk_grid_for and the kernels' loops (NK_BLOCK = 256 threads): the smallest that reach 1, 2, 3 elements (the
odd tail alone, one pair, a pair and the tail), one block more or less, and the saturated grid plus a further, partial trip
through the grid-stride loop."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63    # otherwise the real-data cases skip: need_real()
KINDS = ("exact", "real")
GUARD_BITS = np.int64(0x7FF8C0DEC0DEC0DE)   # a quiet NaN that no arithmetic produces
PRE, POST = 2, 6
MAX_NV, CHUNK = 64, 16


def need_real(kind):
    """the real-data cases need a long double with at least 64 significand bits"""
    if kind == "real" and not LONGDOUBLE_OK:
        import pytest
        pytest.skip("np.longdouble has fewer than 64 significand bits on this machine")


# ------------------------------------------------------------------------------------------------------------------ cases
def _p(e):
    return 1 << e


def even(n):
    return n + (n & 1)


# dot, nrm2: pairs, 512 per block, at most 1024 blocks — the grid saturates at n = 2²⁰
DOT_N = [1, 2, 3, 511, 512, 513, 1023, 1024, 1025, _p(20), _p(20) + 1, _p(20) + 2, _p(20) + _p(19) + 7]
# norm_inf: elements, 1024 per block, at most 1024 blocks
NORM_INF_N = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, _p(20), _p(20) + 1, 5 * _p(18) + 3]
# multidot: pairs, 1024 per block, at most 512 blocks; columns in balanced chunks of at most 16 (edges 16→17, 32→33, 48→49, 64)
MULTIDOT = ([(4099, nv) for nv in list(range(1, 18)) + [31, 32, 33, 47, 48, 49, 63, 64]]
            + [(n, nv) for nv in (3, 17) for n in (1, 2, 3, 2047, 2048, 2049, _p(20) + 2, _p(20) + _p(18) + 5)])
LDV_PADS = (0, 64)                                # ldv = n rounded up to even, and 64 more
# multiaxpy: pairs, 512 per block, at most 1024 blocks; columns unrolled by four with a remainder loop
MULTIAXPY = ([(n, nv) for n in (2050, 4099) for nv in (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64)]
             + [(n, 3) for n in (1, 2, 3, _p(20) + 2, _p(20) + _p(19) + 7)])
# fused pass: elements, 1024 per block, at most 512 blocks; one instantiation per nv
FUSED = ([(4099, nv) for nv in range(1, 33)]
         + [(n, nv) for nv in (1, 16, 17, 32) for n in (1, 2, 255, 256, 257, 1025, _p(19) + 1, _p(19) + _p(17) + 3)])
# axpby, axpy: pairs, 512 per block, at most 4096 blocks — the grid saturates at n = 2²²
AXPBY_N = [1, 2, 3, 1023, 1024, 1025, _p(22) + 2, _p(22) + _p(21) + 5]
FILL_N = [1, 1023, 1024, 1025, _p(22) + 1, 5 * _p(20) + 3]
FILL_VALUES = [0.0, -0.0, 1.5, float("nan"), float("inf")]
# where a NaN is placed for norm_inf: first element, last element, the last block, the last trip of the grid-stride loop
NORM_INF_NAN = [(5 * _p(18) + 3, 0), (5 * _p(18) + 3, 5 * _p(18) + 2), (_p(20), _p(20) - 200), (5 * _p(18) + 3, _p(20) + 17),
                (1, 0), (257, 256)]
# (entry point, n, nv) of the largest case of each reduction, for the stale-partials test
LARGEST = [("dot", DOT_N[-1], 0), ("nrm2", DOT_N[-1], 0), ("norm_inf", NORM_INF_N[-1], 0), ("multidot", _p(20) + _p(18) + 5, 17),
           ("multiaxpy", _p(20) + _p(19) + 7, 3), ("fused", _p(19) + _p(17) + 3, 32)]


def chunks(nv):
    """[(jbase, nvc)] of nk_blas_multidot's column split: balanced chunks of at most 16"""
    nch = (nv + CHUNK - 1) // CHUNK
    out, j = [], 0
    for c in range(nch):
        nvc = (nv - j + (nch - c) - 1) // (nch - c)
        out.append((j, nvc))
        j += nvc
    return out


def cap(entry, n, nv=0):
    """the largest magnitude any partial sum of the exact-data case can reach"""
    if entry in ("dot", "nrm2", "multidot"):
        return n * 64
    if entry == "norm_inf":
        return 8
    if entry == "multiaxpy":
        return n * (8 + 32 * nv) ** 2                                  # Σ w_new², |w_new| ≤ 8 + nv·4·8
    if entry == "fused":
        wmax = 8 + 128 * nv                                            # |w_new| ≤ 8 + nv·(4·4)·8
        return max(n * wmax ** 2, 4 * n * 8 * wmax)                    # Σ w_new², s_j Σ V_ji w_i
    if entry in ("axpby", "axpy"):
        return 128
    raise KeyError(entry)


# ------------------------------------------------------------------------------------------------------------------- data
def _draw(rng, kind, size, top=8):
    sign = rng.choice(np.array([-1.0, 1.0]), size=size)
    if kind == "exact":
        return sign * rng.integers(1, top + 1, size=size).astype(np.float64)
    return sign * rng.uniform(0.5, 2.0, size=size)


def data(entry, kind, n, nv=0):
    """the case's operands (the same for every ldv): x, y, a, b for the two-vector entry points; V (nv × n), w, h, s for the
    basis kernels"""
    rng = np.random.default_rng(zlib.crc32(f"{entry}/{kind}/{n}/{nv}".encode()))
    d = SimpleNamespace(entry=entry, kind=kind, n=n, nv=nv)
    if entry in ("dot", "nrm2", "norm_inf", "axpby", "axpy"):
        d.x, d.y = _draw(rng, kind, n), _draw(rng, kind, n)
        d.a, d.b = (float(t) for t in _draw(rng, kind, 2))
        if entry == "axpy":
            d.b = 1.0
    else:
        d.V = _draw(rng, kind, (nv, n))
        d.w = _draw(rng, kind, n)
        d.h, d.s = _draw(rng, kind, nv, top=4), _draw(rng, kind, nv, top=4)
    return d


def guard_value():
    return np.array([GUARD_BITS]).view(np.float64)[0]


def guarded(v, post=POST):
    """PRE guards, the vector, `post` guards: the vector is buf[PRE : PRE + n]"""
    v = np.asarray(v, dtype=np.float64)
    buf = np.full(PRE + v.size + post, guard_value())
    buf[PRE:PRE + v.size] = v
    return buf


def guarded_basis(V, ldv):
    """PRE guards, nv columns of ldv doubles whose last ldv − n are guards, POST guards: column j is buf[PRE + j·ldv :][:n]"""
    nv, n = V.shape
    assert ldv >= n and ldv % 2 == 0
    buf = np.full(PRE + nv * ldv + POST, guard_value())
    if nv:
        buf[PRE:PRE + nv * ldv].reshape(nv, ldv)[:, :n] = V
    return buf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_guards(buf, n, what):
    """everything around buf[PRE : PRE + n] still holds the guard's bits"""
    b = bits(buf)
    bad = np.flatnonzero(np.concatenate([b[:PRE], b[PRE + n:]]) != GUARD_BITS)
    assert bad.size == 0, f"{what}: {bad.size} guard element(s) around the vector were written"


def check_unchanged(buf, before, what):
    """a read-only operand, guards and padding included, holds the bits it was given"""
    bad = np.flatnonzero(bits(buf) != bits(before))
    assert bad.size == 0, f"{what}: {bad.size} element(s) of a read-only operand or its guards changed, first at {bad[0] - PRE}"


# ------------------------------------------------------------------------------------------------------------- assertions
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _int(a):
    a = np.asarray(a, dtype=np.float64)
    r = a.astype(np.int64)
    assert np.array_equal(r.astype(np.float64), a), "exact data: a value that is not an integer"
    return r


def _equal(got, want, what):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.flatnonzero(~(got == want))                              # a NaN is never equal
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def _close(got, ref, tol, what):
    got, ref, tol = np.atleast_1d(_ld(got)), np.atleast_1d(_ld(ref)), np.atleast_1d(_ld(tol))
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err <= tol))                               # a NaN is never within the bound
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} outside the bound, first at {bad[0]}: |{float(got[bad[0]])!r} − "
                           f"{float(ref[bad[0]])!r}| = {float(err[bad[0]]):.3e} > {float(tol[bad[0]]):.3e}")


def _memo(d, key, fn):
    """a reference that depends on the case's operands alone is evaluated once per case"""
    memo = d.__dict__.setdefault("_memo", {})
    if key not in memo:
        memo[key] = fn()
    return memo[key]


def _sumsq_check(kind, n, w_dev, got, what):
    """‖w‖² against the vector the device itself returned"""
    if kind == "exact":
        wi = _int(w_dev)
        _equal(got, float(int(wi @ wi)), what)
    else:
        ss = _ld(w_dev) @ _ld(w_dev)
        _close(got, ss, 1.01 * (n + 1) * U * ss, what)


def check_dot(d, got, y=None):
    """got = x·y (y: another second operand than the case's, e.g. x itself)"""
    y = d.y if y is None else y
    if d.kind == "exact":
        _equal(got, float(int(_int(d.x) @ _int(y))), "dot")
    else:
        _close(got, _ld(d.x) @ _ld(y), 1.01 * (d.n + 1) * U * float(np.abs(d.x * y).sum()), "dot")


def check_nrm2(d, got):
    if d.kind == "exact":
        xi = _int(d.x)
        _equal(got, math.sqrt(int(xi @ xi)), "nrm2")
    else:
        r = np.sqrt(_ld(d.x) @ _ld(d.x))
        _close(got, r, (0.505 * (d.n + 1) * U + U) * r, "nrm2")


def check_norm_inf(d, got):
    _equal(got, np.max(np.abs(d.x)), "norm_inf")


def check_multidot(d, got):
    assert len(got) == d.nv
    if d.kind == "exact":
        _equal(got, _memo(d, "h", lambda: (_int(d.V) @ _int(d.w)).astype(np.float64)), "multidot h")
    else:
        w = _ld(d.w)
        ref = _memo(d, "h", lambda: np.array([_ld(d.V[j]) @ w for j in range(d.nv)], dtype=np.longdouble))
        _close(got, ref, 1.01 * (d.n + 1) * U * _memo(d, "habs", lambda: np.abs(d.V) @ np.abs(d.w)), "multidot h")


def _update_check(d, coef, extra, w_dev, what):
    """w_dev against w − Σ_j coef_j V_j, to (nv + extra)·u·(|w_i| + Σ_j|coef_j V_ji|)"""
    if d.kind == "exact":
        _equal(w_dev, _memo(d, what, lambda: (_int(d.w) - _int(coef) @ _int(d.V)).astype(np.float64)), what)
        return

    def reference():
        ref, mag = _ld(d.w).copy(), np.abs(d.w)
        for j in range(d.nv):
            ref -= coef[j] * _ld(d.V[j])
            mag = mag + np.abs(np.float64(coef[j]) * d.V[j])
        return ref, mag
    ref, mag = _memo(d, what, reference)
    _close(w_dev, ref, 1.01 * (d.nv + extra) * U * mag, what)


def check_multiaxpy(d, w_dev, norm2=None):
    """w_dev = w − Σ_j h_j V_j; norm2 (if asked for) = Σ w_dev²"""
    _update_check(d, _ld(d.h) if d.kind == "real" else d.h, 2, w_dev, "multiaxpy w")
    if norm2 is not None:
        _sumsq_check(d.kind, d.n, w_dev, norm2, "multiaxpy ‖w‖²")


def check_fused(d, w_dev, h2):
    """w_dev = w − Σ_j (h_j s_j) V_j; h2[j] = s_j·(V_j·w_dev), h2[nv] = Σ w_dev²"""
    assert len(h2) == d.nv + 1
    _update_check(d, _ld(d.h) * _ld(d.s) if d.kind == "real" else d.h * d.s, 3, w_dev, "fused w")
    if d.kind == "exact":
        _equal(h2[:d.nv], (_int(d.s) * (_int(d.V) @ _int(w_dev))).astype(np.float64), "fused h2")
    else:
        wl = _ld(w_dev)
        ref = np.array([d.s[j] * (_ld(d.V[j]) @ wl) for j in range(d.nv)], dtype=np.longdouble)
        _close(h2[:d.nv], ref, 1.01 * (d.n + 2) * U * np.abs(d.s) * (np.abs(d.V) @ np.abs(w_dev)), "fused h2")
    _sumsq_check(d.kind, d.n, w_dev, h2[d.nv], "fused ‖w‖²")


def check_axpby(d, y_dev, a=None, b=None, x=None):
    """y_dev = a x + b y (defaults: the case's own a, b, x)"""
    a, b, x = d.a if a is None else a, d.b if b is None else b, d.x if x is None else x
    if d.kind == "exact":
        _equal(y_dev, (int(a) * _int(x) + int(b) * _int(d.y)).astype(np.float64), "axpby y")
    else:
        al, bl = np.longdouble(a), np.longdouble(b)
        _close(y_dev, al * _ld(x) + bl * _ld(d.y), 2.02 * U * (np.abs(a * x) + np.abs(b * d.y)), "axpby y")
