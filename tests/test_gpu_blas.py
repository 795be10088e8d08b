"""The exported vector kernels (csrc/nk_blas.hip) on their own, through the C ABI, against tests/blas_reference.py: every size
at which a loop, the grid or the column dispatch takes another path; exact integer data whose result has to come back bit for
bit and real data held to the any-order rounding bounds of a long-double reference; NaN guards in front of and behind every
vector and in the padding of every basis column; a small call after a large one on the same context; argument errors, empty
vectors, and the contract for zero coefficients and x == y that include/mi355x_nk.h states. What the assertions are worth is
shown without a GPU by tests/test_blas_reference.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import blas_reference as BR

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------------------------------------------- helpers
class Lib:
    """the ctypes library and the handle of the one context every test here runs on"""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h


@pytest.fixture(scope="module")
def lib(nls):
    from nonlinearsolve_jl_amd import _lib as L
    return Lib(L.lib(), nls.default_context()._h)


class Vec:
    """a guarded buffer on the device; .p is the pointer to the vector inside it (16-byte aligned)"""

    def __init__(self, buf, dev):
        import torch
        self.host = buf
        self.t = torch.from_numpy(buf).to(dev)
        self.p = C.c_void_p(self.t.data_ptr() + 8 * BR.PRE)
        assert self.p.value % 16 == 0

    def back(self):
        return self.t.cpu().numpy()

    def vector(self, n):
        return self.back()[BR.PRE:BR.PRE + n]


def _vec(v, dev):
    return Vec(BR.guarded(v), dev)


def _basis(d, ldv, dev):
    return Vec(BR.guarded_basis(d.V, ldv), dev)


def _intact(v, what):
    BR.check_unchanged(v.back(), v.host, what)


def _dbl(k):
    return (C.c_double * max(k, 1))(*([NAN] * max(k, 1)))


def _arr(v):
    return (C.c_double * max(len(v), 1))(*[float(t) for t in v])


@functools.lru_cache(maxsize=2)
def _data(entry, kind, n, nv=0):
    return BR.data(entry, kind, n, nv)


def _ok(rc):
    from nonlinearsolve_jl_amd import _lib as L
    assert rc == 0, f"the library returned {rc}: {L.lib().nk_last_error().decode(errors='replace')}"


def _ids(cases):
    return ["-".join(str(t) for t in c) for c in cases]


def _kinds(sizes, *more):
    """(kind, size…, extra…) with the cases that share their data next to each other"""
    out = []
    for kind in BR.KINDS:
        for s in sizes:
            s = s if isinstance(s, tuple) else (s,)
            out += [(kind,) + s + (m,) for m in more[0]] if more else [(kind,) + s]
    return out


# --------------------------------------------------------------------------------------------------------------- reductions
def _reduce(lib, entry, x, y, n):
    r = C.c_double(NAN)
    if entry == "dot":
        _ok(lib.lib.nk_dot(lib.h, n, x.p, y.p, C.byref(r)))
    elif entry == "nrm2":
        _ok(lib.lib.nk_nrm2(lib.h, n, x.p, C.byref(r)))
    else:
        _ok(lib.lib.nk_norm_inf(lib.h, n, x.p, C.byref(r)))
    return r.value


@pytest.mark.parametrize("kind,n", _kinds(BR.DOT_N), ids=_ids(_kinds(BR.DOT_N)))
def test_dot_nrm2(lib, dev, kind, n):
    BR.need_real(kind)
    d = _data("dot", kind, n)
    x, y = _vec(d.x, dev), _vec(d.y, dev)
    BR.check_dot(d, _reduce(lib, "dot", x, y, n))
    BR.check_dot(d, _reduce(lib, "dot", x, x, n), y=d.x)               # both operands the same pointer
    BR.check_nrm2(d, _reduce(lib, "nrm2", x, None, n))
    _intact(x, "x"), _intact(y, "y")


@pytest.mark.parametrize("kind,n", _kinds(BR.NORM_INF_N), ids=_ids(_kinds(BR.NORM_INF_N)))
def test_norm_inf(lib, dev, kind, n):
    BR.need_real(kind)
    d = _data("norm_inf", kind, n)
    x = _vec(d.x, dev)
    BR.check_norm_inf(d, _reduce(lib, "norm_inf", x, None, n))
    _intact(x, "x")


@pytest.mark.parametrize("n,at", BR.NORM_INF_NAN, ids=_ids(BR.NORM_INF_NAN))
def test_norm_inf_special_values(lib, dev, n, at):
    """One element that decides the result, at the first and the last position, in the last block and in the last trip of the
    grid-stride loop: a NaN gives NaN, an Inf of either sign Inf, and a planted maximum is found (random data cannot tell
    whether every element is looked at: most of them are not the maximum)."""
    d = _data("norm_inf", "exact", n)
    for val, want in ((NAN, NAN), (-INF, INF), (INF, INF), (-16.0, 16.0)):
        xs = d.x.copy()
        xs[at] = val
        got = _reduce(lib, "norm_inf", _vec(xs, dev), None, n)
        assert (np.isnan(got) if np.isnan(want) else got == want), (val, got)
    xs = d.x.copy()
    xs[at], xs[(at + n // 2) % n] = NAN, INF                           # a NaN wins over an Inf, whichever comes first
    assert n == 1 or np.isnan(_reduce(lib, "norm_inf", _vec(xs, dev), None, n))


@pytest.mark.parametrize("n", [1, 257, 1025, BR.NORM_INF_N[-1]])
def test_norm_inf_of_negative_zeros(lib, dev, n):
    got = _reduce(lib, "norm_inf", _vec(np.full(n, -0.0), dev), None, n)
    assert got == 0.0 and not np.signbit(got)


# ----------------------------------------------------------------------------------------------------------- basis kernels
def _multidot(lib, d, V, ldv, w):
    h = _dbl(d.nv)
    _ok(lib.lib.nk_multidot(lib.h, d.n, d.nv, V.p, ldv, w.p, h))
    return np.array(h[:d.nv])


def _multiaxpy(lib, d, V, ldv, w, norm):
    r = C.c_double(NAN)
    _ok(lib.lib.nk_multiaxpy(lib.h, d.n, d.nv, V.p, ldv, _arr(d.h), w.p, C.byref(r) if norm else None))
    return r.value if norm else None


def _fused(lib, d, V, ldv, w):
    h2 = _dbl(d.nv + 1)
    _ok(lib.lib.nk_fused_axpy_dot(lib.h, d.n, d.nv, V.p, ldv, _arr(d.h), _arr(d.s), w.p, h2))
    return np.array(h2[:d.nv + 1])


MD = _kinds(BR.MULTIDOT, BR.LDV_PADS)


@pytest.mark.parametrize("kind,n,nv,pad", MD, ids=_ids(MD))
def test_multidot(lib, dev, kind, n, nv, pad):
    """every instantiation 1..16 as a chunk of some nv, the split at its edges, both grid regimes; ldv = n rounded up to even
    and 64 more than that"""
    BR.need_real(kind)
    d, ldv = _data("multidot", kind, n, nv), BR.even(n) + pad
    V, w = _basis(d, ldv, dev), _vec(d.w, dev)
    BR.check_multidot(d, _multidot(lib, d, V, ldv, w))
    _intact(V, "V"), _intact(w, "w")


MA = _kinds(BR.MULTIAXPY, (False, True))


@pytest.mark.parametrize("kind,n,nv,norm", MA, ids=_ids(MA))
def test_multiaxpy(lib, dev, kind, n, nv, norm):
    BR.need_real(kind)
    d, ldv = _data("multiaxpy", kind, n, nv), BR.even(n) + 64
    V, w = _basis(d, ldv, dev), _vec(d.w, dev)
    got = _multiaxpy(lib, d, V, ldv, w, norm)
    BR.check_guards(w.back(), n, "w")
    BR.check_multiaxpy(d, w.vector(n), got)
    _intact(V, "V")


FU = _kinds(BR.FUSED)


@pytest.mark.parametrize("kind,n,nv", FU, ids=_ids(FU))
def test_fused_axpy_dot(lib, dev, kind, n, nv):
    """every instantiation 1..32 on its own"""
    BR.need_real(kind)
    d, ldv = _data("fused", kind, n, nv), BR.even(n) + 64
    V, w = _basis(d, ldv, dev), _vec(d.w, dev)
    h2 = _fused(lib, d, V, ldv, w)
    BR.check_guards(w.back(), n, "w")
    BR.check_fused(d, w.vector(n), h2)
    _intact(V, "V")


# ------------------------------------------------------------------------------------------------------------ element-wise
AX = _kinds(BR.AXPBY_N)


@pytest.mark.parametrize("kind,n", AX, ids=_ids(AX))
def test_axpby(lib, dev, kind, n):
    BR.need_real(kind)
    d = _data("axpby", kind, n)
    x, y = _vec(d.x, dev), _vec(d.y, dev)
    _ok(lib.lib.nk_vec_axpby(lib.h, n, d.a, x.p, d.b, y.p))
    BR.check_guards(y.back(), n, "y")
    BR.check_axpby(d, y.vector(n))
    _intact(x, "x")


@pytest.mark.parametrize("kind,n", AX, ids=_ids(AX))
def test_axpy(lib, dev, kind, n):
    BR.need_real(kind)
    d = _data("axpy", kind, n)
    x, y = _vec(d.x, dev), _vec(d.y, dev)
    _ok(lib.lib.nk_axpy(lib.h, n, d.a, x.p, y.p))
    BR.check_guards(y.back(), n, "y")
    BR.check_axpby(d, y.vector(n))
    _intact(x, "x")


@pytest.mark.parametrize("a", BR.FILL_VALUES, ids=[repr(a) for a in BR.FILL_VALUES])
@pytest.mark.parametrize("n", BR.FILL_N)
def test_fill(lib, dev, n, a):
    """the bit pattern of a, −0.0 included, in every element and nowhere else"""
    y = _vec(np.full(n, 7.0), dev)
    _ok(lib.lib.nk_vec_fill(lib.h, n, a, y.p))
    back = y.back()
    BR.check_guards(back, n, "y")
    bad = np.flatnonzero(BR.bits(back[BR.PRE:BR.PRE + n]) != BR.bits(np.array([a]))[0])
    assert bad.size == 0, f"fill({a!r}): {bad.size} of {n} elements hold other bits, first at {bad[0]}: {back[BR.PRE + bad[0]]!r}"


def _axpby_special(lib, dev, a, x, b, y, alias=False):
    """y after nk_vec_axpby(a, x, b, y); alias: x is y"""
    yv = _vec(y, dev)
    xv = yv if alias else _vec(x, dev)
    _ok(lib.lib.nk_vec_axpby(lib.h, len(y), a, xv.p, b, yv.p))
    BR.check_guards(yv.back(), len(y), "y")
    if not alias:
        _intact(xv, "x")
    return yv.vector(len(y))


def _same_bits(got, want, what):
    bad = np.flatnonzero(BR.bits(got) != BR.bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


@pytest.mark.parametrize("n", [1, 2, 1025, BR._p(22) + 5])
def test_axpby_zero_coefficients_and_aliasing(lib, dev, n):
    """A coefficient that is exactly zero, of either sign, means that its operand is not read; both zero store +0.0; x may
    be y. (Julia's rmul!(y, a) is axpby!(0, y, a, y), and a copy into a buffer that held a NaN is axpby(1, x, 0, y).)"""
    d = _data("axpby", "real", n)
    x, y = d.x.copy(), d.y.copy()
    poison = x.copy()
    poison[0] = NAN
    if n > 2:
        poison[[n - 1, n // 2]] = [INF, -INF]
    ypoison = y.copy()
    ypoison[[0, n - 1]] = NAN
    for zero in (0.0, -0.0):
        _same_bits(_axpby_special(lib, dev, zero, poison, -1.75, y), -1.75 * y, "a = 0: y = b·y, x not read")
        _same_bits(_axpby_special(lib, dev, zero, poison, 1.0, y), y, "a = 0, b = 1: y stays")
        _same_bits(_axpby_special(lib, dev, 1.0, x, zero, ypoison), x, "b = 0: y = a·x, a copy")
        _same_bits(_axpby_special(lib, dev, 0.375, x, zero, ypoison), 0.375 * x, "b = 0: y = a·x, y not read")
        for zero2 in (0.0, -0.0):
            _same_bits(_axpby_special(lib, dev, zero, poison, zero2, ypoison), np.zeros(n), "a = b = 0: +0.0")
    # the same through nk_axpy: a = 0 leaves y alone whatever x holds
    yv, xv = _vec(y, dev), _vec(poison, dev)
    _ok(lib.lib.nk_axpy(lib.h, n, 0.0, xv.p, yv.p))
    _same_bits(yv.back(), yv.host, "axpy with a = 0")
    # x == y: scale in place keeps Inf and NaN and gives 2.5·y_i elsewhere; a scaled copy onto itself; a, b ≠ 0
    special = y.copy()
    special[0] = INF
    if n > 2:
        special[[n - 1, n // 2]] = [NAN, -INF]
    got = _axpby_special(lib, dev, 0.0, None, 2.5, special, alias=True)
    _same_bits(got[np.isfinite(special)], 2.5 * special[np.isfinite(special)], "rmul!: finite entries")
    assert np.array_equal(np.isnan(got), np.isnan(special)) and np.array_equal(got[np.isinf(special)], special[np.isinf(special)])
    _same_bits(_axpby_special(lib, dev, -3.0, None, 0.0, y, alias=True), -3.0 * y, "x == y, b = 0")
    d2 = BR.data("axpby", "real", n)
    d2.x = d2.y
    BR.check_axpby(d2, _axpby_special(lib, dev, d.a, None, d.b, d2.y, alias=True))
    e = BR.data("axpby", "exact", n)
    e.x = e.y
    BR.check_axpby(e, _axpby_special(lib, dev, e.a, None, e.b, e.y, alias=True))


# ---------------------------------------------------------------------------------------- stale partials, reproducibility
def _run(lib, dev, d):
    """the entry point of d.entry on fresh device copies; returns everything it gives back, as bits"""
    e, n = d.entry, d.n
    if e in ("dot", "nrm2", "norm_inf"):
        x, y = _vec(d.x, dev), _vec(d.y, dev)
        return [np.array([_reduce(lib, e, x, y, n)])]
    ldv = BR.even(n) + 64
    V, w = _basis(d, ldv, dev), _vec(d.w, dev)
    if e == "multidot":
        return [_multidot(lib, d, V, ldv, w)]
    if e == "multiaxpy":
        r = _multiaxpy(lib, d, V, ldv, w, True)
        return [w.vector(n), np.array([r])]
    h2 = _fused(lib, d, V, ldv, w)
    return [w.vector(n), h2]


def _check(d, out):
    if d.entry == "dot":
        BR.check_dot(d, out[0][0])
    elif d.entry == "nrm2":
        BR.check_nrm2(d, out[0][0])
    elif d.entry == "norm_inf":
        BR.check_norm_inf(d, out[0][0])
    elif d.entry == "multidot":
        BR.check_multidot(d, out[0])
    elif d.entry == "multiaxpy":
        BR.check_multiaxpy(d, out[0], out[1][0])
    else:
        BR.check_fused(d, out[0], out[1])


@pytest.mark.parametrize("entry,n,nv", BR.LARGEST, ids=_ids(BR.LARGEST))
def test_small_after_large_and_reproducible(lib, dev, entry, n, nv):
    """ctx->d_partials is shared by every reduction and its live length is the grid of the last launch: n = 3 after the largest
    case must not see what that left behind, and the largest case gives the same bits when it runs again"""
    BR.need_real("real")
    big, small = BR.data(entry, "real", n, nv), BR.data(entry, "exact", 3, nv)
    first = _run(lib, dev, big)
    _check(big, first)
    _check(small, _run(lib, dev, small))
    again = _run(lib, dev, big)
    for a, b in zip(first, again):
        _same_bits(b, a, f"{entry}: the second run of the same call")


# ------------------------------------------------------------------------------------------------- argument errors, n = 0
def test_argument_errors_launch_nothing(lib, dev):
    """a nonzero code, w as it was"""
    n, ldv = 64, 64
    d = BR.data("multidot", "exact", n, 2)
    V = Vec(np.full(BR.PRE + 66 * (ldv + 2) + BR.POST, 1.0), dev)       # room for whatever a missing check would read
    w = _vec(d.w, dev)
    hs = _arr(np.ones(66))
    out = _dbl(70)
    L = lib.lib
    calls = {
        "multidot nv = 65": lambda: L.nk_multidot(lib.h, n, 65, V.p, ldv, w.p, out),
        "multidot nv = -1": lambda: L.nk_multidot(lib.h, n, -1, V.p, ldv, w.p, out),
        "multiaxpy nv = 65": lambda: L.nk_multiaxpy(lib.h, n, 65, V.p, ldv, hs, w.p, None),
        "multiaxpy nv = -1": lambda: L.nk_multiaxpy(lib.h, n, -1, V.p, ldv, hs, w.p, None),
        "fused nv = 0": lambda: L.nk_fused_axpy_dot(lib.h, n, 0, V.p, ldv, hs, hs, w.p, out),
        "fused nv = 33": lambda: L.nk_fused_axpy_dot(lib.h, n, 33, V.p, ldv, hs, hs, w.p, out),
        "multidot odd ldv": lambda: L.nk_multidot(lib.h, n, 2, V.p, ldv + 1, w.p, out),
        "multiaxpy odd ldv": lambda: L.nk_multiaxpy(lib.h, n, 2, V.p, ldv + 1, hs, w.p, None),
        "fused odd ldv": lambda: L.nk_fused_axpy_dot(lib.h, n, 2, V.p, ldv + 1, hs, hs, w.p, out),
        "dot n = -1": lambda: L.nk_dot(lib.h, -1, w.p, w.p, out),
        "nrm2 n = -1": lambda: L.nk_nrm2(lib.h, -1, w.p, out),
        "norm_inf n = -1": lambda: L.nk_norm_inf(lib.h, -1, w.p, out),
        "axpy n = -1": lambda: L.nk_axpy(lib.h, -1, 2.0, V.p, w.p),
        "axpby n = -1": lambda: L.nk_vec_axpby(lib.h, -1, 2.0, V.p, 3.0, w.p),
        "fill n = -1": lambda: L.nk_vec_fill(lib.h, -1, 2.0, w.p),
        "multiaxpy n = -1": lambda: L.nk_multiaxpy(lib.h, -1, 2, V.p, ldv, hs, w.p, None),
    }
    for what, call in calls.items():
        assert call() != 0, f"{what} was accepted"
        _intact(w, f"{what}: w")
    _ok(L.nk_multidot(lib.h, n, 2, V.p, ldv, w.p, out))                # the context still works
    assert out[0] == float(np.sum(d.w))


def test_empty_vectors_may_be_null(lib):
    """n = 0 with NULL vectors: a no-op, and 0 from every reduction"""
    L, r = lib.lib, C.c_double(NAN)
    for call in (lambda: L.nk_dot(lib.h, 0, None, None, C.byref(r)), lambda: L.nk_nrm2(lib.h, 0, None, C.byref(r)),
                 lambda: L.nk_norm_inf(lib.h, 0, None, C.byref(r)),
                 lambda: L.nk_multiaxpy(lib.h, 0, 3, None, 0, _arr([1.0, 2.0, 3.0]), None, C.byref(r))):
        r.value = NAN
        _ok(call())
        assert r.value == 0.0 and not np.signbit(r.value)
    _ok(L.nk_axpy(lib.h, 0, 2.0, None, None))
    _ok(L.nk_vec_axpby(lib.h, 0, 2.0, None, 3.0, None))
    _ok(L.nk_vec_fill(lib.h, 0, 2.0, None))
    _ok(L.nk_multiaxpy(lib.h, 0, 3, None, 0, _arr([1.0, 2.0, 3.0]), None, None))
    h = _dbl(4)
    _ok(L.nk_multidot(lib.h, 0, 3, None, 0, None, h))
    assert list(h[:3]) == [0.0, 0.0, 0.0]
    h2 = _dbl(4)
    _ok(L.nk_fused_axpy_dot(lib.h, 0, 3, None, 0, _arr([1.0, 2.0, 3.0]), _arr([1.0, 2.0, 3.0]), None, h2))
    assert list(h2[:4]) == [0.0, 0.0, 0.0, 0.0]
