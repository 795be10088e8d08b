"""tests/blas_reference.py kept honest without a GPU. For every case of the GPU test (the two ldv of a case share its data):

  * the exact-data case's worst partial sum is below 2⁵³, so "bit-equal to the int64 evaluation" is a fair demand;
  * three float64 evaluations in different orders — forward, reversed, and blocks of 512 summed pairwise, the columns of an
    update taken forward, backward and in pairs — pass the assertions the GPU test makes (real data: inside the bounds; exact
    data: the integer's bits), so the bounds do not reject a correct kernel;
  * each of these wrong results fails them, so they are not vacuous:
      drop    one element left out of a sum, or not updated by an element-wise kernel
      twice   one element counted, or updated, twice (sumdrop, sumtwice: in the sums of an updating kernel, its w being right)
      swap    two columns of V exchanged (two whose exchange changes the result at all; a case without such a pair says so)
      jbase   the second chunk of the multidot's column split starts at the first chunk's columns (nv > 16)
      past    the element after the n-th read into a sum (it is a guard, or the padding of a column: NaN), or written
      f32     accumulation in float32 — on real data only: on the exact data's small integers float32 is exact too, which is
              why the real data is there.
    norm_inf cannot notice a dropped element unless it is the maximum, so its drop removes a planted maximum, which is also
    what the GPU test plants at the edges of the launch geometry."""
import numpy as np
import pytest

import blas_reference as BR

ORDERS = ("forward", "reversed", "blocked")


def _ids(cases):
    return ["-".join(str(t) for t in c) for c in cases]


def _cases(entry, sizes):
    return [(entry, kind) + (s if isinstance(s, tuple) else (s, 0)) for kind in BR.KINDS for s in sizes]


ALL = (_cases("dot", BR.DOT_N) + _cases("nrm2", BR.DOT_N) + _cases("norm_inf", BR.NORM_INF_N) + _cases("multidot", BR.MULTIDOT)
       + _cases("multiaxpy", BR.MULTIAXPY) + _cases("fused", BR.FUSED) + _cases("axpby", BR.AXPBY_N) + _cases("axpy", BR.AXPBY_N))


# --------------------------------------------------------------------------------------------------------------- emulation
class Unexpressible(Exception):
    """the mutation changes nothing in this case (a handful of rows: every candidate term or update is zero or equal)"""


def _sum(t, order, mut=None):
    """Σ t in float64 in the given order; mut: one nonzero term dropped or counted twice, or float32 accumulation"""
    t = np.asarray(t, dtype=np.float64)
    if mut in ("drop", "twice"):                # (Σ w_new² of the exact data can hold zero terms)
        nz = np.flatnonzero(t)
        if nz.size == 0:
            raise Unexpressible
        k = nz[(2 * nz.size) // 3]
    if mut == "drop":
        t = np.delete(t, k)
    elif mut == "twice":
        t = np.append(t, t[k])
    if t.size == 0:
        return 0.0
    if mut == "f32":
        return float(np.cumsum(t.astype(np.float32), dtype=np.float32)[-1])
    if order == "forward":
        return float(np.cumsum(t)[-1])
    if order == "reversed":
        return float(np.cumsum(t[::-1])[-1])
    pad = (-t.size) % 512
    blocks = np.cumsum(np.concatenate([t, np.zeros(pad)]).reshape(-1, 512), axis=1)[:, -1]
    return float(np.sum(blocks))


def _ext(v):
    """the vector and the guard behind it, as a read one element past n sees them"""
    return BR.guarded(v)[BR.PRE:BR.PRE + len(v) + 1]


def _update(d, coef, order, mut=None, swap=None):
    """w − Σ_j coef_j V_j in float64, one rounding per operation, the columns in the order's sequence"""
    dt = np.float32 if mut == "f32" else np.float64
    V, w, coef = d.V.astype(dt), d.w.astype(dt), np.asarray(coef, dtype=dt).copy()
    if swap:
        coef[list(swap)] = coef[list(swap)[::-1]]
    js = list(range(d.nv))
    out = w.copy()
    if order == "reversed":
        js = js[::-1]
    if order == "blocked":
        for j in range(0, d.nv - 1, 2):
            out = out - (coef[j] * V[j] + coef[j + 1] * V[j + 1])
        js = js[d.nv - d.nv % 2:]
    for j in js:
        out = out - coef[j] * V[j]
    if mut in ("drop", "twice"):                # (at an element the update changes: small integers can cancel)
        changed = np.flatnonzero(out != w)
        if changed.size == 0:
            raise Unexpressible
        k = changed[(2 * changed.size) // 3]
        out[k] = w[k] if mut == "drop" else out[k] + (out[k] - w[k])
    return out.astype(np.float64)


def _swap_pair(d, coef):
    """two columns whose exchange changes w − Σ coef_j V_j somewhere"""
    for j in range(d.nv):
        for k in range(j + 1, d.nv):
            if coef[j] != coef[k] and np.any(d.V[j] != d.V[k]):
                return j, k
    raise Unexpressible


def _evaluate(d, order, mut=None):
    """the entry point's result as a correct kernel summing in `order` would give it, or with one mutation; returns the
    arguments of the entry's check_* function after d"""
    n, k, e = d.n, (2 * d.n) // 3, d.entry
    red = {"drop": "drop", "twice": "twice", "f32": "f32", "sumdrop": "drop", "sumtwice": "twice"}.get(mut)
    if e in ("dot", "nrm2"):
        x, y = (d.x, d.x if e == "nrm2" else d.y) if mut != "past" else (_ext(d.x), _ext(d.x if e == "nrm2" else d.y))
        s = _sum(x * y, order, red)
        return (np.sqrt(s),) if e == "nrm2" else (s,)
    if e == "norm_inf":
        x = d.x.copy() if mut != "past" else _ext(d.x)
        if mut == "drop":
            x = np.delete(x, k)
        return (float(np.max(np.abs(x), initial=0.0)) if not np.isnan(x).any() else float("nan"),)
    if e == "multidot":
        cols = list(range(d.nv))
        if mut == "swap":
            h = [float(np.dot(d.V[j], d.w)) for j in cols]
            pair = next(((j, q) for j in cols for q in cols[j + 1:] if h[j] != h[q]), None)
            if pair is None:
                raise Unexpressible
            cols[pair[0]], cols[pair[1]] = pair[1], pair[0]
        if mut == "jbase":
            (j0, n0), (j1, n1) = BR.chunks(d.nv)[:2]
            cols[j1:j1 + n1] = range(j0, j0 + n1)
        if mut == "past":
            Vx, wx = np.hstack([d.V, np.full((d.nv, 1), BR.guard_value())]), _ext(d.w)
            return (np.array([_sum(Vx[j] * wx, order) for j in cols]),)
        return (np.array([_sum(d.V[j] * d.w, order, red if j == cols[-1] else None) for j in cols]),)
    if e in ("multiaxpy", "fused"):
        coef = d.h if e == "multiaxpy" else d.h * d.s
        swap = _swap_pair(d, coef) if mut == "swap" else None
        w = _update(d, coef, order, mut if d.nv else None, swap)    # (sumdrop, sumtwice: w stays right)
        ss = _sum(w * w, order, red) if mut != "past" else _sum(_ext(w) ** 2, order)
        if e == "multiaxpy":
            return (w, ss)
        h2 = [d.s[j] * _sum(d.V[j] * w, order, red if (mut == "f32" or j == d.nv - 1) else None) for j in range(d.nv)]
        return (w, np.array(h2 + [ss]))
    if e in ("axpby", "axpy"):
        dt = np.float32 if mut == "f32" else np.float64
        x, y, a, b = d.x.astype(dt), d.y.astype(dt), dt(d.a), dt(d.b)
        out = a * x + b * y
        if mut == "drop":
            out[k] = y[k]
        elif mut == "twice":
            out[k] = out[k] + a * x[k]
        return (out.astype(np.float64),)
    raise KeyError(e)


CHECK = {"dot": BR.check_dot, "nrm2": BR.check_nrm2, "norm_inf": BR.check_norm_inf, "multidot": BR.check_multidot,
         "multiaxpy": BR.check_multiaxpy, "fused": BR.check_fused, "axpby": BR.check_axpby, "axpy": BR.check_axpby}


def _mutations(d):
    muts = ["drop", "twice", "past"]
    if d.entry == "norm_inf":
        muts = ["drop", "past"]
    if d.entry in ("axpby", "axpy"):
        muts = ["drop", "twice"]                # (a write past n is the guards' business: test_guards_notice_a_write)
    if d.entry in ("multidot", "multiaxpy", "fused") and d.nv >= 2:
        muts.append("swap")
    if d.entry == "multidot" and d.nv > BR.CHUNK:
        muts.append("jbase")
    if d.kind == "real" and d.entry != "norm_inf":   # (float32 holds the planted maximum exactly)
        muts.append("f32")
    if d.entry in ("multiaxpy", "fused"):
        muts += ["sumdrop", "sumtwice"]         # the reductions alone, behind a correct w
    return muts


# ------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("entry,kind,n,nv", ALL, ids=_ids(ALL))
def test_case(entry, kind, n, nv):
    BR.need_real(kind)
    assert BR.cap(entry, n, nv) < 2 ** 53
    d = BR.data(entry, kind, n, nv)
    if entry == "norm_inf":
        d.x[(2 * n) // 3] = np.copysign(16.0, d.x[(2 * n) // 3])   # the planted maximum (see above)
    for order in ORDERS:
        CHECK[entry](d, *_evaluate(d, order))
    swaps = 0
    for mut in _mutations(d):
        try:
            bad = _evaluate(d, "forward", mut)
        except Unexpressible:
            assert n <= 3
            continue
        swaps += mut == "swap"
        with pytest.raises(AssertionError):
            CHECK[entry](d, *bad)
    if n > 3 and nv >= 2:
        assert swaps == 1


def test_cap_is_the_worst_case():
    """the caps are reached by the all-extreme data and by nothing larger"""
    n, nv = 7, 5
    V, w, h, s = np.full((nv, n), 8.0), np.full(n, -8.0), np.full(nv, 4.0), np.full(nv, 4.0)
    assert BR.cap("dot", n) == np.sum(np.abs(V[0] * w))
    wn = w - h @ V
    assert BR.cap("multiaxpy", n, nv) == np.sum(wn * wn)
    wf = w - (h * s) @ V
    assert BR.cap("fused", n, nv) == max(np.sum(wf * wf), 4 * np.sum(np.abs(V[0] * wf)))
    assert BR.cap("fused", BR._p(19) + BR._p(17) + 3, 32) < 2 ** 53 and 4104 == 8 + 128 * 32


def test_chunks_are_the_librarys_split():
    """balanced chunks of at most 16 columns: 17 → 9 + 8, 31 → 16 + 15, 33 → 11 + 11 + 11, 49 → 13 + 12 + 12 + 12"""
    assert [c[1] for c in BR.chunks(17)] == [9, 8] and [c[1] for c in BR.chunks(31)] == [16, 15]
    assert [c[1] for c in BR.chunks(33)] == [11, 11, 11] and [c[1] for c in BR.chunks(49)] == [13, 12, 12, 12]
    assert BR.chunks(16) == [(0, 16)] and BR.chunks(64) == [(0, 16), (16, 16), (32, 16), (48, 16)] and BR.chunks(0) == []
    for nv in range(1, 65):
        ch = BR.chunks(nv)
        assert sum(c[1] for c in ch) == nv and max(c[1] for c in ch) <= 16 and all(ch[i][0] + ch[i][1] == ch[i + 1][0] for i in range(len(ch) - 1))
    # every instantiation 1..16 of the multidot kernel is some case's chunk
    assert {c[1] for _, nv in BR.MULTIDOT for c in BR.chunks(nv)} == set(range(1, 17))


def test_guards_notice_a_write():
    v = np.arange(1.0, 6.0)
    buf = BR.guarded(v)
    BR.check_guards(buf, 5, "untouched")
    assert np.isnan(buf[:BR.PRE]).all() and np.isnan(buf[BR.PRE + 5:]).all() and (BR.PRE * 8) % 16 == 0
    for at, val in ((BR.PRE + 5, 0.0), (BR.PRE - 1, 1.0), (len(buf) - 1, float("nan")), (BR.PRE + 5, -BR.guard_value())):
        bad = buf.copy()
        bad[at] = val                           # (an ordinary NaN, or the guard with its sign flipped, is a change too)
        with pytest.raises(AssertionError):
            BR.check_guards(bad, 5, "written")
    V = np.arange(1.0, 13.0).reshape(3, 4)
    for ldv in (4, 6):
        B = BR.guarded_basis(V, ldv)
        assert np.array_equal(B[BR.PRE:BR.PRE + 3 * ldv].reshape(3, ldv)[:, :4], V) and np.isnan(B).sum() == B.size - 12
        BR.check_unchanged(B, B.copy(), "basis")
        bad = B.copy()
        bad[BR.PRE + ldv - 1] = 7.0             # the last element of column 0, or of its padding
        with pytest.raises(AssertionError):
            BR.check_unchanged(bad, B, "basis")
    assert BR.guarded_basis(np.zeros((0, 5)), 6).size == BR.PRE + BR.POST


def test_even_ldv_and_case_lists():
    assert BR.even(4099) == 4100 and BR.even(2050) == 2050
    assert {nv for n, nv in BR.FUSED if n == 4099} == set(range(1, 33))
    assert {nv % 4 for n, nv in BR.MULTIAXPY} == {0, 1, 2, 3} and {0, 64} <= {nv for n, nv in BR.MULTIAXPY}
    assert all(at < n for n, at in BR.NORM_INF_NAN)
