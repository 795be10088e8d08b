"""The shared Chebyshev iteration (csrc/nk_cheb.hip: nk_cheb_run) on its own, through the development hook nk_cheb_test, against
the same iteration driven by hand — equal bits. The first step is elementwise, so NumPy float64 is exact; a fused later step is
one nk_spmv_epilogue_test(mode 1) call with the coefficients of the Python recurrence (tests/cheb_reference.py); an unfused one
is the exported nk_spmv and the elementwise update in NumPy. Sizes: 1 and 2 rows, 257 (odd: the double2 tail of the unfused
step), 529 (more than one workgroup of the elementwise kernels). Steps 1, 2, 3, 6 cover both parities of the d ping-pong."""
import ctypes as C
import functools

import numpy as np
import pytest

import cheb_reference

pytestmark = pytest.mark.gpu

GUARD = 8                                       # doubles on either side of every array handed to the hook
CANARY = np.float64(-6.02214076e23)
STEPS = (1, 2, 3, 6)


def _tridiagonal(n, rng):
    rows = [[(i + o, (2.5 + 0.5 * rng.random()) if o == 0 else (-1.0 + 0.1 * rng.random())) for o in (-1, 0, 1) if 0 <= i + o < n]
            for i in range(n)]
    return rows


def _laplacian(ns, rng):
    rows = []
    for j in range(ns):
        for i in range(ns):
            row = [(i + ns * j, 4.0 + 0.5 * rng.random())]
            row += [(ii + ns * jj, -1.0 + 0.1 * rng.random()) for ii, jj in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1))
                    if 0 <= ii < ns and 0 <= jj < ns]
            rows.append(sorted(row))
    return rows


MATRICES = {
    "1x1": lambda rng: [[(0, 3.0)]],
    "2x2": lambda rng: [[(0, 4.0), (1, -1.0)], [(0, -2.0), (1, 5.0)]],
    "tridiagonal257": lambda rng: _tridiagonal(257, rng),
    "laplacian23": lambda rng: _laplacian(23, rng),
}


def _csr(rows):
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    col = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return rowptr, col, val


@functools.lru_cache(maxsize=None)
def _hooks():
    """development hooks: exported, not in the public header, so not in _lib.SIGNATURES"""
    from nonlinearsolve_jl_amd import _lib as L
    lib = L.lib()
    D, P, I = C.c_double, C.c_void_p, C.c_int
    lib.nk_cheb_test.restype = I
    lib.nk_cheb_test.argtypes = [P, I, I, I, D, D, P, P, P, P, P, P, C.POINTER(I)]
    lib.nk_spmv_epilogue_test.restype = I
    lib.nk_spmv_epilogue_test.argtypes = [P, I, P, P, P, P, P, P, D, D, D, P]
    return lib, L.check


def _guarded(values):
    whole = np.full(values.size + 2 * GUARD, CANARY)
    whole[GUARD:GUARD + values.size] = values
    return whole, whole[GUARD:GUARD + values.size]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b, what):
    bad = np.flatnonzero(_bits(a) != _bits(b))
    assert bad.size == 0, f"{what}: {bad.size} of {np.size(a)} entries differ, first at {bad[0]}: {a[bad[0]]!r} != {b[bad[0]]!r}"


def _fused_step(A, d, r, x, dinv, c1, c2):
    """one mode-1 row epilogue: r −= A d; d' = c1 d + c2 [dinv·]r; x += d'"""
    lib, check = _hooks()
    d, r, x, dnew = np.ascontiguousarray(d), r.copy(), x.copy(), np.empty_like(d)
    p = lambda a: None if a is None else a.ctypes.data
    check(lib.nk_spmv_epilogue_test(A._h, 1, p(d), None, p(r), p(dnew), p(x), p(dinv), c1, c2, 0.0, None))
    return dnew, r, x


@pytest.mark.parametrize("path", ["fused", "fused_dinv", "unfused"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_driver_equals_the_iteration_by_hand(nls, name, path):
    lib, check = _hooks()
    rng = np.random.default_rng(len(name) + 10 * len(path))
    rowptr, col, val = _csr(MATRICES[name](rng))
    n = rowptr.size - 1
    A = nls.CSRMatrix.from_arrays(rowptr, col, val)
    rowof = np.repeat(np.arange(n), np.diff(rowptr))
    diag = np.zeros(n)
    diag[rowof[col == rowof]] = val[col == rowof]
    dinv = np.ascontiguousarray(1.0 / diag) if path == "fused_dinv" else None
    absrow = np.bincount(rowof, weights=np.abs(val), minlength=n)
    lmax = float(np.max(absrow / np.abs(diag) if dinv is not None else absrow))
    lmin = lmax / 4.0
    fused = path != "unfused"
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    for steps in STEPS:
        inv_theta, coef = cheb_reference.coefficients(lmin, lmax, steps)
        for zero in (True, False):
            what = f"{name} {path} steps {steps} {'from zero' if zero else 'from x0'}"
            # ---- by hand
            r = b.copy() if zero else b - A.matvec(x0)
            d = (dinv * r if dinv is not None else r) * inv_theta
            x = d.copy() if zero else x0 + d
            other = None                                   # what the second buffer holds: the previous d (fused) or A d (unfused)
            for c1, c2 in coef:
                if fused:
                    other, (d, r, x) = d, _fused_step(A, d, r, x, dinv, c1, c2)
                else:
                    other = A.matvec(d)
                    r = r - other
                    d = c1 * d + c2 * r
                    x = x + d
            # ---- the driver; from zero neither x nor r is read: they arrive as NaN
            bufs = {"b": _guarded(b), "x": _guarded(np.full(n, np.nan) if zero else x0),
                    "r": _guarded(np.full(n, np.nan) if zero else b - A.matvec(x0)),
                    "d": _guarded(np.full(n, CANARY)), "t": _guarded(np.full(n, CANARY))}
            if dinv is not None:
                bufs["dinv"] = _guarded(dinv)
            ptr = lambda k: bufs[k][1].ctypes.data if k in bufs else None
            last_in_t = C.c_int(-1)
            check(lib.nk_cheb_test(A._h, steps, int(zero), int(fused), lmin, lmax, ptr("b"), ptr("dinv"), ptr("x"), ptr("r"), ptr("d"),
                                   ptr("t"), C.byref(last_in_t)))
            assert last_in_t.value == (1 if fused and (steps - 1) % 2 == 1 else 0), what
            last, second = ("t", "d") if last_in_t.value else ("d", "t")
            _same(bufs["x"][1], x, what + ": x")
            _same(bufs["r"][1], r, what + ": r")
            _same(bufs[last][1], d, what + ": the last d")
            _same(bufs[second][1], np.full(n, CANARY) if other is None else other, what + ": the second buffer")
            _same(bufs["b"][1], b, what + ": b")
            for k, (whole, _) in bufs.items():
                edge = np.concatenate([whole[:GUARD], whole[-GUARD:]])
                _same(edge, np.full(2 * GUARD, CANARY), what + f": guard words of {k}")
    A.close()
