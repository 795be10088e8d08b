"""The CSR layer (csrc/nk_csr.hip) on its own, through the C ABI / CSRMatrix, against tests/csr_reference.py: the streaming SpMV
for every tile size and kernel variant, its row epilogues, the transposed product and colsumsq, the Gershgorin kernel and the
cache in front of it, the flags that say which value-dependent cache is stale, and the assembled JᵀJ + λD.

Every assertion is bit equality with a float64 sum in the promised order, or — where a whole workgroup reduces one long row in an
order of its own — the componentwise bound γ_k (|A||x|)_i against a long-double sum (derivations in csr_reference.py). No
max-norm tolerance. The environment switches are read when a matrix is created (the transpose is created at the first
rmatvec / colsumsq), so monkeypatch.setenv for the length of a test is enough."""
import ctypes as C
import functools

import numpy as np
import pytest

import csr_reference as CR
from oracle import reference_restatement as R

pytestmark = pytest.mark.gpu

VARIANTS = {"default": {}, "noremap": {"NK_SPMV_VARIANT": "2"}, "col32": {"NK_SPMV_COL32": "1"}}


def _env(monkeypatch, tile, variant="default"):
    for k in ("NK_SPMV_TILE", "NK_SPMV_VARIANT", "NK_SPMV_COL32"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NK_SPMV_TILE", str(tile))
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)


def _dev(nls, M):
    return nls.CSRMatrix.from_arrays(M.rowptr.astype(np.int32), M.col.astype(np.int32), M.val)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.flatnonzero(_bits(a) != _bits(b))
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} entries differ, first at {bad[0]}: {a[bad[0]]!r} != {b[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def _hooks():
    """The development hooks of csrc/nk_csr.hip (exported, not in the public header, so not in _lib.SIGNATURES)."""
    from nonlinearsolve_jl_amd import _lib as L
    lib = L.lib()
    D, P = C.c_double, C.c_void_p
    lib.nk_spmv_epilogue_test.restype = C.c_int
    lib.nk_spmv_epilogue_test.argtypes = [P, C.c_int, P, P, P, P, P, P, D, D, D, P]
    lib.nk_csr_gershgorin_test.restype = C.c_int
    lib.nk_csr_gershgorin_test.argtypes = [P, P]
    lib.nk_normal_plan_test.restype = C.c_int
    lib.nk_normal_plan_test.argtypes = [P, D, P, C.POINTER(C.c_int64), P, P, P]
    return lib, L.check


def _gersh(A):
    lib, check = _hooks()
    out = np.zeros(2)
    check(lib.nk_csr_gershgorin_test(A._h, out.ctypes.data))
    return float(out[0]), float(out[1])


# ------------------------------------------------------------------------------------------------------------------- SpMV
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("tile", CR.TILES)
@pytest.mark.parametrize("name", CR.CASES)
def test_spmv(nls, dev, monkeypatch, name, tile, variant):
    """Tile rows bit for bit, long rows within γ_k |A||x|; host and device vectors; every case × tile × {XCD remap, no remap,
    32-bit columns}. The 16-bit column path runs exactly where csr_reference.FITS16 says (edge16: offsets −32768 and +32767)."""
    import torch
    _env(monkeypatch, tile, variant)
    M, x = CR.case(name, tile), CR.vector(name, tile)
    A = _dev(nls, M)
    seq = CR.spmv_sequential(M, x)
    CR.check_rows(A.matvec(x), M, x, tile, f"{name} tile {tile} {variant} host", seq)
    yd = A.matvec(torch.tensor(x, device=dev))
    CR.check_rows(yd.cpu().numpy(), M, x, tile, f"{name} tile {tile} {variant} device", seq)
    out = torch.full((M.n,), 7.0, dtype=torch.float64, device=dev)
    A.matvec(torch.tensor(x, device=dev), out=out)      # every row is written, the empty ones with 0
    _same(out.cpu().numpy(), yd.cpu().numpy(), "out=")
    A.close()


@pytest.mark.parametrize("tile", CR.TILES)
@pytest.mark.parametrize("name", ["long", "ragged", "empty_run"])
def test_spmv_nonfinite_and_scaling(nls, monkeypatch, name, tile):
    """x[0] = NaN / Inf reaches exactly the rows that store column 0 (lanes beyond the block's non-zeros gather x[0] and must
    not let it out); a stored zero times Inf is NaN; powers of two scale the result exactly."""
    _env(monkeypatch, tile)
    M, x = CR.case(name, tile), CR.vector(name, tile, 1)
    A = _dev(nls, M)
    lng = CR.long_rows(M.rowptr, tile)
    stores0 = np.bincount(M.rowof[M.col == 0], minlength=M.n) > 0
    assert name == "empty_run" or (stores0.any() and not stores0.all())
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[0] = bad
        y, ref = A.matvec(xb), CR.spmv_sequential(M, xb)
        _same(y[~lng], ref[~lng], f"{name} x[0] = {bad}")
        assert np.array_equal(np.isfinite(y), ~stores0), f"{name} x[0] = {bad}: the non-finite rows are not the rows that store column 0"
        assert np.array_equal(np.isnan(y), np.isnan(ref))
    zc = M.col[M.val == 0.0]
    if zc.size:                                          # explicit zero × Inf = NaN, as IEEE and the reference have it
        xb = x.copy()
        xb[zc[0]] = np.inf
        y, ref = A.matvec(xb), CR.spmv_sequential(M, xb)
        _same(y[~lng], ref[~lng], f"{name} zero × Inf")
        hit = np.bincount(M.rowof[(M.col == zc[0]) & (M.val == 0.0)], minlength=M.n) > 0
        assert hit.any() and np.all(np.isnan(y[hit])) and np.array_equal(np.isnan(y), np.isnan(ref))
    y0 = A.matvec(x)
    for e in (300, -300):
        As = _dev(nls, M.with_values(np.ldexp(M.val, e)))
        _same(As.matvec(x), np.ldexp(y0, e), f"{name} 2^{e} A")
        _same(As.matvec(np.ldexp(x, e)), np.ldexp(y0, 2 * e), f"{name} 2^{e} A, 2^{e} x")
        As.close()
        _same(A.matvec(np.ldexp(x, e)), np.ldexp(y0, e), f"{name} 2^{e} x")
    A.close()


# ------------------------------------------------------------------------------------------------- transpose and colsumsq
@pytest.mark.parametrize("tile", CR.TILES)
@pytest.mark.parametrize("name", CR.CASES)
def test_transpose_and_colsumsq(nls, dev, monkeypatch, name, tile):
    """Aᵀ x and Σ_i a_ij²: ascending-row sequential sums bit for bit, a long column (a long row of the transpose) within γ_k."""
    import torch
    _env(monkeypatch, tile)
    M, x = CR.case(name, tile), CR.vector(name, tile, 2)
    T = M.transpose()[0]
    A = _dev(nls, M)
    CR.check_rows(A.rmatvec(x), T, x, tile, f"{name} tile {tile} Aᵀx")
    CR.check_rows(A.colsumsq(), CR.squared(M), np.ones(M.n), tile, f"{name} tile {tile} colsumsq")
    CR.check_rows(A.rmatvec(torch.tensor(x, device=dev)).cpu().numpy(), T, x, tile, f"{name} tile {tile} Aᵀx device, after colsumsq")
    CR.check_rows(A.matvec(x), M, x, tile, f"{name} tile {tile} A x after the transposed products")
    A.close()


# ------------------------------------------------------------------------------------------------------------ stale caches
def _fresh_products(nls, M, x):
    F = _dev(nls, M)
    out = F.rmatvec(x), F.matvec(x), F.colsumsq()
    F.close()
    return out


@pytest.mark.parametrize("route", ["set_values_host", "set_values_device", "raw_pointer", "csc_host", "csc_device"])
def test_transposed_values_follow_a_refresh(nls, dev, monkeypatch, route):
    """rmatvec (the transposed values are permuted once and kept), new values by every route a caller has, rmatvec and matvec
    again: both equal a freshly ingested matrix with the new values bit for bit; colsumsq (which leaves squares in the
    transposed array) in between in either order."""
    import torch
    _env(monkeypatch, 1024)
    M, x = CR.case("ragged", 1024), CR.vector("ragged", 1024, 3)
    colptr, rowval, perm = M.csc()
    if route.startswith("csc"):
        A = nls.CSRMatrix.from_csc(colptr + 1, rowval + 1, M.val[perm])
    else:
        A = _dev(nls, M)
    raw = A.values_device() if route == "raw_pointer" else None
    rng = np.random.default_rng(9)
    old = _fresh_products(nls, M, x)
    _same(A.rmatvec(x), old[0], f"{route}: first rmatvec")
    for rnd in range(3):
        new = rng.standard_normal(M.nnz)
        if route == "set_values_host":
            A.set_values(new)
        elif route == "set_values_device":
            A.set_values(torch.tensor(new, device=dev))
        elif route == "raw_pointer":
            raw.copy_(torch.tensor(new, device=dev))
            torch.cuda.synchronize()
        elif route == "csc_host":
            A.set_values_csc(new[perm])
        else:
            A.set_values_csc(torch.tensor(new[perm], device=dev))
        want = _fresh_products(nls, M.with_values(new), x)
        if rnd == 1:                                     # colsumsq first: the transposed array holds squares afterwards
            _same(A.colsumsq(), want[2], f"{route} round {rnd}: colsumsq before rmatvec")
        _same(A.rmatvec(x), want[0], f"{route} round {rnd}: rmatvec after new values")
        _same(A.matvec(x), want[1], f"{route} round {rnd}: matvec after new values")
        if rnd != 1:
            _same(A.colsumsq(), want[2], f"{route} round {rnd}: colsumsq after rmatvec")
        _same(A.rmatvec(torch.tensor(x, device=dev)).cpu().numpy(), want[0], f"{route} round {rnd}: rmatvec after colsumsq")
        _same(A.values(), new, f"{route} round {rnd}: values")
    A.close()


def test_transposed_values_follow_jac_values(nls):
    """The fill kernels of a built-in problem (nk_jac_values) as the refresh."""
    ns = 40
    rng = np.random.default_rng(4)
    x = rng.standard_normal(ns * ns)
    for make in (lambda: nls.Bratu2D(ns, 6.0), lambda: nls.Brusselator2D(20)):
        P = make()
        n = P.n_local
        xx = x[:n]
        J, F = P.jac_csr(), P.jac_csr()
        for rnd in range(3):
            u = 1.0 + 0.2 * rng.standard_normal(n)
            P.jac_values(u, J)
            P.jac_values(u, F)
            for k, (a, b) in enumerate(((J.rmatvec(xx), F.rmatvec(xx)), (J.matvec(xx), F.matvec(xx)))):
                _same(a, b, f"round {rnd} product {k}")
            F.close()
            F = P.jac_csr()                              # a fresh matrix every round: its transpose is built from current values
        J.close()
        F.close()


def _pt_cache(nls, ns):
    from nonlinearsolve_jl_amd import _lib as L
    cache = nls.init(nls.NonlinearProblem(nls.Bratu2D(ns, 6.0)),
                     nls.PseudoTransient(linsolve=nls.KrylovJL_GMRES(), alpha_initial=10.0, concrete_jac=True), abstol=1e-12, maxiters=50)
    J = nls.CSRMatrix(L.lib().nk_solver_jacobian(cache._h), cache.prob.ctx, owned=False)
    G = nls.GMRES.__new__(nls.GMRES)
    G._h = L.lib().nk_solver_gmres(cache._h)
    return cache, J, G


def _fresh_with(nls, ns, vals):
    F = nls.Bratu2D(ns, 6.0).jac_csr()
    F.set_values(vals)
    return F


def test_transposed_values_follow_the_diagonal_damping(nls):
    """PseudoTransient takes its step on J + α⁻¹ I, the shift added to the stored diagonal (nk_csr_add_to_diagonal_dev). A step
    that evaluates J refills it first, and the fill marks the transposed values stale on its own; so the damping is isolated
    by steps that RE-USE the Jacobian (recompute_jacobian=False): between two Aᵀx only α⁻¹ on the diagonal changes."""
    ns = 24
    cache, J, _G = _pt_cache(nls, ns)
    x = np.random.default_rng(6).standard_normal(ns * ns)
    cache.step()
    seen = [J.values().copy()]
    for i in range(3):
        F = _fresh_with(nls, ns, seen[-1])
        _same(J.rmatvec(x), F.rmatvec(x), f"step {i}: rmatvec")        # the transposed values are current from here on
        _same(J.matvec(x), F.matvec(x), f"step {i}: matvec")
        F.close()
        njacs = cache.stats.njacs
        cache.step(recompute_jacobian=False)
        assert cache.stats.njacs == njacs, "the step evaluated a Jacobian: the damping is not isolated"
        seen.append(J.values().copy())
        changed = np.flatnonzero(seen[-1] != seen[-2])
        assert changed.size == ns * ns, f"step {i}: {changed.size} values changed, expected the {ns * ns} diagonal entries"
    F = _fresh_with(nls, ns, seen[-1])
    _same(J.rmatvec(x), F.rmatvec(x), "last: rmatvec")
    F.close()


# --------------------------------------------------------------------------------------------------------------- epilogues
def _epilogue(A, n, mode, x, r=None, yacc=None, dinv=None, c1=0.0, c2=0.0, theta=0.0, out_scale=None):
    lib, check = _hooks()
    buf = dict(y=np.full(n, 3.25), r=None if r is None else np.array(r), dnew=np.full(n, -1.5),
               yacc=None if yacc is None else np.array(yacc))
    p = lambda a: None if a is None else a.ctypes.data
    os_ = None if out_scale is None else np.array([out_scale], dtype=np.float64)
    dv = None if dinv is None else np.ascontiguousarray(dinv)
    xx = np.ascontiguousarray(x)
    uses = {0: ("y",), 3: ("y",), 2: ("y", "r"), 4: ("r",), 1: ("r", "dnew", "yacc")}[mode]
    check(lib.nk_spmv_epilogue_test(A._h, mode, p(xx), *(p(buf[k]) if k in uses else None for k in ("y", "r", "dnew", "yacc")),
                                    p(dv), c1, c2, theta, p(os_)))
    return {k: buf[k] for k in uses if not (mode == 2 and k == "r")}, buf


@pytest.mark.parametrize("tile", CR.TILES)
@pytest.mark.parametrize("name", ["ragged", "long", "empty_run", "wide"])
def test_epilogues(nls, monkeypatch, name, tile):
    """Modes 0 … 4 of spmv_store_row on ragged rows, long rows, blocks of empty rows and 32-bit columns: the same epilogue applied
    to the sequential sum in float64, bit for bit on tile rows; long rows within the γ_k bound on s carried through the
    epilogue's further roundings (csr_reference.epilogue_bound). An empty row under mode 2 gives y = b."""
    _env(monkeypatch, tile)
    M = CR.case(name, tile)
    rng = np.random.default_rng(tile + len(name))
    x, r, yacc, dinv = (rng.standard_normal(M.n) for _ in range(4))
    A = _dev(nls, M)
    lng = CR.long_rows(M.rowptr, tile)
    s = CR.spmv_sequential(M, x)
    S = CR.spmv_longdouble(M, x)
    delta = CR.gamma(M.rowlen).astype(CR.LD) * CR.abs_spmv(M, x)
    kw = dict(c1=0.37, c2=-1.9, theta=2.5)
    for mode, extra in ((0, {}), (0, dict(out_scale=0.3)), (1, dict(yacc=yacc)), (1, dict(yacc=yacc, dinv=dinv)), (2, {}),
                        (3, {}), (3, dict(out_scale=-7.0)), (4, {})):
        got, buf = _epilogue(A, M.n, mode, x, r=r, **kw, **extra)
        ref = CR.epilogue(mode, s, x, r=r, **kw, **extra)
        refl = CR.epilogue(mode, S, x, r=r, **kw, **extra)
        bnd = CR.epilogue_bound(mode, delta, S, x, r=r, **kw, **extra)
        assert set(got) == set(ref)
        for key in got:
            what = f"{name} tile {tile} mode {mode} {sorted(extra)} {key}"
            _same(got[key][~lng], ref[key][~lng], what)
            err = np.abs(got[key][lng].astype(CR.LD) - refl[key][lng])
            assert np.all(err <= bnd[key][lng]), f"{what}: long rows {np.flatnonzero(lng)}: error {err} > {bnd[key][lng]}"
        if mode == 2:
            _same(buf["r"], r, "mode 2 leaves b alone")
            empty = M.rowlen == 0
            _same(got["y"][empty], r[empty], "mode 2 on an empty row is b")
    A.close()


# -------------------------------------------------------------------------------------------------------------- Gershgorin
@pytest.mark.parametrize("tile", CR.TILES)
@pytest.mark.parametrize("name", CR.CASES)
def test_gershgorin_of_a_fresh_matrix(nls, monkeypatch, name, tile):
    """{−lo, hi}: equal to the restatement where every row is a tile row; γ_{k+1} Σ|v| on a long row. Rows without a stored
    diagonal, empty rows, diagonal-only rows are in the cases."""
    _env(monkeypatch, tile)
    M = CR.case(name, tile)
    A = _dev(nls, M)
    CR.gershgorin_check(_gersh(A), M, tile, f"{name} tile {tile}")
    CR.gershgorin_check(_gersh(A), M, tile, f"{name} tile {tile} again")
    A.close()


def test_gershgorin_on_signs_and_missing_diagonals(nls, monkeypatch):
    """The radius takes |v|: all off-diagonal entries negative, and a matrix whose extreme discs belong to rows without a stored
    diagonal."""
    _env(monkeypatch, 1024)
    M = CR.case("ragged", 1024)
    for vals in (-np.abs(M.val), np.where(M.col == M.rowof, 0.01 * M.val, -np.abs(M.val) - 1.0)):
        Mv = M.with_values(vals)
        A = _dev(nls, Mv)
        CR.gershgorin_check(_gersh(A), Mv, 1024, "negative off-diagonals")
        A.close()


def _bratu_mat(ns, u, J):
    """The device Jacobian J as a Mat: the oracle's pattern with the device's values. That pattern and order are the device's
    is proved without a tolerance: J x equals the sequential sum over (pattern, J.values()) bit for bit for a random x."""
    import scipy.sparse as sp
    S = sp.csr_matrix(R.Bratu2D(ns, 6.0).jac(u))
    S.sort_indices()
    vals = J.values()
    assert S.nnz == vals.size
    M = CR.Mat(S.shape[0], S.indptr, S.indices, vals)
    x = np.random.default_rng(ns).standard_normal(M.n)
    _same(J.matvec(x), CR.spmv_sequential(M, x), "pattern and order of the device Jacobian")
    return M


@pytest.mark.parametrize("route", ["set_values", "raw_pointer", "jac_values"])
def test_gershgorin_cache_follows_the_values(nls, dev, route):
    """The Bratu fill kernel leaves per-block bounds that the first reader reduces (bounds_pending → bounds_valid). They are the
    discs of the values it wrote (any order of ≤ 5 terms: γ_6 Σ|v|); after new values by any route the pair is that of a fresh
    matrix with those values, bit for bit."""
    import torch
    ns = 64
    P = nls.Bratu2D(ns, 6.0)
    J = P.jac_csr()
    rng = np.random.default_rng(8)
    u = 0.3 * rng.standard_normal(ns * ns)
    P.jac_values(u, J)
    M = _bratu_mat(ns, u, J)
    pair = _gersh(J)                                     # through the pending partials
    assert _gersh(J) == pair                             # … and through the settled cache
    ref = CR.gershgorin_pair(M)
    bound = float(np.max(CR.gamma(M.rowlen + 1) * CR.segsum(M.rowptr, np.abs(M.val))))
    assert abs(pair[0] - ref[0]) <= bound and abs(pair[1] - ref[1]) <= bound, (pair, ref, bound)
    raw = J.values_device() if route == "raw_pointer" else None
    for rnd in range(2):
        if route == "jac_values":
            u2 = 0.3 * rng.standard_normal(ns * ns) + rnd
            P.jac_values(u2, J)
            M2 = _bratu_mat(ns, u2, J)
            got, ref2 = _gersh(J), CR.gershgorin_pair(M2)
            bound2 = float(np.max(CR.gamma(M2.rowlen + 1) * CR.segsum(M2.rowptr, np.abs(M2.val))))
            assert abs(got[0] - ref2[0]) <= bound2 and abs(got[1] - ref2[1]) <= bound2 and got != pair, (rnd, got, ref2, bound2)
            continue
        new = M.val * rng.uniform(0.5, 3.0, M.nnz)
        if route == "set_values":
            J.set_values(new if rnd == 0 else torch.tensor(new, device=dev))
        else:
            raw.copy_(torch.tensor(new, device=dev))
            torch.cuda.synchronize()
        F = _dev(nls, M.with_values(new))
        got, want = _gersh(J), _gersh(F)
        assert got == want == CR.gershgorin_pair(M.with_values(new)), (route, rnd, got, want)
        F.close()
    J.close()


def test_gershgorin_cache_follows_set_values_csc(nls):
    M = CR.case("small", 1024)
    colptr, rowval, perm = M.csc()
    A = nls.CSRMatrix.from_csc(colptr + 1, rowval + 1, M.val[perm])
    assert _gersh(A) == CR.gershgorin_pair(M)
    new = np.random.default_rng(2).standard_normal(M.nnz)
    A.set_values_csc(new[perm])
    assert _gersh(A) == CR.gershgorin_pair(M.with_values(new))
    A.close()


def test_gershgorin_cache_follows_the_diagonal_damping(nls):
    """The Bratu fill leaves bounds of J; PseudoTransient then moves the diagonal (nk_csr_add_to_diagonal_dev). After the step
    the bounds the cache hands out are those of the matrix as it stands, J + α⁻¹ I — a fresh matrix with its values, bit for
    bit — and so is the interval that step's linear solve placed its shifts on (the values have not changed since). Steps
    that evaluate J and steps that re-use it (only the shift changes)."""
    ns = 32
    cache, J, G = _pt_cache(nls, ns)
    u0 = np.asarray(cache.u).copy()
    for i, reuse in enumerate((False, False, True, True, False)):
        cache.step(recompute_jacobian=False) if reuse else cache.step()
        vals = J.values()
        F = _fresh_with(nls, ns, vals)
        want = _gersh(F)
        F.close()
        bs, newton, _bd = G.sstep_state()
        assert newton, "the solve built no Newton-basis blocks: no interval was taken"
        lo, hi = G.sstep_interval()
        assert (-lo, hi) == want, f"step {i}: the solve took {(-lo, hi)!r}, the damped matrix has {want!r}"
        assert _gersh(J) == want, f"step {i}: the cache hands out {_gersh(J)!r}, the damped matrix has {want!r}"
    assert want == CR.gershgorin_pair(_bratu_mat(ns, u0, J))           # (the oracle's pattern with the last step's values)


def _newton_cache(nls, prob):
    from nonlinearsolve_jl_amd import _lib as L
    cache = nls.init(nls.NonlinearProblem(prob), nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True),
                     abstol=1e-14, maxiters=50)
    G = nls.GMRES.__new__(nls.GMRES)
    G._h = L.lib().nk_solver_gmres(cache._h)
    return cache, G


@pytest.mark.parametrize("which", ["bratu64", "brusselator32"])
def test_interval_a_newton_solve_takes(nls, which):
    """NewtonRaphson with a concrete Jacobian on the default s-step path: the fill kernel's per-block partials, their reduction
    folded into the solve's begin kernel (nk_csr_take_pending_bounds), the speculative fill into the spare value set and the
    swap of the two sets. After each of 4 steps the interval the NEXT linear solve takes — observed by letting it take it:
    nk_gmres_get_sstep_interval after the following step — equals the oracle's gershgorin_interval of the oracle's Jacobian at
    the device's iterate, to 1e-13 of the interval's scale max(|lo|, |hi|) (the Jacobian values agree to 1e-13 of their
    largest, tests/test_gpu_kernels.py; this is that bound, not a new number). The first solve (J(u0), filled at init) too."""
    if which == "bratu64":
        prob, P = nls.Bratu2D(64, 6.0), R.Bratu2D(64, 6.0)
    else:
        prob, P = nls.Brusselator2D(32), R.Brusselator2D(32)
    cache, G = _newton_cache(nls, prob)
    for i in range(5):
        u_at = np.asarray(cache.u).copy()                # the iterate the next solve's Jacobian belongs to
        if 0 < i <= 2:
            assert not np.array_equal(u_at, u_prev), "the iterate did not move: the steps test nothing"
        cache.step()
        bs, newton, _bd = G.sstep_state()
        assert newton, f"step {i}: the solve built no Newton-basis blocks"
        lo, hi = G.sstep_interval()
        lo_o, hi_o = R.gershgorin_interval(P.jac(u_at))
        scale = max(abs(lo_o), abs(hi_o))
        print(f"{which} step {i}: device [{lo!r}, {hi!r}], oracle [{lo_o!r}, {hi_o!r}], "
              f"errors {abs(lo - lo_o) / scale:.2e} {abs(hi - hi_o) / scale:.2e} of the scale")
        assert abs(lo - lo_o) <= 1e-13 * scale and abs(hi - hi_o) <= 1e-13 * scale, (which, i, (lo, hi), (lo_o, hi_o))
        u_prev = u_at


# --------------------------------------------------------------------------------------------------------------- JᵀJ + λD
@pytest.mark.parametrize("name,lam,with_d", [("small", 0.0, False), ("small", 0.75, True), ("small", 0.75, False),
                                              ("exact_tile", 2.0, True), ("n1", 0.5, True)])
def test_normal_matrix(nls, monkeypatch, name, lam, with_d):
    """The assembled JᵀJ + λ diag(d): the pattern integer-exact with every diagonal position present (column 7 of `small` is
    empty: N[7, 7] is a stored entry that receives λ d_7 and nothing else), values bit for bit against the row-ordered sum;
    λ = 0 without d; λ > 0 without d adds nothing (nk_normal_plan_values: d may be NULL)."""
    _env(monkeypatch, 512)
    lib, check = _hooks()
    J = CR.case(name, 512)
    d = np.random.default_rng(3).uniform(0.5, 2.0, J.n) if with_d else None
    A = _dev(nls, J)
    nnz = C.c_int64(0)
    check(lib.nk_normal_plan_test(A._h, lam, None, C.byref(nnz), None, None, None))
    rp, col, val = np.zeros(J.n + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value)
    check(lib.nk_normal_plan_test(A._h, lam, None if d is None else d.ctypes.data, C.byref(nnz), rp.ctypes.data, col.ctypes.data,
                                  val.ctypes.data))
    rrp, rcol, rval = CR.normal_matrix(J, lam, d)
    assert np.array_equal(rp, rrp) and np.array_equal(col, rcol)
    _same(val, rval, f"{name} λ = {lam}")
    if name == "small":
        k = rp[7] + int(np.searchsorted(col[rp[7]:rp[8]], 7))
        assert col[k] == 7 and rp[8] - rp[7] == 1 and val[k] == (lam * d[7] if with_d else 0.0)
    A.close()
