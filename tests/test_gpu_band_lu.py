"""The right-looking band LU (csrc/nk_band.hip: k_band_fill, k_band_step, k_band_sweep) called directly through
nls.BandedLU and measured against the long-double unpivoted LU of tests/band_lu_reference.py — the same operation, so the
bounds can be tight: backward error ≤ 256 u and forward error ≤ 64 κ∞ u (a correct float64 unpivoted LU stays at ≤ 21 u and
≤ 5.5 κu). The Newton driver's a-posteriori check (1e-8 after one refinement step, then a GMRES fallback) and the multigrid's
V-cycle hide anything the kernel gets slightly wrong; these tests do not.

Every case asserts that the factorisation object runs on the band LU: the router sends matrices of four or more block rows of
order b (the bandwidth rounded up to 32) to block cyclic reduction, so the default-routed shapes here keep n ≤ 3b, and the long
chains run in a child process with NK_DIRECT=band (the variable is read once per process)."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import band_lu_reference as BR
from oracle import reference_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blk(kl, ku):
    return ((max(kl, ku, 1) + 31) // 32) * 32


def _factor(nls, J, engine="band_lu"):
    A = nls.CSRMatrix.from_scipy(sp.csr_matrix(J))
    F = nls.BandedLU(A)
    info = F.info()
    assert info["engine"] == engine, info
    assert (info["kl"], info["ku"]) == BR.bandwidths(J), info
    return A, F


@functools.lru_cache(maxsize=None)
def _case(key):
    """(J, b, x_ref, κ∞) of a named, seeded case; the long-double reference is computed once per module."""
    family, n, kl, ku, seed = key
    J = _FAMILIES[family](n, kl, ku, seed)
    x_true = np.random.default_rng(seed + 7).standard_normal(n)
    b = BR.manufactured(J, x_true)
    return J, b, BR.reference_solve(J, b), BR.cond_inf(J)


def _run(nls, key, nrhs=1):
    J, b, x_ref, kappa = _case(key)
    A, F = _factor(nls, J)
    try:
        x = F.solve(b)
        BR.check_solution(J, x, b, x_ref, kappa, str(key))
        rng = np.random.default_rng(99)
        for _ in range(nrhs - 1):       # factor once, solve many
            b2 = BR.manufactured(J, rng.standard_normal(J.shape[0]))
            BR.check_solution(J, F.solve(b2), b2, BR.reference_solve(J, b2), kappa, f"{key} another right-hand side")
    finally:
        F.close()
        A.close()


# ------------------------------------------------------------------------------------------------------------ families
def _spd(n, kl, ku, seed):
    """B Bᵀ + δI with B lower banded of width kl (= ku) and one zero column, δ = 1e-6 ‖B Bᵀ‖∞: κ∞ ≈ 1e6 … 1e8, multipliers
    O(1) (no dominant diagonal damps a wrong L21 / U12 term)."""
    assert kl == ku
    w = min(kl, n - 1)
    rng = np.random.default_rng(seed)
    B = sp.diags([rng.standard_normal(n - k) for k in range(w + 1)], [-k for k in range(w + 1)], shape=(n, n)).tolil()
    if n > 1:
        B[:, n // 2] = 0.0
    B = sp.csr_matrix(B)
    G = (B @ B.T).tocsr()
    delta = 1e-6 * BR.norm_inf(G)
    return (G + sp.identity(n) * delta).tocsr()


def _outer(n, kl, ku, seed):
    """Only the diagonal and the outermost diagonals −kl and +ku: everything in between is fill-in (band-edge masks)."""
    rng = np.random.default_rng(seed)
    kl, ku = min(kl, n - 1), min(ku, n - 1)
    d = {0: 4.0 + rng.random(n)}
    if kl:
        d[-kl] = rng.uniform(-1.0, 1.0, n - kl)
    if ku:
        d[ku] = rng.uniform(-1.0, 1.0, n - ku)
    return sp.diags(list(d.values()), list(d.keys()), shape=(n, n)).tocsr()


_FAMILIES = {"dominant": BR.dominant_band, "spd": _spd, "outer": _outer}


PAIRS = [(0, 0), (0, 40), (40, 0), (1, 1), (31, 31), (32, 32), (33, 33), (3, 48), (3, 49), (48, 3), (255, 255), (256, 256),
         (257, 257), (300, 40), (40, 500), (447, 447), (447, 512)]


def _sizes(kl, ku):
    b = _blk(kl, ku)
    return sorted({1, 2, 31, 32, 33, 64, 65, 2 * b + 17, 3 * b})


@pytest.mark.parametrize("kl,ku", PAIRS)
def test_band_lu_shapes_diagonally_dominant(nls, kl, ku):
    """Every n of the default routing's range for each bandwidth pair: one block (n ≤ 32), two, three, a partial last panel
    whose band runs past n (2b + 17) and 3b; block counts of every residue mod 4. Bands wider than 32 take the update
    workgroups, kl > 256 the second 256-row block of the panel update and L21, kl or ku > 256 the 512-thread sweeps."""
    seen = set()
    for n in _sizes(kl, ku):
        key = ("dominant", n, kl, ku, 1000 + n + kl + 7 * ku)
        J = _case(key)[0]
        shape = (n,) + BR.bandwidths(J)
        if shape in seen:
            continue
        seen.add(shape)
        _run(nls, key)


def test_band_lu_shapes_cover_every_block_count_residue():
    counts = {(n + 31) // 32 for kl, ku in PAIRS for n in _sizes(kl, ku)}
    assert {c % 4 for c in counts} == {0, 1, 2, 3}
    # and every (n, kl, ku) is one the default routing sends to the band LU: fewer than four block rows of order b
    for kl, ku in PAIRS:
        for n in _sizes(kl, ku):
            b = _blk(min(kl, n - 1), min(ku, n - 1))
            assert (n + b - 1) // b < 4


@pytest.mark.parametrize("w", [1, 31, 32, 33, 255, 256, 257, 447])
def test_band_lu_spd_ill_conditioned(nls, w):
    b = _blk(w, w)
    # the wide bands at one size (the long-double reference is the cost there)
    for n in ([2 * b + 17] if w >= 255 else [2 * b + 17, 3 * b]):
        key = ("spd", n, w, w, 2000 + n + w)
        J, _b, _x, kappa = _case(key)
        assert BR.bandwidths(J) == (w, w)
        assert 1e6 <= kappa <= 1e8, kappa
        _run(nls, key)


@pytest.mark.parametrize("kl,ku", [p for p in PAIRS if p != (0, 0)])
def test_band_lu_outermost_diagonals_only(nls, kl, ku):
    n = 2 * _blk(kl, ku) + 17
    key = ("outer", n, kl, ku, 3000 + kl + ku)
    assert BR.bandwidths(_case(key)[0]) == (kl, ku)
    _run(nls, key)


# --------------------------------------------------------------------------------------------- sparse patterns in the band
def _bratu_strip(nx, ny, seed):
    """Bratu's 5-point Jacobian on an nx × ny strip (bandwidth nx, fill-in between ±1 and ±nx)."""
    T = lambda m: sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    u = 0.3 * np.random.default_rng(seed).standard_normal(nx * ny)
    h2 = 1.0 / (nx + 1) ** 2
    L = sp.kron(sp.identity(ny), T(nx)) + sp.kron(T(ny), sp.identity(nx))
    return (L - sp.diags(6.0 * h2 * np.exp(u))).tocsr()


def _pattern_cases():
    rng = np.random.default_rng(4)
    out = {}
    for ns in (8, 9):
        out[f"bratu{ns}"] = sp.csr_matrix(R.Bratu2D(ns, 6.0).jac(0.3 * rng.standard_normal(ns * ns)))
    for N in (4, 6):
        P = R.Brusselator2D(N)
        out[f"brusselator{N}"] = sp.csr_matrix(P.jac(1.0 + 0.1 * rng.standard_normal(P.n)))
    out["bratu_strip_100x3"] = _bratu_strip(100, 3, 5)
    out["bratu_strip_40x2"] = _bratu_strip(40, 2, 6)
    # rows 32 and 45 with NO stored diagonal: their pivots come from fill (the update of the previous panel, and the
    # elimination inside the diagonal block)
    M = BR.dominant_band(150, 40, 40, 8).tolil()
    for i in (32, 45):
        M[i, i - 1] = M[i - 1, i - 1]
        M[i - 1, i] = 0.5 * M[i - 1, i - 1]
        M[i, i] = 0.0
    M = sp.csr_matrix(M)
    M.eliminate_zeros()
    out["no_stored_diagonal"] = M
    return out


@pytest.mark.parametrize("name", ["bratu8", "bratu9", "brusselator4", "brusselator6", "bratu_strip_100x3", "bratu_strip_40x2",
                                  "no_stored_diagonal"])
def test_band_lu_sparse_patterns_with_fill(nls, name):
    J = _pattern_cases()[name]
    n = J.shape[0]
    if name == "no_stored_diagonal":
        d = J.diagonal()
        assert d[32] == 0.0 and d[45] == 0.0
    x_true = np.random.default_rng(11).standard_normal(n)
    b = BR.manufactured(J, x_true)
    x_ref = BR.reference_solve(J, b)
    A, F = _factor(nls, J)
    BR.check_solution(J, F.solve(b), b, x_ref, BR.cond_inf(J), name)
    F.close()
    A.close()


# ------------------------------------------------------------------------------------------------------------ long chains
_CHAIN_CODE = (
    "import sys, numpy as np, scipy.sparse as sp\n"
    "sys.path.insert(0, TESTS)\n"
    "import band_lu_reference as BR, nonlinearsolve_jl_amd as nls\n"
    "out = {}\n"
    "for n, kl, ku in CASES:\n"
    "    J = BR.dominant_band(n, kl, ku, n + kl + ku)\n"
    "    b = BR.manufactured(J, np.random.default_rng(n).standard_normal(n))\n"
    "    A = nls.CSRMatrix.from_scipy(J)\n"
    "    F = nls.BandedLU(A)\n"
    "    i = F.info()\n"
    "    out[f'engine_{n}'] = np.array([i['engine'] == 'band_lu', i['kl'], i['ku']])\n"
    "    out[f'x_{n}'] = F.solve(b)\n"
    "    F.close(); A.close()\n"
    "np.savez(OUT, **out)\n")

CHAINS = [(8192, 40, 40), (16384, 100, 100), (4099, 300, 30), (65536, 256, 256)]


@pytest.fixture(scope="module")
def chains():
    with tempfile.NamedTemporaryFile(suffix=".npz") as tf:
        code = _CHAIN_CODE.replace("TESTS", repr(os.path.join(ROOT, "tests"))).replace("CASES", repr(CHAINS)).replace(
            "OUT", repr(tf.name))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NK_DIRECT="band"), capture_output=True, text=True,
                           timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = np.load(tf.name)
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("n,kl,ku", CHAINS)
def test_band_lu_long_chains_forced_by_nk_direct(nls, chains, n, kl, ku):
    """Hundreds to thousands of dependent block columns on the band LU (nblk mod 4 = 0, and 1 for n = 4099, whose ku = 30 is
    below the block size). κ∞ is Varah's upper bound here: these matrices are too large to invert densely."""
    assert list(chains[f"engine_{n}"]) == [1, kl, ku]
    J = BR.dominant_band(n, kl, ku, n + kl + ku)
    b = BR.manufactured(J, np.random.default_rng(n).standard_normal(n))
    x = chains[f"x_{n}"]
    kappa = BR.cond_inf_dominant(J)
    if n * kl * ku <= 2e8:
        BR.check_solution(J, x, b, BR.reference_solve(J, b, dense=False), kappa, str((n, kl, ku)))
    else:
        # config C2's band: a long-double reference is too slow at this size — LAPACK's float64 band solver instead
        ab = np.zeros((kl + ku + 1, n))
        Cj = J.tocoo()
        ab[ku + Cj.row - Cj.col, Cj.col] = Cj.data
        xs = sla.solve_banded((kl, ku), ab, b)
        assert BR.backward_error(J, x, b) <= BR.BACKWARD_BOUND * BR.U64
        assert BR.forward_error(x, xs) <= BR.FORWARD_FACTOR * kappa * BR.U64


# ------------------------------------------------------------------------------------------- factor once, solve many
def test_band_lu_several_right_hand_sides(nls):
    _run(nls, ("dominant", 2 * 64 + 17, 40, 60, 41), nrhs=4)


def test_band_lu_host_and_device_memspace_agree_bitwise_and_may_alias(nls, dev):
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    J, b, x_ref, kappa = _case(("dominant", 3 * 320, 300, 40, 5))
    A, F = _factor(nls, J)
    xh = F.solve(b)
    BR.check_solution(J, xh, b, x_ref, kappa, "host")
    bd = torch.tensor(b, device=dev)
    xd = F.solve(bd)
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
    # b and x the same device vector (mi355x_nk.h: "b and x may alias")
    v = bd.clone()
    L.check(L.lib().nk_lu_solve(F._h, C.c_void_p(v.data_ptr()), C.c_void_p(v.data_ptr()), L.DEVICE))
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy(), xh)
    assert np.array_equal(bd.cpu().numpy(), b)   # the non-aliased solve left b alone
    F.close()
    A.close()


def test_band_lu_refactor_equals_a_fresh_factorisation_and_recovers_from_a_breakdown(nls):
    J = BR.dominant_band(3 * 64, 50, 37, 12)
    J2 = J.copy()
    J2.data = J2.data * (1.0 + 0.05 * np.cos(np.arange(J2.nnz)))
    b = BR.manufactured(J2, np.random.default_rng(3).standard_normal(J.shape[0]))
    A, F = _factor(nls, J)
    x1 = F.solve(b)
    A.set_values(J2.data)
    F.factor()
    x_re = F.solve(b)
    A2, F2 = _factor(nls, J2)
    assert np.array_equal(x_re, F2.solve(b)) and not np.array_equal(x_re, x1)
    BR.check_solution(J2, x_re, b, BR.reference_solve(J2, b), BR.cond_inf(J2), "refactored")
    # a failed factorisation on the same object, then a good one: the failure flag is reset
    bad = J2.copy().tolil()
    bad[70, 70] = np.nan
    A.set_values(sp.csr_matrix(bad).data)
    with pytest.raises(nls.NKError):
        F.factor()
    A.set_values(J2.data)
    F.factor()
    assert np.array_equal(F.solve(b), x_re)
    for o in (F, F2, A, A2):
        o.close()


# ------------------------------------------------------------------------------------------------- breakdown reporting
def _breakdown(kind, n=100):
    """A matrix whose unpivoted LU meets an exact zero / non-finite pivot, and the row where it does."""
    M = BR.dominant_band(n, 3, 40, 21).toarray()
    if kind in ("first", "middle", "last"):
        k = {"first": 5, "middle": 32 * 1 + 7, "last": n - 2}[kind]   # n = 100: the last panel holds rows 96 … 99
        M[k, :k + 1] = 0.0   # no multiplier reaches row k: its pivot is the zero on the diagonal
    elif kind == "cancel32":
        # [[2, 3], [4, 6]] on rows / columns 31, 32: row 31's update cancels the pivot of row 32 exactly (previous panel)
        k = 32
        M[31:33, :] = 0.0
        M[:, 31:33] = 0.0
        M[31, 31], M[31, 32], M[32, 31], M[32, 32] = 2.0, 3.0, 4.0, 6.0
    else:
        k = 60
        M[k, k] = np.inf if kind == "inf" else np.nan
    J = sp.csr_matrix(M)
    # same pattern as the full dominant band: the zeros stay stored entries, so the bandwidths do not change
    Jp = BR.dominant_band(n, 3, 40, 21)
    vals = sp.csr_matrix((np.asarray(M)[Jp.nonzero()], Jp.indices, Jp.indptr), shape=(n, n))
    return Jp, vals, k, J


@pytest.mark.parametrize("kind", ["first", "middle", "last", "cancel32", "inf", "nan"])
def test_band_lu_reports_breakdown(nls, kind):
    Jp, vals, k, J = _breakdown(kind)
    with pytest.raises(BR.ZeroPivot) as e:
        BR.reference_solve(J, np.ones(J.shape[0]))
    assert e.value.k == k
    A, F = _factor(nls, Jp)
    A.set_values(vals.data)
    with pytest.raises(nls.NKError):
        F.factor()
    F.close()
    A.close()


# ------------------------------------------------------------------------------------------------------ exponent range
@pytest.mark.parametrize("e", [1000, -1000])
def test_band_lu_exponent_range(nls, e):
    """2^e A x = b gives x scaled by 2^−e: the pivot reciprocal (v_rcp_f64 + two Newton steps) at the ends of the range."""
    J, b, x_ref, kappa = _case(("dominant", 2 * 64 + 17, 40, 40, 77))
    s = np.ldexp(1.0, e)
    Js = (J * s).tocsr()
    A, F = _factor(nls, J)
    x = F.solve(b)
    As, Fs = _factor(nls, Js)
    xs = Fs.solve(b)
    xr_s = np.asarray(x_ref, dtype=BR.LD) * BR.LD(np.ldexp(1.0, -e))
    BR.check_solution(Js, xs, b, xr_s, kappa, f"2^{e}")
    assert np.max(np.abs(np.ldexp(xs, e) - x)) <= 8 * BR.U64 * np.max(np.abs(x))
    for o in (F, Fs, A, As):
        o.close()


# ------------------------------------------------------------------------------------ kl > 447: block cyclic reduction
@pytest.mark.parametrize("n", [480, 977, 1440])
def test_lower_bandwidth_beyond_the_band_lu_goes_to_block_cyclic_reduction(nls, n):
    """kl = 460 does not fit the band LU's LDS panel (kl ≤ 447); with fewer than four block rows of order 480 such a matrix
    was routed there and refused. Block cyclic reduction takes it."""
    J = BR.dominant_band(n, 460, 200, n)
    assert BR.bandwidths(J) == (460, 200)
    b = BR.manufactured(J, np.random.default_rng(n).standard_normal(n))
    A, F = _factor(nls, J, engine="block_cyclic_reduction")
    assert F.info()["block"] == 480
    BR.check_solution(J, F.solve(b), b, BR.reference_solve(J, b), BR.cond_inf(J), f"kl=460 n={n}")
    F.close()
    A.close()


# ---------------------------------------------------------------------------------------------------------- end to end
def _wide_stencil_problem(nls, dev, n, kl, ku, seed):
    """F(u) = A u + 0.1 u³ − c with a diagonally dominant band A; J(u) = A + diag(0.3 u²) through jac / jac_prototype."""
    import torch
    A = BR.dominant_band(n, kl, ku, seed)
    A.sort_indices()
    c = np.linspace(0.5, 1.5, n) * BR.norm_inf(A) / 10
    proto = nls.CSRMatrix.from_scipy(A)
    Ad = nls.CSRMatrix.from_scipy(A)
    dpos = torch.tensor(np.flatnonzero(A.indices == np.repeat(np.arange(n), np.diff(A.indptr))), device=dev)
    base = torch.tensor(A.data, device=dev)
    cd = torch.tensor(c, device=dev)

    def F(du, u, p):
        Ad.matvec(u, out=du)
        du.add_(0.1 * u ** 3 - cd)

    def jac(nzval, u, p):
        nzval.copy_(base)
        nzval[dpos] += 0.3 * u * u

    prob = nls.NonlinearProblem(nls.NonlinearFunction(F, jac=jac, jac_prototype=proto), torch.zeros(n, dtype=torch.float64, device=dev))
    ref = R.FunctionProblem(lambda u: A @ u + 0.1 * u ** 3 - c, np.zeros(n), jac=lambda u: sp.csr_matrix(A + sp.diags(0.3 * u * u)))
    return prob, ref, (proto, Ad)


@pytest.mark.parametrize("n,kl,ku,engine", [(384, 100, 100, 0), (977, 460, 120, 1)])
def test_direct_newton_on_a_wide_band(nls, dev, n, kl, ku, engine):
    """`linsolve = nothing` NewtonRaphson on a user problem with a concrete banded J: (384, ±100) is three block rows of
    order 128 — the band LU, with update workgroups (ku > 32); kl = 460 used to fail at init and now runs on block cyclic
    reduction. No GMRES fallback may have happened, and every step factored its Jacobian once (njacs counts one more:
    the cache is built with J(u0), FirstOrder/src/solve.jl:171-186 — the reference's counts are asserted as they are)."""
    prob, ref, keep = _wide_stencil_problem(nls, dev, n, kl, ku, 31)
    sol = nls.solve(prob, nls.NewtonRaphson(), abstol=1e-10, maxiters=30)
    rs = R.solve(ref, R.NewtonRaphson(linsolve=None), abstol=1e-10, maxiters=30)
    assert sol.retcode == "Success" == R.RETCODE_NAMES[rs.retcode]
    assert sol.stats.gmres_iters == 0
    assert sol.stats.nfactors == sol.stats.nsolve == sol.stats.nsteps >= 2
    assert (sol.stats.nsteps, sol.stats.nf, sol.stats.njacs) == (rs.stats.nsteps, rs.stats.nf, rs.stats.njacs)
    u = sol.u.cpu().numpy()
    assert np.max(np.abs(u - rs.u)) <= 1e-12 * max(1.0, float(np.max(np.abs(rs.u))))
    # the same band through the factorisation object: the engine the solver ran on
    J = ref.jac(u)
    _A, _F = _factor(nls, J, engine=("band_lu", "block_cyclic_reduction")[engine])
    _F.close()
    _A.close()
    for o in keep:
        o.close()
