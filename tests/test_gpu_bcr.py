"""Block cyclic reduction (csrc/nk_bcr.hip: k_bcr_fill, k_bcr_gemm, k_bcr_inv128<false|true>, k_bcr_gemv) called directly
through nls.BandedLU and measured against the long-double solve of tests/band_lu_reference.py: backward error
‖b − A x‖∞ / (‖A‖∞ ‖x‖∞) in units of u = 2⁻⁵³ and forward error in units of κ∞ u, per family and inversion kernel, with the
bounds of tests/bcr_reference.py — 8 × what a float64 NumPy restatement of the same algorithm reaches on the same cases
(dominant bands 128 u / 64 κu, SPD 32 u / 1 κu, Bratu 128 u / 0.125 κu, …), about four decades below the 1e-10 of
tests/test_gpu_direct.py. The Newton driver's residual check, refinement step and GMRES fallback hide what the engine gets
slightly wrong; these tests do not.

Every case asserts the engine, its block order and its number of levels. NK_BCR_PIVOT is read at every construction of a
factorisation object, so the inversion kernel is chosen per case: "never" = Gauss–Jordan on the diagonal (a breakdown
raises instead of switching the object over), "always" = row pivoting inside the 128-leaves."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import band_lu_reference as BR
import bcr_reference as B

pytestmark = pytest.mark.gpu


class _Factored:
    """CSR matrix + factorisation object on the engine under test, closed on exit."""

    def __init__(self, nls, monkeypatch, J, mode, block=None, levels=None):
        if mode == "auto":
            monkeypatch.delenv("NK_BCR_PIVOT", raising=False)
        else:
            monkeypatch.setenv("NK_BCR_PIVOT", mode)
        self.A = nls.CSRMatrix.from_scipy(sp.csr_matrix(J))
        try:
            self.F = nls.BandedLU(self.A)
        except Exception:
            self.A.close()
            raise
        info = self.info = self.F.info()
        assert info["engine"] == "block_cyclic_reduction", info
        assert (info["kl"], info["ku"]) == BR.bandwidths(J), info
        n, b = J.shape[0], B.block_order(info["kl"], info["ku"])
        assert info["block"] == b == (block or b), info
        assert info["levels"] == math.ceil(math.log2(-(-n // b))) + 1 == (levels or info["levels"]), info

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.F.close()
        self.A.close()


def _run(nls, monkeypatch, name, mode):
    """Factor the committed case on the given inversion kernel, solve, assert its bounds; returns (x, info)."""
    J, b, _x_ref, _kappa, blk, lev = B.problem(name)
    with _Factored(nls, monkeypatch, J, mode, blk, lev) as S:
        x = S.F.solve(b)
        B.check(name, mode, x)
        return x, S.info


# ------------------------------------------------------------------------------------------------------ every block order
def test_every_block_order_on_its_inversion_kernels(nls, monkeypatch):
    """b = 32 … 512, all 16: every branch of bcr_invert — direct (≤ 128), 128 + n2 (n2 = 32 … 128), 256 + n2 with n2 ≤ 128
    and with n2 = 160 … 256 (a second recursion). kl ≠ ku with the larger on either side, kl = b or ku = b exactly on eight
    of them: both pairs of triangular level-0 products see a full triangle, diagonal included. b ∈ {32, 128, 160, 256, 288,
    512} run on both inversion kernels; on these dominant matrices partial pivoting picks the diagonal, so the two do the
    same arithmetic up to the permuted store and their solutions agree to 4 u."""
    seen, kernels = set(), set()
    for b in B.ORDERS:
        xs = {}
        for mode in B.CASES[f"order{b}"]["modes"]:
            xs[mode], info = _run(nls, monkeypatch, f"order{b}", mode)
            seen.add(info["block"])
            kernels.add(mode)
        if len(xs) == 2:
            d = np.max(np.abs(xs["never"] - xs["always"])) / np.max(np.abs(xs["never"]))
            print(f"order{b}: never vs always {d / BR.U64:.2f} u")
            assert d <= 4 * BR.U64, (b, d / BR.U64)
    assert seen == set(range(32, 513, 32))
    assert kernels == {"never", "always"}


# ------------------------------------------------------------------------------------------------------ every level shape
def test_every_level_shape(nls, monkeypatch):
    """m = 4 … 33 block rows of order 32: odd and even counts at every level (an even row without a right neighbour, cP ≠ cQ),
    each with n = m b, m b − (b − 1) (a last block row that is all padding but one row) and m b − 1."""
    chains = []
    for m in B.LEVEL_M:
        for n in (32 * m, 32 * m - 31, 32 * m - 1):
            _x, info = _run(nls, monkeypatch, f"levels{m}_{n}", "never")
            assert info["block"] == 32 and info["levels"] == math.ceil(math.log2(m)) + 1
        ch = [m]
        while ch[-1] > 1:
            ch.append((ch[-1] + 1) // 2)
        assert len(ch) == info["levels"]
        chains.append(ch)
    for lvl in range(5):
        assert {ch[lvl] % 2 for ch in chains if len(ch) > lvl and ch[lvl] >= 2} == {0, 1}, lvl


# ---------------------------------------------------------------------------------------------------------------- families
_FAMILY_RUNS = [(n, m) for n, m, r in B.RUNS if r == 0 and B.CASES[n]["family"] in ("spd", "outer", "bratu", "brusselator")]


@pytest.mark.parametrize("name,mode", _FAMILY_RUNS, ids=[f"{n}-{m}" for n, m in _FAMILY_RUNS])
def test_families(nls, monkeypatch, name, mode):
    """spd: B Bᵀ + 1e-3 ‖B Bᵀ‖∞ I (κ∞ ≈ 4e3 … 1e4, multipliers O(1), no dominant diagonal to damp a wrong P C or Q A term), on
    both kernels at b = 32, 128, 160, 256, 288, 512; outer: only the diagonals 0, −kl, +ku, everything between is fill; Bratu
    Jacobians at 32², 50², 100², 130² (both kernels but 50²); Brusselator Jacobians at N = 16, 24, renumbered to half
    bandwidth 4N (bcr_reference.brusselator: in the problem's own numbering they do not reach this engine)."""
    _run(nls, monkeypatch, name, mode)


# --------------------------------------------------------------------------------------------------- pivoting that is needed
@pytest.mark.parametrize("b", [160, 256, 512])
def test_row_pivoting_inside_the_leaves_under_the_schur_recursion(nls, monkeypatch, b):
    """Rows 2i ↔ 2i + 1 of a dominant band exchanged: an exact zero on every other diagonal entry, the dominant entries next
    to it, inside the 128-leaves of the recursion (128 + 32, 128 + 128, 256 + 256). Measured against the long-double solve
    of the matrix with the exchange undone. On the diagonal-pivot kernel the same matrix is refused."""
    name = f"exchanged{b}"
    J = B.problem(name)[0]
    assert np.all(J.diagonal()[0::2] == 0.0)
    _x, info = _run(nls, monkeypatch, name, "always")
    assert info["block"] == b
    with pytest.raises(nls.NKError):
        with _Factored(nls, monkeypatch, J, "never"):
            pass
    # default policy: starts on the diagonal, meets the zero, switches the object to row pivoting
    with _Factored(nls, monkeypatch, J, "auto", b) as S:
        B.check(name, "always", S.F.solve(B.problem(name)[1]), "auto")


# -------------------------------------------------------------------------------------------------------- object semantics
def test_several_right_hand_sides_after_one_factorisation(nls, monkeypatch):
    name = B.MANY_RHS
    J, _b, _x, _k, blk, lev = B.problem(name)
    with _Factored(nls, monkeypatch, J, "never", blk, lev) as S:
        for r in range(4):
            B.check(name, "never", S.F.solve(B.problem(name, r)[1]), f"rhs {r}", rhs=r)


@pytest.mark.parametrize("mode", ["never", "always"])
def test_host_and_device_memspace_agree_bitwise_and_may_alias(nls, dev, monkeypatch, mode):
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    name = "order288"
    J, b, _x, _k, blk, lev = B.problem(name)
    with _Factored(nls, monkeypatch, J, mode, blk, lev) as S:
        xh = S.F.solve(b)
        B.check(name, mode, xh, "host")
        assert np.array_equal(S.F.solve(b), xh)             # the same input twice: the same bits
        bd = torch.tensor(b, device=dev)
        xd = S.F.solve(bd)
        assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
        v = bd.clone()                                      # b and x the same device vector
        L.check(L.lib().nk_lu_solve(S.F._h, C.c_void_p(v.data_ptr()), C.c_void_p(v.data_ptr()), L.DEVICE))
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy(), xh)
        assert np.array_equal(bd.cpu().numpy(), b)          # the non-aliased solve left b alone


@pytest.mark.parametrize("mode", ["never", "always"])
def test_refactor_equals_a_fresh_factorisation_and_recovers_from_a_breakdown(nls, monkeypatch, mode):
    """set_values + factor() against a fresh object (bitwise); then a NaN and a zero-pivot factorisation on the same object
    raise, and the next good factor() gives the bitwise-same solution as before: the failure flag is reset, and nothing of
    the failed attempt survives in the stored blocks."""
    J = BR.dominant_band(5 * 160 - 30, 150, 137, 12)
    J2 = J.copy()
    J2.data = J2.data * (1.0 + 0.05 * np.cos(np.arange(J2.nnz)))
    n = J.shape[0]
    b = BR.manufactured(J2, np.random.default_rng(3).standard_normal(n))
    with _Factored(nls, monkeypatch, J, mode, 160, 4) as S, _Factored(nls, monkeypatch, J2, mode, 160, 4) as S2:
        x1 = S.F.solve(b)
        S.A.set_values(J2.data)
        S.F.factor()
        x_re = S.F.solve(b)
        assert np.array_equal(x_re, S2.F.solve(b)) and not np.array_equal(x_re, x1)
        be, fe = B.errors(J2, x_re, b, BR.reference_solve(J2, b), BR.cond_inf(J2))
        bb, fb = B.BOUNDS[("dominant", mode)]
        assert be <= bb and fe <= fb, (be, fe)
        for row, value in ((170, np.nan), (171, 0.0)):
            bad = J2.copy().tolil()
            if value == 0.0:
                bad[:, row] = 0.0          # an exactly zero column: singular for either kernel
            bad[row, row] = value
            vals = np.asarray(bad.toarray())[J2.nonzero()]
            S.A.set_values(vals)
            with pytest.raises(nls.NKError):
                S.F.factor()
            S.A.set_values(J2.data)
            S.F.factor()
            assert np.array_equal(S.F.solve(b), x_re)


# ------------------------------------------------------------------------------------------------------ breakdown reporting
@pytest.mark.parametrize("mode", ["never", "always", "auto"])
@pytest.mark.parametrize("kind", list(B.BREAKDOWN_LEVEL))
def test_reports_breakdown(nls, monkeypatch, kind, mode):
    """An exactly zero column, inf and nan on the diagonal, an exact 2 × 2 cancellation inside an odd row's diagonal block,
    and one that only appears in a level-1 Schur complement (bcr_reference.breakdown): each is singular for either
    inversion kernel and must raise."""
    Jp, vals, _M = B.breakdown(kind)
    with _Factored(nls, monkeypatch, Jp, mode, 32, 4) as S:
        S.A.set_values(vals.data)
        with pytest.raises(nls.NKError):
            S.F.factor()


# ---------------------------------------------------------------------------------------------------------- exponent range
def _scaled(nls, monkeypatch, name, mode, e):
    J, b, x_ref, kappa, blk, lev = B.problem(name)
    Js = (J * np.ldexp(1.0, e)).tocsr()
    with _Factored(nls, monkeypatch, J, mode, blk, lev) as S, _Factored(nls, monkeypatch, Js, mode, blk, lev) as Ss:
        x, xs = S.F.solve(b), Ss.F.solve(b)
    assert np.all(np.isfinite(xs))
    xr_s = np.asarray(x_ref, dtype=BR.LD) * BR.LD(np.ldexp(1.0, -e))
    be, fe = B.errors(Js, xs, b, xr_s, kappa)
    d = np.max(np.abs(np.ldexp(xs, e) - x)) / np.max(np.abs(x))
    print(f"{name} {mode} 2^{e}: backward {be:.2f} u, forward {fe:.3f} κu, scaled vs unscaled {d / BR.U64:.2f} u")
    bb, fb = B.BOUNDS[(B.CASES[name]["family"], mode)]
    assert be <= bb and fe <= fb, (be, fe)
    assert d <= 8 * BR.U64, d / BR.U64


@pytest.mark.parametrize("e", [-1000, -200, 200, 1000])
def test_exponent_range_on_the_diagonal_pivot_kernel(nls, monkeypatch, e):
    """2^e A x = b gives x scaled by 2^−e, to 8 u: a pivot is refused for being zero or non-finite, not for being small
    (2⁻¹⁰⁰⁰ ≈ 9e-302 is below the 1e-290 the kernel used to compare its pivots with)."""
    _scaled(nls, monkeypatch, "order160", "never", e)


@pytest.mark.parametrize("e", [-200, 200])
def test_exponent_range_on_the_row_pivoting_kernel(nls, monkeypatch, e):
    """The same on the row-exchanged matrix, which needs the pivot search: the candidates are ranked on the high word of the
    double, so the order of their magnitudes is the same at 2^±200 as at 1 (ranked as floats they all became inf or 0, and
    the search fell on the first unused row — here one that holds an exact zero)."""
    _scaled(nls, monkeypatch, "exchanged160", "always", e)
