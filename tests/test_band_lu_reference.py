"""The long-double unpivoted LU that tests/test_gpu_band_lu.py measures the device band LU against: pinned here against SciPy
(CPU only)."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import band_lu_reference as BR


def _dominant(n, kl, ku, seed):
    rng = np.random.default_rng(seed)
    M = sp.diags([rng.standard_normal(n - abs(k)) for k in range(-kl, ku + 1)], range(-kl, ku + 1)).tocsr()
    return (M + sp.identity(n) * (1.5 * (kl + ku + 1))).tocsr()


@pytest.mark.parametrize("n,kl,ku", [(1, 0, 0), (7, 0, 3), (7, 3, 0), (50, 1, 1), (97, 33, 5), (130, 40, 64)])
def test_reference_agrees_with_scipy_dense_and_band(n, kl, ku):
    A = _dominant(n, kl, ku, n + kl + ku)
    assert BR.bandwidths(A) == (kl, ku)
    rng = np.random.default_rng(1)
    x_true = rng.standard_normal(n)
    b = BR.manufactured(A, x_true)
    xd = BR.reference_solve(A, b, dense=True)
    xb = BR.reference_solve(A, b, dense=False)
    xs = sla.solve(A.toarray(), b)
    kappa = BR.cond_inf(A)
    assert BR.forward_error(xs, xd) <= 8 * kappa * BR.U64
    # both forms run the same operations in the same order
    assert np.array_equal(xd, xb)
    # extended precision: far below what a float64 solve can reach
    assert BR.backward_error(A, xd.astype(np.float64), b) <= 2 * BR.U64
    assert BR.forward_error(xd, x_true) <= 4 * kappa * BR.U64
    assert kappa <= BR.cond_inf_dominant(A) * (1 + 1e-12)
    BR.check_solution(A, xs, b, xd, kappa, "scipy")


def test_reference_keeps_extended_precision_on_an_ill_conditioned_spd_matrix():
    """B Bᵀ + δI (κ ≈ 1e7): the long-double factors leave a forward error orders of magnitude below a float64 solve's."""
    n, w = 120, 6
    rng = np.random.default_rng(5)
    B = sp.diags([rng.standard_normal(n - k) for k in range(w + 1)], [-k for k in range(w + 1)]).toarray()
    B[:, 17] = 0.0
    G = B @ B.T
    A = G + np.eye(n) * 1e-7 * np.linalg.norm(G, 2)
    kappa = BR.cond_inf(A)
    assert 1e6 <= kappa <= 1e9
    x_true = rng.standard_normal(n)
    b = BR.manufactured(A, x_true)
    xd = BR.reference_solve(A, b)
    x64 = sla.solve(A, b)
    assert BR.forward_error(x64, xd) <= BR.FORWARD_FACTOR * kappa * BR.U64
    # the reference solves the rounded b: its distance to x_true is the conditioning of that rounding, not its own error
    r = np.asarray(b, dtype=BR.LD) - BR.matvec_ld(A, xd)
    assert float(np.max(np.abs(r))) <= 1e-16 * float(np.max(np.abs(b)))


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("k", [0, 5, 32, 49])
def test_reference_reports_an_exact_zero_pivot(dense, k):
    """A zero on the diagonal at row k, or one that appears there through the elimination (k = 32: row 31's update cancels
    it exactly), raises ZeroPivot(k)."""
    n = 50
    A = _dominant(n, 2, 2, 3).toarray()
    if k == 32:
        # 2×2 block [[a, c], [d, c·d/a]] at rows 31, 32 whose Schur complement vanishes; the rows above do not reach row 32
        A[31, :] = 0.0
        A[32, :] = 0.0
        A[:, 31] = 0.0
        A[:, 32] = 0.0
        A[31, 31], A[31, 32], A[32, 31], A[32, 32] = 2.0, 3.0, 4.0, 6.0
    else:
        A[k, :k + 1] = 0.0   # no multiplier reaches row k either: its pivot is the stored zero
    with pytest.raises(BR.ZeroPivot) as e:
        BR.reference_solve(sp.csr_matrix(A), np.ones(n), dense=dense)
    assert e.value.k == k


def test_reference_reports_a_non_finite_pivot():
    A = _dominant(10, 1, 1, 0).toarray()
    A[4, 4] = np.nan
    with pytest.raises(BR.ZeroPivot):
        BR.reference_solve(A, np.ones(10))
