"""Pins tests/csr_reference.py without a GPU: the sequential sums against the C oracle (bit for bit) and SciPy (within the derived
bound), the Gershgorin restatement against the oracle's, and — for every tile — that the case list really contains every kind
of block it is tagged with, so tests/test_gpu_csr.py cannot quietly stop covering a path."""
import numpy as np
import pytest
import scipy.sparse as sp

import csr_reference as CR
from oracle import c_oracle as CO
from oracle import reference_restatement as R


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


@pytest.mark.parametrize("name", CR.CASES)
def test_sequential_sum_is_the_oracles_and_scipys(name):
    A, x = CR.case(name, 1024), CR.vector(name, 1024)
    y = CR.spmv_sequential(A, x)
    assert np.array_equal(y.view(np.int64), CO.spmv(_i32(A.rowptr), _i32(A.col), A.val, x).view(np.int64))
    bound = CR.gamma(np.maximum(A.rowlen, 1)) * CR.abs_spmv(A, x)           # SciPy sums in some order of its own
    assert np.all(np.abs((A.scipy() @ x).astype(CR.LD) - CR.spmv_longdouble(A, x)) <= bound)
    assert np.all(np.abs(y.astype(CR.LD) - CR.spmv_longdouble(A, x)) <= bound)
    # the transposed sums: ascending row inside a column is what the oracle's scatter loop does as well
    yt = CR.spmv_t_sequential(A, x)
    assert np.array_equal(yt.view(np.int64), CO.spmv_t(_i32(A.rowptr), _i32(A.col), A.val, x, A.n).view(np.int64))
    T, perm = A.transpose()
    assert (T.scipy() != A.scipy().T).nnz == 0 and np.array_equal(T.val, A.val[perm])
    assert np.all(np.abs(CR.colsumsq_sequential(A).astype(CR.LD) - CR.colsumsq_longdouble(A))
                  <= CR.gamma(np.maximum(T.rowlen, 1) + 1) * CR.colsumsq_longdouble(A))


def test_rowblocks_restates_the_host_loop():
    """Against the loop of build_rowblocks written out literally."""
    def literal(rowptr, tile):
        n, rb, r = len(rowptr) - 1, [0], 0
        while r < n:
            e, base = r, rowptr[r]
            while e < n and rowptr[e + 1] - base <= tile and e - r < 1024:
                e += 1
            if e == r:
                e = r + 1
            rb.append(e)
            r = e
        return rb
    for name in ("exact_tile", "long", "empty_run", "n1", "ragged", "small"):
        for tile in CR.TILES:
            A = CR.case(name, tile)
            assert list(CR.rowblocks(A.rowptr, tile)) == literal(A.rowptr.tolist(), tile), (name, tile)


@pytest.mark.parametrize("tile", CR.TILES)
def test_every_tagged_path_is_in_the_case_list(tile):
    seen = set()
    for name in CR.CASES:
        A = CR.case(name, tile)
        kinds = CR.block_kinds(A, tile)
        missing = set(CR.TAGS[name]) - kinds
        assert not missing, f"case {name!r}, tile {tile}: tagged {sorted(missing)} but rowblocks shows no such block"
        assert CR.fits16(A, tile) == CR.FITS16[name], (name, tile, CR.block_offsets(A, tile))
        assert A.n <= 70000 and A.nnz <= 400000
        seen |= kinds
    assert seen >= {"block_exact_tile", "long_row", "row_tile", "row_tile_plus_1", "row_3tile_17", "row_cap", "rows_gt_256",
                    "rows_gt_512", "first_last_empty", "n1", "no_diagonal", "diag_only_row", "explicit_zero", "empty_column",
                    "empty_row", "long_column", "col32", "col16_edge", "col32_edge"}


@pytest.mark.parametrize("tile", CR.TILES)
def test_the_edge_cases_sit_on_the_edge(tile):
    assert CR.block_offsets(CR.case("edge16", tile), tile) == (-32768, 32767)
    assert CR.block_offsets(CR.case("edge32", tile), tile) == (-32769, 32768)
    lo, hi = CR.block_offsets(CR.case("wide", tile), tile)
    assert lo < -60000 and hi > 60000


def _mat(J):
    J = sp.csr_matrix(J)
    J.sort_indices()
    return CR.Mat(J.shape[0], J.indptr, J.indices, J.data)


@pytest.mark.parametrize("which", ["bratu", "brusselator"])
def test_gershgorin_restatement_is_the_oracles(which):
    if which == "bratu":
        P = R.Bratu2D(64, 6.0)
        u = 0.3 * np.random.default_rng(1).standard_normal(P.n)
    else:
        P = R.Brusselator2D(32)
        u = 1.0 + 0.1 * np.random.default_rng(2).standard_normal(P.n)
    J = P.jac(u)
    A = _mat(J)
    mlo, hi = CR.gershgorin_pair(A)
    lo_o, hi_o = R.gershgorin_interval(J)
    # the oracle forms Σ|a_ij| − |a_ii| (another order of the same ≤ k + 1 additions): equal within γ_{k+1} Σ|a_ij|
    bound = float(np.max(CR.gamma(A.rowlen + 1) * CR.segsum(A.rowptr, np.abs(A.val))))
    assert abs(-mlo - lo_o) <= bound and abs(hi - hi_o) <= bound
    CR.gershgorin_check((mlo, hi), A, 1024)


def test_normal_matrix_is_jtj():
    for name, lam, d in (("small", 0.0, None), ("small", 0.75, "d"), ("n1", 2.0, "d")):
        J = CR.case(name, 512)
        dd = None if d is None else np.random.default_rng(3).uniform(0.5, 2.0, J.n)
        rp, col, val = CR.normal_matrix(J, lam, dd)
        S = J.scipy()
        N = (S.T @ S + (sp.diags(lam * dd) if dd is not None else sp.csr_matrix((J.n, J.n)))).toarray()
        got = sp.csr_matrix((val, col, rp), shape=(J.n, J.n))
        assert np.all(np.diff(rp) >= 1) and np.all(got.diagonal() == val[col == np.repeat(np.arange(J.n), np.diff(rp))])
        mag = (abs(S).T @ abs(S)).toarray() + (np.diag(lam * dd) if dd is not None else 0.0)
        k = int(np.max(np.bincount(J.col, minlength=J.n))) + 2
        assert np.all(np.abs(got.toarray() - N) <= 2 * CR.gamma(k) * mag)
        # pattern: exactly the structural non-zeros of JᵀJ and the diagonal
        O = J.with_values(np.ones(J.nnz)).scipy()          # (stored zeros belong to the pattern)
        P = (O.T @ O + sp.identity(J.n)).tocsr()
        P.sort_indices()
        assert np.array_equal(P.indptr, rp) and np.array_equal(P.indices, col)


def test_epilogue_bound_covers_a_perturbed_sum():
    """The propagation in epilogue_bound: perturb s by ±δ in float64, run the epilogue in float64, compare with the long-double
    epilogue of the unperturbed sum."""
    rng = np.random.default_rng(5)
    n = 4000
    S = rng.standard_normal(n).astype(CR.LD) * 50
    delta = np.abs(S) * CR.LD(2.0 ** -45)
    s = (S + rng.choice([-1.0, 1.0], n) * delta).astype(np.float64)
    x, r, yacc, dinv = (rng.standard_normal(n) for _ in range(4))
    kw = dict(c1=0.37, c2=-1.9, theta=2.5)
    for mode, extra in ((0, {}), (0, dict(out_scale=0.3)), (1, dict(yacc=yacc)), (1, dict(yacc=yacc, dinv=dinv)), (2, {}),
                        (3, {}), (3, dict(out_scale=-7.0)), (4, {})):
        got = CR.epilogue(mode, s, x, r=r, **kw, **extra)
        ref = CR.epilogue(mode, S, x, r=r, **kw, **extra)
        bnd = CR.epilogue_bound(mode, delta + np.abs(S) * CR.LD(CR.U), S, x, r=r, **kw, **extra)
        assert set(got) == set(ref) == set(bnd)
        for key in got:
            assert np.all(np.abs(got[key].astype(CR.LD) - ref[key]) <= bnd[key]), (mode, extra, key)
