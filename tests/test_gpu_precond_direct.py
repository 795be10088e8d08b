"""The preconditioner objects (csrc/nk_precond.hip) on their own, through the C ABI / the Preconditioner classes, against
tests/precond_reference.py: the ILU(0) factorisation and both triangular solves on every schedule shape — per-level launches,
the persistent-workgroup chain kernels (with levels wider than their 1024 threads: tridiag17x4096, mixed_schedule), one of each
inside the same apply — Jacobi, ILU(τ) with its host factorisation, in-place application, and failure and recovery.

Every numerical assertion is equality of bits with the sequential float64 sweep of the same operations (the library is built with
-ffp-contract=off; one rounding per operation, a row's entries in CSR order). Which kernel a case runs is not observable through
the ABI: every case first asserts that the restated rule (precond_reference.chain_pays) sends its matrix where the case list says,
and that the object reports the reference's level counts — a change of the rule fails the cases instead of moving them."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import precond_reference as PR
from oracle import reference_restatement as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b, what="", rowof=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: {a.shape} != {b.shape}"
    bad = np.flatnonzero(_bits(a) != _bits(b))
    where = "" if rowof is None or bad.size == 0 else f" (row {rowof[bad[0]]})"
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} entries differ, first at {bad[0]}{where}: {a[bad[0]]!r} != {b[bad[0]]!r}"


def _csr(nls, A):
    return nls.CSRMatrix.from_arrays(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)


def _raw(M):
    """(rowptr, col, values, perm) of an incomplete-LU object as the device holds them: one row-major array, L below the
    diagonal, U on and above"""
    from nonlinearsolve_jl_amd import _lib as L
    nnz = C.c_int64(0)
    L.check(L.lib().nk_precond_ilu0_factors(M._h, C.byref(nnz), None, None, None, None))
    n = M.A.shape[0]
    rp, ci = np.zeros(n + 1, dtype=np.int32), np.zeros(nnz.value, dtype=np.int32)
    v, perm = np.zeros(nnz.value), np.zeros(n, dtype=np.int32)
    L.check(L.lib().nk_precond_ilu0_factors(M._h, None, C.c_void_p(rp.ctypes.data), C.c_void_p(ci.ctypes.data),
                                            C.c_void_p(v.ctypes.data), C.c_void_p(perm.ctypes.data)))
    return rp, ci, v, perm


def _check_factors(M, ref, perm, what):
    rp, ci, dg, lu = ref
    rpd, cid, lud, permd = _raw(M)
    assert np.array_equal(permd, np.arange(rp.size - 1) if perm is None else perm), f"{what}: permutation"
    assert np.array_equal(rpd, rp) and np.array_equal(cid, ci), f"{what}: pattern"
    _same(lud, lu, f"{what}: factors", rowof=np.repeat(np.arange(rp.size - 1), np.diff(rp)))
    return lud


def _check_apply(M, ref, perm, x, what, dev):
    """host vector in, device tensor in, a second time: the reference's bits each time"""
    import torch
    rp, ci, dg, lu = ref
    want = PR.tri_apply(rp, ci, dg, lu, perm, x)
    got = M.apply(x)
    _same(got, want, f"{what}: apply (host vector)", rowof=np.arange(x.size))
    xd = torch.tensor(x, device=dev)
    _same(M.apply(xd).cpu().numpy(), got, f"{what}: apply (device tensor)")
    _same(M.apply(xd).cpu().numpy(), got, f"{what}: second apply")
    _same(xd.cpu().numpy(), x, f"{what}: apply wrote into its input")


# ------------------------------------------------------------------------------------------------------- ILU(0) and Jacobi
@pytest.mark.parametrize("name,ordering", PR.CASE_IDS)
def test_ilu0_bit_for_bit(nls, dev, name, ordering):
    """Permutation, pattern, factors and M⁻¹x equal to the sequential sweep, for the values the object was created with, after a
    second update(), after new values on the same pattern, and for the same matrix handed over with every row's columns
    shuffled (the per-row sort and the value gather of the symbolic phase)."""
    nl, nu, wl, wu, chain_l, chain_u = expected = PR.EXPECTED[(name, ordering)]
    assert PR.schedule(name, ordering) == expected                     # the path this case is for, by the restated rule
    A, perm = PR.matrix(name), PR.permutation(name, ordering)
    ref = PR.factors(name, ordering)
    x, b = PR.vectors(name)
    what = f"{name} {ordering}"
    J = _csr(nls, A)
    M = nls.ILU0Preconditioner(J, ordering=ordering)
    info = M.info()
    assert (info["levels_lower"], info["levels_upper"]) == (nl, nu)
    if ordering == "multicolor":
        assert info["ncolors"] == R.multicolor_permutation(A)[1]
    first = _check_factors(M, ref, perm, what)
    Ld, Ud, permd = M.factors()
    Lr, Ur = PR.split_lu(ref[0], ref[1], ref[3])
    for Fd, Fr in ((Ld, Lr), (Ud, Ur)):
        Fd.sort_indices(); Fr.sort_indices()
        assert np.array_equal(Fd.indptr, Fr.indptr) and np.array_equal(Fd.indices, Fr.indices)
        _same(Fd.data, Fr.data, f"{what}: factors()")
    _check_apply(M, ref, perm, x, what, dev)
    _check_apply(M, ref, perm, b, what + " (A @ ones)", dev)
    M.update()
    _same(_raw(M)[2], first, f"{what}: second update()")
    # new values on the same pattern
    B = PR.new_values(A)
    ref2 = PR.ilu0_sweep(B, perm)
    J.set_values(B.data)
    M.update()
    _check_factors(M, ref2, perm, what + " new values")
    _check_apply(M, ref2, perm, x, what + " new values", dev)
    # the same matrix with every row's columns in a random order
    rps, cis, order = PR.shuffled(A)
    Js = nls.CSRMatrix.from_arrays(rps, cis, A.data[order])
    Ms = nls.ILU0Preconditioner(Js, ordering=ordering)
    _check_factors(Ms, ref, perm, what + " shuffled")
    _same(Ms.apply(x), PR.tri_apply(*ref, perm, x), what + " shuffled: apply")
    Js.set_values(B.data[order])
    Ms.update()
    _check_factors(Ms, ref2, perm, what + " shuffled, new values")
    # Jacobi: k_jacobi_setup stores 1/d, k_jacobi_apply multiplies by it — (1.0 / d) * x, not x / d
    import torch
    for Jm, values in ((J, A.data), (Js, A.data[order])):               # (both hold B's values now)
        Mj = nls.JacobiPreconditioner(Jm)
        _same(Mj.apply(x), (1.0 / B.diagonal()) * x, what + ": Jacobi")
        _same(Mj.apply(torch.tensor(x, device=dev)).cpu().numpy(), (1.0 / B.diagonal()) * x, what + ": Jacobi (device tensor)")
        Jm.set_values(values)
        Mj.update()
        _same(Mj.apply(x), (1.0 / A.diagonal()) * x, what + ": Jacobi after update()")


# ------------------------------------------------------------------------------------------------------------------ in place
@pytest.mark.parametrize("kind", ["jacobi", "ilu0_natural", "ilu0_multicolor", "ilut", "amg"])
def test_apply_in_place_equals_apply_out_of_place(nls, dev, kind):
    """nk_precond_apply with the same device pointer for x and y (the header allows it; Preconditioner.apply never does it)"""
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    if kind == "amg":
        pb = R.Bratu2D(32)
        A = sp.csr_matrix(pb.jac(np.full(pb.n, 0.3)))
        A.sort_indices()
    elif kind == "ilut":
        A = PR.ilut_case("random400")[0]
    else:
        A = PR.matrix("random_banded")
    J = _csr(nls, A)
    M = {"jacobi": lambda: nls.JacobiPreconditioner(J), "ilu0_natural": lambda: nls.ILU0Preconditioner(J, ordering="natural"),
         "ilu0_multicolor": lambda: nls.ILU0Preconditioner(J, ordering="multicolor"),
         "ilut": lambda: nls.ILUTPreconditioner(J, 0.05), "amg": lambda: nls.AMGPreconditioner(J)}[kind]()
    x = np.random.default_rng(7).standard_normal(A.shape[0])
    xd = torch.tensor(x, device=dev)
    want = M.apply(xd.clone()).cpu().numpy()
    assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0.0
    L.check(L.lib().nk_precond_apply(M._h, C.c_void_p(xd.data_ptr()), C.c_void_p(xd.data_ptr()), L.DEVICE))
    _same(xd.cpu().numpy(), want, f"{kind}: in place")
    if kind != "amg":
        hx = x.copy()                                                  # host vectors are staged on the device: aliasing is free
        L.check(L.lib().nk_precond_apply(M._h, C.c_void_p(hx.ctypes.data), C.c_void_p(hx.ctypes.data), L.HOST))
        _same(hx, want, f"{kind}: in place (host vector)")


# ------------------------------------------------------------------------------------------------------ failure and recovery
def _two_by_two():
    good = sp.csr_matrix(np.array([[2.0, 1.0], [1.0, 2.0]]))
    return good, np.ones(4), "row 1"


def _chain40():
    """interleaved_tridiag(20, 2): 20 levels of 2 rows, the chain kernels. Rows 1 and 3 are the first two of chain b = 1; with
    (1,1) = 2, (1,3) = 1, (3,1) = 2, (3,3) = 1 the multiplier is 2 / 2 = 1 and the pivot of row 3 is 1 − 1 · 1 = 0 exactly."""
    good = PR.interleaved_tridiag(20, 2)
    wl, wu = PR.level_widths(good)
    assert len(wl) == len(wu) == 20 and PR.chain_pays(wl) and PR.chain_pays(wu)
    bad = good.copy()
    for (i, j, v) in ((1, 1, 2.0), (1, 3, 1.0), (3, 1, 2.0), (3, 3, 1.0)):
        bad[i, j] = v
    assert bad.nnz == good.nnz and np.array_equal(bad.indices, good.indices)
    return good, bad.data.copy(), "row 3"


def _with_nan(good):
    bad = good.data.copy()
    # the first entry of a middle row, below the diagonal: ILU(0) meets it as a multiplier, so in the row's pivot; in ILU(τ)
    # `|w| ≥ τ` is false for a NaN, which would drop it as if it were small — ilut_update tests the candidates explicitly
    bad[good.indptr[good.shape[0] // 2]] = np.nan
    return bad


@pytest.mark.parametrize("kind", ["ilu0", "ilut"])
@pytest.mark.parametrize("case", ["two_by_two", "chain40"])
def test_a_zero_pivot_met_during_elimination_and_a_nan_refuse_and_recover(nls, dev, case, kind):
    """The input has no zero on its diagonal: the pivot cancels during elimination. Creation with such values raises; an
    existing object raises at update(), refuses to apply until an update() with good values, and then gives the reference's bits
    again. The same with one value NaN."""
    good, bad, row = _two_by_two() if case == "two_by_two" else _chain40()
    with pytest.raises(ArithmeticError, match=row):
        PR.ilu0_sweep(sp.csr_matrix((bad, good.indices, good.indptr), shape=good.shape))
    make = (lambda J: nls.ILU0Preconditioner(J, ordering="natural")) if kind == "ilu0" else (lambda J: nls.ILUTPreconditioner(J, 0.0))
    if kind == "ilu0":
        ref = PR.ilu0_sweep(good)
    else:
        ref = PR.pack_lu(*R.ilut(good, 0.0))
    x = np.random.default_rng(8).standard_normal(good.shape[0])
    want = PR.tri_apply(*ref, None, x)
    for values, msg in ((bad, "pivot"), (_with_nan(good), "non-finite")):
        with pytest.raises(nls.NKError, match=msg):
            make(nls.CSRMatrix.from_arrays(good.indptr.astype(np.int32), good.indices.astype(np.int32), values))
    J = _csr(nls, good)
    M = make(J)
    _same(M.apply(x), want, f"{case} {kind}: before")
    for values, msg in ((bad, "pivot"), (_with_nan(good), "non-finite")):
        J.set_values(values)
        with pytest.raises(nls.NKError, match=msg):
            M.update()
        with pytest.raises(nls.NKError, match="no valid factors"):
            M.apply(x)
        with pytest.raises(nls.NKError, match="no valid factors"):
            M.apply(x)                                                 # it keeps refusing
        J.set_values(good.data)
        M.update()
        _same(_raw(M)[2], ref[3], f"{case} {kind}: factors after recovery")
        _same(M.apply(x), want, f"{case} {kind}: apply after recovery")


def test_jacobi_zero_or_missing_diagonal(nls, dev):
    good = PR.interleaved_tridiag(20, 2)
    n = good.shape[0]
    x = np.random.default_rng(8).standard_normal(n)
    zero = good.copy()
    zero[7, 7] = 0.0                                                   # stored, and zero
    assert zero.nnz == good.nnz
    with pytest.raises(nls.NKError, match="diagonal"):
        nls.JacobiPreconditioner(_csr(nls, zero))
    keep = ~((np.repeat(np.arange(n), np.diff(good.indptr)) == 7) & (good.indices == 7))
    rp = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(good.indptr))[keep], minlength=n))])
    with pytest.raises(nls.NKError, match="diagonal"):                 # row 7 stores no diagonal entry
        nls.JacobiPreconditioner(nls.CSRMatrix.from_arrays(rp.astype(np.int32), good.indices[keep].astype(np.int32), good.data[keep]))
    J = _csr(nls, good)
    M = nls.JacobiPreconditioner(J)
    _same(M.apply(x), (1.0 / good.diagonal()) * x, "Jacobi: before")
    nan = good.copy()
    nan[7, 7] = np.nan
    for values in (zero.data, nan.data):
        J.set_values(values)
        with pytest.raises(nls.NKError, match="diagonal"):
            M.update()
        with pytest.raises(nls.NKError, match="no valid factors"):
            M.apply(x)
        J.set_values(good.data)
        M.update()
        _same(M.apply(x), (1.0 / good.diagonal()) * x, "Jacobi: after recovery")


# --------------------------------------------------------------------------------------------------------------------- ILU(τ)
def _check_ilut(nls, dev, P, A, tau, packed, what):
    """the host factorisation against the oracle's Crout restatement (both sum in ascending i, neither contracts), the device's
    substitutions on those factors against the sequential ones"""
    rp, ci, dg, lu = packed
    Lo, Uo = R.ilut(A, tau)
    Ld, Ud, perm = P.factors()
    for Fd, Fo in ((Ld, Lo), (Ud, Uo)):
        Fd.sort_indices(); Fo.sort_indices()
        assert np.array_equal(Fd.indptr, Fo.indptr) and np.array_equal(Fd.indices, Fo.indices), f"{what}: pattern of factors()"
        _same(Fd.data, Fo.data, f"{what}: factors()")
    _check_factors(P, packed, None, what)
    wl, wu = PR.level_widths(sp.csr_matrix((np.ones(ci.size), ci, rp), shape=A.shape))
    info = P.info()
    assert info["kind"] == "ilut" and (info["levels_lower"], info["levels_upper"]) == (len(wl), len(wu))
    x = np.random.default_rng(6).standard_normal(A.shape[0])
    _check_apply(P, packed, None, x, what, dev)
    _check_apply(P, packed, None, A @ np.ones(A.shape[0]), what + " (A @ ones)", dev)
    return wl, wu


@pytest.mark.parametrize("name", list(PR.ILUT_CASES))
def test_ilut_bit_for_bit(nls, dev, name):
    A, tau, packed = PR.ilut_case(name)
    P = nls.ILUTPreconditioner(_csr(nls, A), tau)
    wl, wu = _check_ilut(nls, dev, P, A, tau, packed, name)
    if name == "tridiagonal3000_tau0":                                 # the chain kernels on ILU(τ)'s replaced device arrays
        assert len(wl) == len(wu) == 3000 and PR.chain_pays(wl) and PR.chain_pays(wu)
    rps, cis, order = PR.shuffled(A)
    Ps = nls.ILUTPreconditioner(nls.CSRMatrix.from_arrays(rps, cis, A.data[order]), tau)
    _check_factors(Ps, packed, None, name + " shuffled")


@pytest.mark.parametrize("name", list(PR.ILUT_HAND))
def test_ilut_hand_cases(nls, dev, name):
    """|z| == τ is kept and one ulp above it is dropped; a row without a stored diagonal entry whose pivot fill creates (the host
    factorisation goes on by design; ILU(0) needs the stored entry)"""
    A, tau, Lh, Uh = PR.ILUT_HAND[name]
    n = A.shape[0]
    J = _csr(nls, A)
    assert J.info()["nnz"] == A.nnz
    P = nls.ILUTPreconditioner(J, tau)
    Ld, Ud, _ = P.factors()
    assert np.array_equal(Ld.toarray(), np.array(Lh, dtype=np.float64) + np.eye(n))
    assert np.array_equal(Ud.toarray(), np.array(Uh, dtype=np.float64))
    assert Ld.nnz == np.count_nonzero(Lh) + n and Ud.nnz == np.count_nonzero(Uh)
    packed = PR.pack_lu(*R.ilut(A, tau))
    _check_ilut(nls, dev, P, A, tau, packed, name)
    if name == "missing_diagonal":
        with pytest.raises(nls.NKError, match="diagonal"):
            nls.ILU0Preconditioner(J, ordering="natural")


def test_ilut_update_replans_for_factors_of_another_size(nls, dev):
    """update() after values that change the kept pattern: fewer entries, then more again — factors and apply follow"""
    A, tau, packed = PR.ilut_case("unsymmetric400_tau0.05")
    B = A.copy()
    B.data = A.data * 0.3                                              # more entries fall under τ
    B.setdiag(A.diagonal())
    assert np.array_equal(B.indices, A.indices) and B.nnz == A.nnz
    packed_b = PR.pack_lu(*R.ilut(B, tau))
    J = _csr(nls, A)
    P = nls.ILUTPreconditioner(J, tau)
    nnz_a = _raw(P)[2].size
    _check_ilut(nls, dev, P, A, tau, packed, "before")
    J.set_values(B.data)
    P.update()
    nnz_b = _raw(P)[2].size
    assert nnz_b < nnz_a and nnz_b == packed_b[3].size
    _check_ilut(nls, dev, P, B, tau, packed_b, "smaller factors")
    J.set_values(A.data)
    P.update()
    assert _raw(P)[2].size == nnz_a
    _check_ilut(nls, dev, P, A, tau, packed, "larger factors again")
