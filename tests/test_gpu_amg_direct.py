"""The aggregation AMG (csrc/nk_amg.hip) against tests/amg_reference.py: the hierarchy's structure — sizes, the aggregates of every
level, every level matrix (nk_precond_amg_level_matrix) and λmax — bit for bit against the sequential float64 reference, and the
V-cycle against the long-double V-cycle on the same structure within the case's row of AR.TABLE × 100; at non-default parameters,
one-level and tiny hierarchies, the scan's tile edges and its third level, the Gershgorin reduction's block edges, a stall below
level 0, after update(), under both set-ups, on a rank's local block, and through every documented error."""
import ctypes as C
import os
import socket
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_reference as AR  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not AR.LONGDOUBLE_OK, reason="np.longdouble has fewer than 64 significand bits")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 64, -7.25
INVALID, SINGULAR = "status -1:", "status -7:"


def _matrix(nls, A, v=None):
    A = sp.csr_matrix(A)
    return nls.CSRMatrix.from_arrays(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data if v is None else v)


def _device_got(P):
    """the device's hierarchy in the form AR.check_structure takes"""
    h = P.hierarchy()
    levels = []
    for l, (n, nnz, _lm) in enumerate(h):
        Ml = P.level_matrix(l)
        info = Ml.info()
        assert (info["nrows_local"], info["nnz"], info["n_halo"]) == (n, nnz, 0)
        levels.append(dict(nnz=nnz, vals=Ml.values(), y=Ml.matvec(AR.probe(n, l)) if n else np.zeros(0)))
    return dict(sizes=[x[0] for x in h], aggs=[P.aggregates(l) for l in range(len(h) - 1)], lmax=[x[2] for x in h], levels=levels)


def _apply_guarded(nls, P, b, device):
    """y = P b through the C entry point on vectors that sit between guard values, which must come back untouched"""
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    n = len(b)
    if device:
        xb = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda:0")
        yb = xb.clone()
        xb[GUARD:GUARD + n] = torch.as_tensor(b, dtype=torch.float64)
        px, py = xb.data_ptr() + 8 * GUARD, yb.data_ptr() + 8 * GUARD
    else:
        xb, yb = np.full(n + 2 * GUARD, SENTINEL), np.full(n + 2 * GUARD, SENTINEL)
        xb[GUARD:GUARD + n] = b
        px, py = xb.ctypes.data + 8 * GUARD, yb.ctypes.data + 8 * GUARD
    L.check(L.lib().nk_precond_apply(P._h, C.c_void_p(px), C.c_void_p(py), L.DEVICE if device else L.HOST))
    xh, yh = (xb.cpu().numpy(), yb.cpu().numpy()) if device else (xb, yb)
    assert np.array_equal(xh[GUARD:GUARD + n], b), "the right-hand side was written"
    for buf in (xh, yh):
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + n:] == SENTINEL), "a guard value was overwritten"
    return yh[GUARD:GUARD + n].copy()


def _check_applies(nls, P, name, refs, rhs, what):
    """device and host vectors within the bound, two applies the same bits; returns (the device results, the largest deviation)"""
    out, worst = [], 0.0
    for b, ref in zip(rhs, refs):
        yd = _apply_guarded(nls, P, b, True)
        yh = _apply_guarded(nls, P, b, False)
        worst = max(worst, AR.relmax(yd, ref), AR.relmax(yh, ref))
        AR.check_apply(name, yd, ref, what + "device vectors: ")
        AR.check_apply(name, yh, ref, what + "host vectors: ")
        assert np.array_equal(yd, yh) and np.array_equal(yd, _apply_guarded(nls, P, b, True)), what + "two applies differ"
        out.append(yd)
    return out, worst


_RUNS = {}


def _run(nls, name, matching):
    """create → structure → apply → update(new values) → structure → apply → update(first values) → the first bits"""
    if (name, matching) in _RUNS:
        return _RUNS[(name, matching)]
    case, A = AR.CASES[name], AR.matrix(name)
    n = A.shape[0]
    v0, v1, rhs = AR.values(name, 0), AR.values(name, 1), AR.rhs_set(n, name)
    M = _matrix(nls, A, v0)
    P = nls.AMGPreconditioner(M, matching=matching, **case.params)
    assert P.matching == AR.oracle_matching(matching)
    S = AR.structure(name, matching)
    got0 = _device_got(P)
    AR.check_structure(S, AR.numbers(S, v0), got0, "created: ")
    y0, w0 = _check_applies(nls, P, name, AR.reference_applies(name, matching, 0), rhs, "created: ")
    M.set_values(v1)
    P.update()
    AR.check_structure(S, AR.numbers(S, v1), _device_got(P), "updated: ")
    _y1, w1 = _check_applies(nls, P, name, AR.reference_applies(name, matching, 1), rhs, "updated: ")
    M.set_values(v0)
    P.update()
    for a, b in zip(y0, rhs):
        assert np.array_equal(a, _apply_guarded(nls, P, b, True)), "an update back to the first values does not give the first bits"
    print(f"DEVIATION family={case.family} case={name} matching={matching} dev={max(w0, w1):.3e} bound={AR.bound(name):.3e}")
    _RUNS[(name, matching)] = (got0, y0)
    P.close()
    M.close()
    return _RUNS[(name, matching)]


@pytest.mark.parametrize("matching", AR.MATCHINGS)
@pytest.mark.parametrize("name", list(AR.CASES))
def test_structure_apply_and_update_against_the_reference(nls, dev, name, matching):
    _run(nls, name, matching)


@pytest.mark.parametrize("name", AR.SAME_AGGREGATES)
def test_host_and_device_setups_agree_bit_for_bit(nls, dev, name):
    """the same aggregates under both matchings: the host's emap → gptr plan and the device's key sort give the same sums"""
    (ga, ya), (gg, yg) = _run(nls, name, "auto"), _run(nls, name, "greedy")
    assert ga["sizes"] == gg["sizes"] and ga["lmax"] == gg["lmax"]
    for a, g in zip(ga["levels"], gg["levels"]):
        assert np.array_equal(a["vals"].view(np.int64), g["vals"].view(np.int64)) and np.array_equal(a["y"], g["y"])
    for a, g in zip(ya, yg):
        assert np.array_equal(a, g)


# ------------------------------------------------------------------------------------------------------------- the third scan level
@pytest.mark.parametrize("matching", AR.MATCHINGS)
def test_chain_4_to_the_11_the_scans_third_level(nls, dev, matching):
    """chain(4**11, 0.5): n + 1 > 2048² entries in the scans of the device set-up. Structure: the closed form of
    AR.closed_chain4 (proved against the restatement at 4**6 and 4**7 without a GPU), every level matrix bit for bit; apply:
    against the module's float64 V-cycle (the long-double one takes seconds per right-hand side at this size). Creating the
    matrix and its hierarchy takes 0.15 s (device set-up) / 0.45 s (host set-up) on an MI355X, the whole case 1.5 s."""
    k = AR.CHAIN4.k
    n = 4 ** k
    S = AR.closed_chain4(k)
    t0 = time.time()
    rp, ci = S.pats[0][0], S.pats[0][1]
    M = nls.CSRMatrix.from_arrays(rp.astype(np.int32), ci.astype(np.int32), S.fixed_values[0])
    P = nls.AMGPreconditioner(M, matching=matching)
    t1 = time.time()
    assert P.matching == AR.oracle_matching(matching)
    lv = AR.numbers(S, None)
    AR.check_structure(S, lv, _device_got(P))
    V = AR.VCycle(S, None, np.float64)
    worst = 0.0
    for b in AR.rhs_set(n, AR.CHAIN4.name):
        ref = V(b)
        y = P.apply(b)
        worst = max(worst, AR.relmax(y, ref))
        AR.check_apply(AR.CHAIN4.name, y, ref)
    print(f"DEVIATION family=chain4 case={AR.CHAIN4.name} matching={matching} dev={worst:.3e} bound={AR.bound(AR.CHAIN4.name):.3e} "
          f"create={t1 - t0:.2f}s")


# ------------------------------------------------------------------------------------------------------------- errors
def _usable(nls):
    """the context after an error: a create and an apply succeed and are right"""
    name = "chain9"
    P = nls.AMGPreconditioner(_matrix(nls, AR.matrix(name), AR.values(name)))
    for b, ref in zip(AR.rhs_set(9, name), AR.reference_applies(name, "auto", 0)):
        AR.check_apply(name, P.apply(b), ref, "after an error: ")


def _with_value(A, i, j, val):
    A = sp.csr_matrix(A).copy()
    k = A.indptr[i] + int(np.nonzero(A.indices[A.indptr[i]:A.indptr[i + 1]] == j)[0][0])
    A.data[k] = val
    return A


def _without_entry(A, i, j):
    A = sp.csr_matrix(A).tolil()
    A[i, j] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    return A


@pytest.mark.parametrize("matching", AR.MATCHINGS)
@pytest.mark.parametrize("n", [100, 300])
def test_zero_and_missing_diagonal_entries_are_singular(nls, dev, n, matching):
    for A in (_with_value(AR.chain(n), 7, 7, 0.0), _without_entry(AR.chain(n), n - 1, n - 1), _without_entry(AR.chain(n), 0, 0)):
        with pytest.raises(nls.NKError, match=SINGULAR):
            nls.AMGPreconditioner(_matrix(nls, A), matching=matching)
    _usable(nls)


@pytest.mark.parametrize("matching", AR.MATCHINGS)
def test_a_singular_coarsest_matrix_is_singular(nls, dev, matching):
    """small integers, two equal rows, one dense level: the elimination meets an exact zero pivot (in the first group of eight
    pivots; n = 9 and 120: with the identity border / further groups behind it)"""
    for n in (4, 9, 120):
        D = np.eye(n) * 3.0
        D[0, :2] = D[1, :2] = (2.0, 1.0)
        with pytest.raises(nls.NKError, match=SINGULAR):
            nls.AMGPreconditioner(_matrix(nls, sp.csr_matrix(D)), matching=matching)
        with pytest.raises(ArithmeticError):
            AR.ge_solve(D, np.ones(n), AR.LD)
    _usable(nls)


@pytest.mark.parametrize("matching", AR.MATCHINGS)
@pytest.mark.parametrize("n", [100, 128, 129, 300])
def test_unsorted_and_duplicate_columns_are_refused_by_both_setups(nls, dev, n, matching):
    A = AR.chain(n)
    rp, ci, v = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()
    r = n // 2
    swapped = ci.copy()
    swapped[rp[r]], swapped[rp[r] + 1] = ci[rp[r] + 1], ci[rp[r]]
    dup = ci.copy()
    dup[rp[n - 1]] = dup[rp[n - 1] + 1]                   # the last row holds its diagonal twice
    for cols in (swapped, dup):
        M = nls.CSRMatrix.from_arrays(rp, cols, v)
        with pytest.raises(nls.NKError, match=INVALID + ".*not sorted"):
            nls.AMGPreconditioner(M, matching=matching)
    _usable(nls)


def test_parameter_fields(nls, dev):
    """zero: the default; out of range, negative, NaN, cheb_ratio in (0, 1]: NK_E_INVALID — nothing is replaced silently"""
    name = "chain300cm64"
    M = _matrix(nls, AR.matrix(name), AR.values(name))
    P0 = nls.AMGPreconditioner(M, nu=0, passes=0, theta=0.0, overcorrection=0.0, cheb_ratio=0.0, coarse_max=0)
    Pd = nls.AMGPreconditioner(M, **AR.DEFAULTS)
    assert P0.hierarchy() == Pd.hierarchy() == nls.AMGPreconditioner(M).hierarchy()
    b = AR.rhs_set(300, name)[0]
    assert np.array_equal(P0.apply(b), Pd.apply(b))
    for bad in (dict(nu=17), dict(passes=5), dict(coarse_max=129), dict(nu=-1), dict(passes=-1), dict(coarse_max=-1),
                dict(theta=-0.25), dict(theta=float("nan")), dict(overcorrection=-1.8), dict(overcorrection=float("nan")),
                dict(cheb_ratio=-4.0), dict(cheb_ratio=0.5), dict(cheb_ratio=1.0), dict(cheb_ratio=float("nan"))):
        with pytest.raises(nls.NKError, match=INVALID):
            nls.AMGPreconditioner(M, **bad)
    from nonlinearsolve_jl_amd import _lib as L
    for mt in (3, -1):
        prm, h = L.AMGParams(0, 0, 0, mt, 0.0, 0.0, 0.0), C.c_void_p()
        assert L.lib().nk_precond_create_amg(M._h, C.byref(prm), C.byref(h)) == -1
    # the boundary values themselves are taken
    for ok in (dict(nu=16), dict(passes=4), dict(coarse_max=128), dict(cheb_ratio=1.0000001)):
        nls.AMGPreconditioner(M, **ok).apply(b)
    with pytest.raises(nls.NKError, match=INVALID + ".*level 7 outside"):
        Pd.level_matrix(7)
    with pytest.raises(nls.NKError, match=INVALID):
        Pd.level_matrix(-1)
    _usable(nls)


@pytest.mark.parametrize("matching", AR.MATCHINGS)
@pytest.mark.parametrize("name", ["chain65", "chain200"])
def test_a_failed_update_blocks_apply_until_a_good_update(nls, dev, name, matching):
    A, v0 = AR.matrix(name), AR.values(name)
    n = A.shape[0]
    M = _matrix(nls, A, v0)
    P = nls.AMGPreconditioner(M, matching=matching)
    bad = v0.copy()
    bad[A.indptr[n // 3] + 1] = 0.0                       # (an interior row of a chain: its second entry is the diagonal)
    M.set_values(bad)
    with pytest.raises(nls.NKError, match=SINGULAR):
        P.update()
    b = AR.rhs_set(n, name)[0]
    for x in (b, __import__("torch").tensor(b, device=dev)):
        with pytest.raises(nls.NKError, match=SINGULAR):
            P.apply(x)
    M.set_values(AR.values(name, 1))
    P.update()
    S = AR.structure(name, matching)
    AR.check_structure(S, AR.numbers(S, AR.values(name, 1)), _device_got(P))
    _check_applies(nls, P, name, AR.reference_applies(name, matching, 1), AR.rhs_set(n, name), "recovered: ")


@pytest.mark.parametrize("matching", AR.MATCHINGS)
def test_a_matrix_without_rows(nls, dev, matching):
    import torch
    from nonlinearsolve_jl_amd import _lib as L
    M = nls.CSRMatrix.from_arrays(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    P = nls.AMGPreconditioner(M, matching=matching)
    assert P.hierarchy() == [(0, 0, 1.0)]
    P.update()
    assert P.hierarchy() == [(0, 0, 1.0)]
    assert P.level_matrix(0).info()["nrows_local"] == 0
    # nothing is read or written: one-element buffers come back as they were
    xh, yh = np.full(1, SENTINEL), np.full(1, SENTINEL)
    L.check(L.lib().nk_precond_apply(P._h, C.c_void_p(xh.ctypes.data), C.c_void_p(yh.ctypes.data), L.HOST))
    xd, yd = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev), torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    L.check(L.lib().nk_precond_apply(P._h, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), L.DEVICE))
    assert xh[0] == yh[0] == SENTINEL and float(xd[0]) == float(yd[0]) == SENTINEL
    assert P.apply(np.zeros(0)).shape == (0,)


# ------------------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def general_matrix(n=700):
    """a general (non-grid) CSR matrix: a chain with seeded long-range couplings, diagonally dominant, non-symmetric values"""
    rng = np.random.default_rng(11)
    i = rng.integers(0, n, 3 * n)
    j = rng.integers(0, n, 3 * n)
    keep = i != j
    B = sp.csr_matrix((-rng.uniform(0.1, 1.0, keep.sum()), (i[keep], j[keep])), shape=(n, n))
    B.sum_duplicates()
    B = (B + AR.chain(n) - sp.diags(AR.chain(n).diagonal())).tocsr()
    A = (B + sp.diags(np.asarray(abs(B).sum(axis=1)).ravel() + 0.5)).tocsr()
    A.sort_indices()
    return A


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import nonlinearsolve_jl_amd as nls
        from oracle import reference_restatement as R
        torch.cuda.set_device(0)
        ctx = nls.Context(device=0)
        nls.set_default_context(ctx)
        assert nls.dist.init_comm(ctx, "torch") == "torch"
        dev = torch.device("cuda:0")
        devs = []
        for label, Ag, granule in (("bratu24", AR.bratu(24), 24), ("general700", general_matrix(), 1)):
            n = Ag.shape[0]
            ranges = [nls.partition_range(n, granule, world, r_) for r_ in range(world)]
            b, e = ranges[rank]
            loc = Ag[b:e].tocsr()
            loc.sort_indices()
            J = nls.CSRMatrix.from_arrays(loc.indptr.astype(np.int32), loc.indices.astype(np.int32), loc.data, n_global=n, row_begin=b)
            assert J.info()["n_halo"] > 0
            blk = Ag[b:e, b:e].tocsr()
            blk.sort_indices()
            src = np.nonzero((loc.indices >= b) & (loc.indices < e))[0]          # the block's entries within the rank's rows
            with pytest.raises(nls.NKError, match="status -1:.*without halo columns"):
                nls.AMGPreconditioner(J, matching="handshake")
            P = nls.AMGPreconditioner(J)
            assert P.matching == "greedy"
            rhs = AR.rhs_set(e - b, label + str(rank))
            vals = loc.data.copy()
            O = R.AggregationAMG(blk, matching="greedy")   # the aggregates are those of the creation-time values, for good
            S = AR.structure_from_oracle(O, AR.DEFAULTS)
            for step in range(2):       # the creation-time values, then set_values + update (k_amg_gather)
                O.update(sp.csr_matrix((vals[src], blk.indices, blk.indptr), shape=blk.shape))
                AR.check_structure(S, AR.numbers(S, vals[src]), _device_got(P), f"{label} rank {rank} step {step}: ")
                V = AR.VCycle(S, vals[src], AR.LD)
                row = AR.pow2_up(max(AR.relmax(O(x_), V(x_)) for x_ in rhs))
                bound = max(AR.FACTOR * row, AR.FLOOR)
                assert bound <= AR.LIMIT
                for x_ in rhs:
                    ref = V(x_)
                    for y in (P.apply(x_), P.apply(torch.tensor(x_, device=dev)).cpu().numpy()):
                        devs.append(AR.relmax(y, ref))
                        assert devs[-1] <= bound, (label, rank, step, devs[-1], bound)
                if step == 0:
                    vals = vals * (1.0 + 0.1 * np.random.default_rng(5 + rank).random(len(vals)))
                    J.set_values(vals)
                    P.update()
            # as Pl of the distributed GMRES: the block-diagonal restatement, iteration counts within one
            vg = nls.dist.gather_vector(vals, Ag.nnz, int(Ag.indptr[b]))
            Au = sp.csr_matrix((vg, Ag.indices, Ag.indptr), shape=Ag.shape)
            blocks = [R.AggregationAMG(Ag[b_:e_, b_:e_].tocsr(), matching="greedy").update(Au[b_:e_, b_:e_].tocsr()) for b_, e_ in ranges]

            def Mblock(x_):
                return np.concatenate([blk_(x_[b_:e_]) for blk_, (b_, e_) in zip(blocks, ranges)])
            g = np.random.default_rng(3).standard_normal(n)
            xo, io = R.gmres(lambda z: Au @ z, g, rtol=1e-9, restart=30, itmax=300, ortho="cgs2", Ml=Mblock)
            G = nls.GMRES(e - b, restart=30, ortho="dcgs2").set_operator(J).set_preconditioner(P, side="left")
            x, gi = G.solve(torch.tensor(g[b:e], device=dev), reltol=1e-9, maxiters=300)
            assert gi["converged"] and io.converged and abs(gi["iters"] - io.iters) <= 1, (gi["iters"], io.iters)
            xg = nls.dist.gather_vector(x, n, b)
            assert np.linalg.norm(xg - xo) <= 1e-7 * np.linalg.norm(xo)
        q.put((rank, "ok", max(devs)))
    except Exception:
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), -1.0))
    finally:
        dist.destroy_process_group()


def test_two_ranks_local_blocks(nls, dev):
    """each rank's AMG is that of its local square block Ag[b:e, b:e] (halo columns dropped, host set-up): structure, apply,
    set_values + update through k_amg_gather, the refused device set-up, and block-Jacobi AMG as Pl of the distributed GMRES"""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), res
    print(f"DEVIATION family=two_ranks dev={max(r[2] for r in res):.3e} bound<={AR.LIMIT:.1e}")
