"""Compiled grid problems on several ranks on the device (csrc/nk_grid.hip, slabs of the outermost axis): two and three
processes share cuda:0 as in tests/test_gpu_multirank.py, collectives go through the callback communicator over
torch.distributed/gloo or the peer-mapped arenas. Every rank builds, for each case, the slab problem on the multi-rank context
and the one-rank problem on a second, communicator-free Context in the same process, and compares its slice:

  * residual, J·v and the fill values equal the one-rank device results moved by the permutation, BIT FOR BIT — the same
    nk_point on the same inputs;
  * residual, J·v, the fill values, Jᵀv (P.vjp) and the filled matrix times v meet the project's bound against the restatement
    tests/gridmr_reference.py:  |device − float64| <= 16 × |float64 − long double| + 4 eps × Σ|terms|;
  * J.info()["n_halo"] is the number of distinct ghost unknowns the pattern names;
  * fields round-trip the slab, and a field changed on one rank changes the neighbour's residual on its boundary line;
  * NewtonRaphson + GMRES + Eisenstat–Walker, matrix-free and with a concrete Jacobian, against the one-rank solve in the same
    process with the thresholds of the multi-rank Bratu test; conservation between zero-flux walls across the cut.

The Bratu solve: the issue's channel {"x": "periodic", "y": "mirror_face"} has no regular root for Bratu's source — the
Laplacian sums to zero between zero-flux walls, so Σ F = −c·Σ exp(u) < 0 and Newton can only run off to u → −∞ along the
singular constant mode. The channel solved here keeps the mirror-face wall on the low side of the split axis and holds the
high side at Dirichlet-0 ({"x": "periodic", "y": ("mirror_face", "dirichlet")}); every threshold is the issue's."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (case of gridmr_reference.PROBLEMS, shape or None for the smallest that splits): the cases of two ranks
CASES_2 = [("bratu_ydir", None), ("bratu_yper", None), ("bratu_ymnode", None), ("bratu_ymface", None), ("bratu_ymixed", None),
           ("bratu_xper_yper", None), ("bratu_xmface_ymixed", None), ("brus_site_yper", None), ("brus_site_ydir", None),
           ("box_xmface_yper", None), ("box_xmnode_ymixed", None), ("star2_yper", None), ("star2_ydir", None),
           ("diamond2_ymnode", None), ("diamond2_yper", None), ("star3_zper", (4, 3, 5)), ("star3_zmixed", (4, 3, 5)),
           ("star2_3_zmnode", None), ("vardiff_yper", None), ("vardiff_ymface", None),
           ("brus_site_yper", (40, 14)), ("box_xmnode_ymixed", (40, 14))]   # slabs of 280 nodes: a piece boundary inside the slab
CASES_PEER = [("bratu_yper", None), ("box_xmface_yper", None), ("vardiff_ymface", None)]
CASES_3 = [("brus_site_ydir", None), ("brus_site_yper", None), ("star2_ydir", None), ("star2_yper", None)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, transport, plan):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import hashlib
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    digest, log = {}, []

    def note(key, arr):   # what the parent compares bit for bit between the transports
        digest[key] = hashlib.sha1(np.ascontiguousarray(arr).tobytes()).hexdigest()

    try:
        import nonlinearsolve_jl_amd as nls
        import grid_core as GC
        import grid_device as D
        import gridmr_reference as R
        torch.cuda.set_device(0)
        ctx = nls.Context(device=0)
        nls.set_default_context(ctx)
        assert nls.dist.init_comm(ctx, transport) == ("none" if world == 1 else "torch" if transport == "torch" else "peer+torch")
        assert ctx.comm_info()[1:] == (world, rank)
        one = nls.Context(device=0)            # communicator-free: the one-rank problems of this process
        assert one.comm_info()[1] == 1
        dev = torch.device("cuda:0")

        def t(x):
            return D.to_device(x, dev)

        def create(prob, shape, c, params=None):
            return D.create(nls, prob, shape, params, ctx=c)

        def parity(name, shape):
            prob = R.PROBLEMS[name]
            shape = tuple(shape or R.small_shape(prob, world))
            ref, S = GC.reference(prob, shape), R.slab(name, shape, world, rank)
            tag = f"{name} {'x'.join(map(str, shape))} rank {rank}/{world}"
            Pm, P1 = create(prob, shape, ctx), create(prob, shape, one)
            assert Pm.lines == S.lines and P1.lines == (0, shape[-1])
            assert (Pm.n_local, Pm.n_global, Pm.row_begin, Pm.nn) == (S.n_local, S.n_global, S.row_begin, S.nn_loc)
            assert np.array_equal(Pm.local_of(ref.u), S.local(ref.u))
            if prob.nfields:
                for k in range(prob.nfields):
                    P1.set_field(k, ref.fields[k])
                    mine = ref.fields[k][S.rows[:S.nn_loc]]
                    Pm.set_field(k, mine)
                    assert np.array_equal(Pm.field(k).cpu().numpy(), mine)           # round trip of the slab
            got = D.device_quantities(Pm, S.local(ref.u), S.local(ref.v), dev)
            full = D.device_quantities(P1, ref.u, ref.v, dev)
            info = Pm.jac_csr().info()
            assert info["nrows_local"] == S.n_local and info["nnz"] == S.colind.size and info["n_halo"] == S.n_halo, (tag, info)
            want = R.expected(name, shape, world, rank)
            for k in D.QUANTITIES:
                exp, bound = want[k]
                err = np.abs(got[k] - exp)
                log.append(f"{tag} {k}: max err {err.max():.3e}, max bound {bound.max():.3e}, worst err - bound "
                           f"{float(np.max(err - bound)):.3e}")
                assert np.all(np.isfinite(got[k])), (tag, k)
                assert np.all(err <= bound), (tag, k, float(np.max(err - bound)))
            for k in ("f", "jv", "vals"):     # the one-rank device results, moved: bit for bit
                moved = S.values(full[k]) if k == "vals" else S.local(full[k])
                same = int(np.sum(got[k] == moved))
                log.append(f"{tag} {k}: {same}/{moved.size} bitwise equal to the one-rank device result")
                assert np.array_equal(got[k], moved), (tag, k, same, moved.size)
                note(f"{name}-{'x'.join(map(str, shape))}-{k}", got[k])
            Pm.close()
            P1.close()

        def solve_pair(name, prob, shape, params, start):
            """NewtonRaphson + GMRES + Eisenstat–Walker on the slabs against the one-rank solve in this process"""
            Pm, P1 = create(prob, shape, ctx, params), create(prob, shape, one, params)
            for concrete in (False, True):
                alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), forcing=nls.EisenstatWalkerForcing2(), concrete_jac=concrete)
                s1 = nls.solve(nls.NonlinearProblem(P1, u0=t(start)), alg, abstol=1e-9, maxiters=50)
                sm = nls.solve(nls.NonlinearProblem(Pm, u0=t(Pm.local_of(start))), alg, abstol=1e-9, maxiters=50)
                ug = nls.dist.gather_grid(Pm, sm.u)
                du = float(np.max(np.abs(ug - s1.u.cpu().numpy())))
                log.append(f"{name} concrete={concrete} rank {rank}: {sm.retcode}/{s1.retcode}, steps {sm.stats.nsteps}/"
                           f"{s1.stats.nsteps}, max|du| {du:.3e}, halo {sm.stats.halo_exchanges}, allreduces {sm.stats.allreduces}")
                assert sm.retcode == "Success" and s1.retcode == "Success"
                assert np.max(np.abs(s1.u.cpu().numpy() - start)) > 1e-3       # (the root is not the initial guess)
                assert du <= 1e-7
                assert abs(sm.stats.nsteps - s1.stats.nsteps) <= 1
                assert sm.stats.halo_exchanges > 0 and sm.stats.allreduces > 0
                note(f"solve-{name}-{concrete}", ug)
            Pm.close()
            P1.close()

        def bratu_solve():
            import grid_reference as G1
            shape, params = (24, 20), [1.0, 1e-3]
            prob = G1.PROBLEMS["bratu"].with_boundary("bratu_channel_mr", (R.PE, R.PE, R.MF, R.DI))
            solve_pair("bratu_channel", prob, shape, params, 0.5 * GC.inputs(prob, shape)[0])

        if plan == "full2":
            for name, shape in CASES_2:
                parity(name, shape)
            # ---------------- a field changed on one rank changes the neighbour's residual on its boundary line (and only there)
            name, shape = "vardiff_yper", (4, 5)
            prob, S = R.PROBLEMS[name], R.slab(name, shape, world, rank)
            ref = GC.reference(prob, shape)
            Pm = create(prob, shape, ctx)
            for k in range(prob.nfields):
                Pm.set_field(k, ref.fields[k][S.rows[:S.nn_loc]])
            ul = t(S.local(ref.u))
            f0 = Pm.residual(ul).cpu().numpy()
            kappa = ref.fields[1][S.rows[:S.nn_loc]].copy()
            if rank == 1:
                kappa[:shape[0]] += 0.5        # rank 1's first line (line 2 of the grid): rank 0's last line reads it
            Pm.set_field(1, kappa)             # (collective: both ranks call it)
            f1 = Pm.residual(ul).cpu().numpy()
            changed = (f0 != f1).reshape(-1, shape[0]).any(axis=1)
            log.append(f"field across the cut, rank {rank}: lines changed {changed.tolist()}")
            assert changed.tolist() == ([False, True] if rank == 0 else [True, True, False])
            Pm.close()
            # ---------------- solves
            bratu_solve()
            import grid_reference as G1
            shape = (16, 12)
            prob = G1.PROBLEMS["brusselator"].with_boundary("brus_mr", (R.PE, R.PE, R.MF, R.MF))
            nn = shape[0] * shape[1]
            start = np.concatenate([np.full(nn, 1.0), np.full(nn, 3.4)]) + 0.05 * GC.inputs(prob, shape)[0]
            solve_pair("brusselator", prob, shape, None, start)
            # ---------------- conservation: zero-flux walls on all sides, a divergence-form source — the fluxes telescope
            # to zero over the whole grid, so the all-reduced sum of the residual is the reaction part's alone, here
            # Σ p0·(u − a0) − Σ a2; the bound is the rounding of the sums (gridbc's conservation test, split across the cut)
            name, shape = "vardiff_ymface", (24, 20)
            prob = R.PROBLEMS[name]
            S = R.Slab(shape, prob.dof, prob.offsets(), prob.sides, world, rank)
            u = GC.inputs(prob, shape)[0]
            fields = GC.seeded_fields(3, shape)
            fields[0], fields[2] = u, 0.0 * u          # a0 = u and no source: F is the flux divergence alone
            Pm = create(prob, shape, ctx)
            for k in range(3):
                Pm.set_field(k, fields[k][S.rows[:S.nn_loc]])
            f = Pm.residual(t(S.local(u))).cpu().numpy()
            parts = [None] * world
            dist.all_gather_object(parts, (float(np.sum(f.astype(np.longdouble))), float(np.abs(f).sum())))
            total, mag = sum(p[0] for p in parts), sum(p[1] for p in parts)
            # A face's flux p1·½(κ + κ_nb)(u − u_nb) is computed from the same operands on both of its sides and differs in sign
            # only, so in exact sums the total is 0; what is left is the rounding of each node's five-term accumulation, at most
            # 8 eps × Σ|terms of the node| (the project's floor with the accumulation's depth for margin). Σ over the nodes of
            # Σ|terms| <= p1 · κ̄ · Σ_faces (|u| + |u_nb|) <= p1 · 1.5 · 8 · Σ|u| (4 faces, κ̄ <= 1.37)
            terms = 8.0 * prob.params[1] * 1.5 * float(np.abs(u).sum())
            bound = 8 * GC.EPS * terms
            log.append(f"conservation rank {rank}: |sum F| {abs(total):.3e}, bound {bound:.3e}, |F|_1 {mag:.3e}")
            assert mag > 1e6 * bound and abs(total) <= bound
            Pm.close()
        elif plan == "peer2":
            for name, shape in CASES_PEER:
                parity(name, shape)
            bratu_solve()
            assert ctx.comm_peer_status()[1] == 0
        elif plan == "torch2_for_peer":
            for name, shape in CASES_PEER:
                parity(name, shape)
            bratu_solve()
        elif plan == "three":
            for name, shape in CASES_3:
                parity(name, shape)
        elif plan == "one":
            # a one-rank context of the multi-rank-capable build: the slab is the grid
            name, shape = "brus_site_yper", (4, 5)
            prob = R.PROBLEMS[name]
            ref = GC.reference(prob, shape)
            P1 = create(prob, shape, ctx)
            assert P1.lines == (0, 5) and P1.row_begin == 0 and P1.n_local == P1.n_global == ref.u.size
            got = D.device_quantities(P1, ref.u, ref.v, dev)
            for k in D.QUANTITIES:
                assert np.all(np.abs(got[k] - getattr(ref, k)) <= getattr(ref, k + "_bound")), k
            assert np.array_equal(P1.to_full(P1.local_of(ref.u)), ref.u)
        q.put((rank, "ok", digest, log))
    except Exception:
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), {}, log))
    finally:
        dist.destroy_process_group()


def _run(world, transport, plan):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, transport, plan)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=280) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for r in sorted(res):
        print("\n".join(r[3]))
    assert all(r[1] == "ok" for r in res), [r[:2] for r in res]
    return {r[0]: r[2] for r in res}


_DIGESTS = {}


def test_two_ranks_callback_transport():
    """every case of CASES_2, the field across the cut, the two solves and the conservation check in one worker set"""
    _run(2, "torch", "full2")


def test_two_ranks_peer_transport_equals_the_callback_transport():
    """residual, J·v and fill of three cases and one solve with the peer-mapped halo exchange and all-reduce: SHA digests equal
    the callback transport's (the parent-side comparison of test_two_ranks_on_one_gpu_peer_comm)"""
    _DIGESTS["torch"] = _run(2, "torch", "torch2_for_peer")
    _DIGESTS["peer"] = _run(2, "peer", "peer2")
    assert _DIGESTS["peer"] == _DIGESTS["torch"] and all(len(d) > 0 for d in _DIGESTS["peer"].values())


def test_three_ranks_have_an_interior_rank():
    """radius 1 at ny = 7 (2|2|3) and radius 2 at ny = 9, Dirichlet and periodic on the split axis, dof 2: the only place a rank
    with a cut on both sides and two different neighbours runs"""
    _run(3, "torch", "three")


def test_one_rank_context_is_unchanged():
    """a process group of one: P.lines == (0, n_outer), the five arrays under the restatement's bound"""
    _run(1, "torch", "one")
