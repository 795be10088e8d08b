#!/usr/bin/env python
"""One SHA-256 per case of the raw output bytes of the preconditioned solves: the Chebyshev polynomial (fused in the CSR row
epilogue, unfused behind a callable operator and behind a shift), the Bratu and Brusselator V-cycles, the aggregation AMG and
the grid multigrid of a compiled problem. Two builds of the library that print the same listing compute the same bits.

    python tools/precond_bits.py [case-prefix …]      (needs the GPU)

The library reads NK_MG_GRAPH once per process: run the "bratu vcycle" cases a second time with NK_MG_GRAPH=0 for the plain
launches (the case names carry the value)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def _csr(nls, A):
    return nls.CSRMatrix.from_arrays(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data)


def cases(nls, R):
    from nonlinearsolve_jl_amd import _lib as L
    rng = np.random.default_rng(7)

    # ---- GMRES(30), fixed_iters = 5, Chebyshev polynomial of degree 1, 2, 8 on the Bratu 33² Jacobian (n = 1089: odd)
    pb = R.Bratu2D(33, 6.0)
    u = pb.u0() + 0.1 * rng.standard_normal(pb.n)
    J = pb.jac(u).tocsr()
    b = rng.standard_normal(pb.n)
    A = _csr(nls, J)
    lam = float(abs(J).sum(axis=1).max())
    for degree in (1, 2, 8):
        for form in ("csr", "callable", "shift"):
            def run(degree=degree, form=form):
                G = nls.GMRES(pb.n, restart=30, ortho="cgs2")
                G.set_operator(A if form != "callable" else (lambda x: A.matvec(x)))
                if form == "shift":
                    L.check(L.lib().nk_gmres_set_shift(G._h, 0.75))
                G.set_chebyshev_preconditioner(degree, lam / 30.0, lam)
                x, _ = G.solve(b, fixed_iters=5)
                G.close()
                return _sha(x)
            yield f"cheb degree={degree} {form}", run

    # ---- the Bratu V-cycle, ns = 63, coarse_max = 15
    for nu in (1, 2, 3):
        def run(nu=nu):
            P = nls.Bratu2D(63, 6.0)
            pr = R.Bratu2D(63, 6.0)
            uu = pr.u0() + 0.1 * np.random.default_rng(3).standard_normal(pr.n)
            op = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), uu)
            G = nls.GMRES(pr.n, restart=30, ortho="cgs2").set_operator(op)
            G.set_multigrid_preconditioner(P, uu, nu=nu, coarse_max=15)
            bb = np.random.default_rng(4).standard_normal(pr.n)
            out = [G.solve(bb, fixed_iters=k)[0] for k in (1, 3)]
            G.close()
            return _sha(*out)
        yield f"bratu vcycle nu={nu} NK_MG_GRAPH={os.environ.get('NK_MG_GRAPH', 'unset')}", run

    # ---- the Brusselator V-cycle, N = 32, nu = 2, coarse_max = 8
    def run():
        pr = R.Brusselator2D(32)
        uu = pr.u0() + 0.05 * np.random.default_rng(1).standard_normal(pr.n)
        P = nls.Brusselator2D(32)
        op = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), uu)
        G = nls.GMRES(pr.n, restart=30, ortho="cgs2").set_operator(op)
        G.set_multigrid_preconditioner(P, uu, nu=2, coarse_max=8)
        bb = np.random.default_rng(2).standard_normal(pr.n)
        out = [G.solve(bb, fixed_iters=k)[0] for k in (1, 3)]
        G.close()
        return _sha(*out)
    yield "brusselator vcycle N=32 nu=2", run

    # ---- AMGPreconditioner.apply: Bratu 24² (dense coarsest level), stall600 (Chebyshev coarsest level)
    import amg_reference as AR
    p24 = R.Bratu2D(24, 6.0)
    mats = {"bratu24": (p24.jac(p24.u0() + 0.1 * np.random.default_rng(5).standard_normal(p24.n)).tocsr(), {}),
            "stall600": (AR.matrix("stall600"), dict(AR.CASES["stall600"].params))}
    for name, (M, params) in mats.items():
        for nu in (1, 2):
            def run(M=M, params=params, nu=nu):
                Pm = nls.AMGPreconditioner(_csr(nls, M.tocsr()), **dict(params, nu=nu))
                sizes = [h[0] for h in Pm.hierarchy()]
                y = Pm.apply(np.random.default_rng(6).standard_normal(M.shape[0]))
                return _sha(y) + f"  levels {sizes}"
            yield f"amg {name} nu={nu}", run

    # ---- the grid multigrid of a 17² compiled problem, nu = 2
    def run():
        import gridmg_reference as GM
        from grid_device import create
        ref = GM.reference("bratu", (17, 17), 4)
        P = create(nls, ref.prob, (17, 17))
        op = nls.StatefulJacobianOperator(nls.JacobianOperator(nls.NonlinearProblem(P)), ref.u)
        G = nls.GMRES(ref.u.size, restart=30, ortho="cgs2").set_operator(op)
        G.set_multigrid_preconditioner(P, ref.u, nu=2, coarse_max=4)
        out = [G.solve(ref.b, fixed_iters=k)[0] for k in (1, 3)]
        G.close()
        return _sha(*out)
    yield "gridmg 17x17 nu=2", run


def main():
    import nonlinearsolve_jl_amd as nls
    from oracle import reference_restatement as R
    want = sys.argv[1:]
    for name, run in cases(nls, R):
        if not want or any(name.startswith(w) for w in want):
            print(f"{run()}  {name}", flush=True)


if __name__ == "__main__":
    main()
