"""Where the launches of a compiled problem are booked by the context's profiler (ctx.profile_enable / profile_report): one
launcher serves the generated kernels of all three kinds (csrc/nk_compiled.hip). From the code — nk_prof_next hands a launch
inside a scope the scope's family, nk_prof_flush counts a family's launch when it carries the scope's bytes (its first) and
every launch of elem_gather, and nk_problems.hip opens one scope around each callback — P.residual, P.jvp and P.jac_values
book one launch each under residual, jvp and jacfill, and an element problem's gather three more under elem_gather.

The callbacks on a stream that is not the context's (which the launcher leaves untimed) are not covered: the Python interface
hands every callback the context's stream."""
import numpy as np
import pytest

import elem_core as EC
import elem_reference as ER
import graph_core as GC
import graph_reference as GR
import grid_reference as G1

pytestmark = pytest.mark.gpu

GENERATED = {"residual": 1, "jvp": 1, "jacfill": 1}


def _grid(nls):
    p = G1.PROBLEMS["bratu"]
    return nls.CompiledGridProblem(p.source, 5, 5, dof=1, stencil="star", boundary=p.boundary, params=p.params)


def _graph(nls):
    p, G = GR.PROBLEMS["cubic"], GR.GRAPHS["ring257"]
    P = nls.CompiledGraphProblem(p.source, *G.csr(), dof=p.dof, params=p.params, edge_data=p.nedge, node_data=p.nnode)
    W, A = GC.data(p, G)
    for k in range(W.shape[0]):
        P.set_edge_data(k, W[k])
    for k in range(A.shape[0]):
        P.set_node_data(k, A[k])
    return P


def _elem(nls):
    p, M = ER.PROBLEMS["diffusion"], ER.MESHES["tri2"]
    P = nls.CompiledElementProblem(p.source, M.conn32(), M.nn, dof=p.dof, params=p.params, node_data=p.nnode, elem_data=p.nelem)
    A, W = EC.data(p, M)
    for k in range(A.shape[0]):
        P.set_node_data(k, A[k])
    for k in range(W.shape[0]):
        P.set_elem_data(k, W[k])
    return P


@pytest.mark.parametrize("make,expected", [(_grid, GENERATED), (_graph, GENERATED), (_elem, dict(GENERATED, elem_gather=3))],
                         ids=["grid", "graph", "element"])
def test_each_callback_books_its_launches(nls, dev, make, expected):
    import torch
    P = make(nls)
    try:
        rng = np.random.default_rng(7)
        u = torch.tensor(0.1 * rng.standard_normal(P.n_local), dtype=torch.float64, device=dev)
        v = torch.tensor(rng.standard_normal(P.n_local), dtype=torch.float64, device=dev)
        J = P.jac_csr()
        P.ctx.profile_enable(True)
        try:
            P.residual(u)
            P.jvp(v, u)
            P.jac_values(u, J)
            report = P.ctx.profile_report()
        finally:
            P.ctx.profile_enable(False)
        booked = {k: r["launches"] for k, r in report.items()}
        print(f"{make.__name__}: booked {booked}")
        for family in ("residual", "jvp", "jacfill", "elem_gather"):
            assert booked.get(family, 0) == expected.get(family, 0), (family, booked)
    finally:
        P.close()
