"""What the device tests of the compiled grid problems share (tests/test_gpu_grid*.py): host ↔ device conversion, the check of
one quantity against the restatement's bound, the five quantities of a problem, the creation of a CompiledGridProblem from a
grid_core.Problem, the problems the tests keep for a whole module, and the parity test's body."""
import numpy as np

import grid_core as GC

QUANTITIES = ("f", "jv", "vals", "jtv", "spmv")
_PROBLEMS = {}


def to_device(x, dev):
    import torch
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, device=dev)


def to_numpy(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def check(what, got, ref, bound, exact=False):
    """exact: the case agrees bit for bit (measured on the MI355X), so that is what is asserted"""
    err = np.abs(got - ref)
    worst = float(np.max(err - bound))
    same = int(np.sum(got == ref))
    print(f"{what}: max err {err.max():.3e}, max bound {bound.max():.3e}, min bound {bound.min():.3e}, worst err - bound "
          f"{worst:.3e}, bitwise equal {same}/{got.size}")
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= bound), (what, worst)
    if exact:
        assert np.array_equal(got, ref), what


def device_quantities(P, u, v, dev):
    """residual, J·v, CSR values of the fill, Jᵀv and the filled matrix times v"""
    du, dv = to_device(u, dev), to_device(v, dev)
    J = P.jac_csr()
    P.jac_values(du, J)
    return dict(f=to_numpy(P.residual(du)), jv=to_numpy(P.jvp(dv, du)), vals=np.array(J.values()), jtv=to_numpy(P.vjp(dv, du)),
                spmv=to_numpy(J.matvec(dv)))


def create(nls, prob, shape, params=None, **kw):
    return nls.CompiledGridProblem(prob.source, shape[0], shape[1], dof=prob.dof, stencil=prob.stencil, boundary=prob.boundary,
                                   params=prob.params if params is None else params, nz=shape[2] if prob.dim == 3 else None,
                                   fields=prob.nfields, **kw)


def set_fields(P, fields):
    for k in range(P.nfields):
        P.set_field(k, fields[k])


def problem(nls, prob, shape):
    """one compiled problem per case for the whole module, holding the seeded fields (whoever changes the fields or the
    parameters puts them back)"""
    key = (prob, tuple(shape))
    if key not in _PROBLEMS:
        _PROBLEMS[key] = create(nls, prob, shape)
        if prob.nfields:
            set_fields(_PROBLEMS[key], GC.seeded_fields(prob.nfields, shape))
    return _PROBLEMS[key]


def close_problems():
    """the problems the module shared are freed; a double close is harmless"""
    for P in _PROBLEMS.values():
        P.close()
        P.close()
    _PROBLEMS.clear()


def assert_parity(nls, dev, prob, shape, exact):
    """the five quantities of the shared problem of a case against the shared reference, every entry within its bound (bit for
    bit where `exact`), then the consistency of fill and JVP: the filled matrix times v against the dual JVP within the sum of
    the two bounds. Returns (P, ref)"""
    ref, P = GC.reference(prob, shape), problem(nls, prob, shape)
    assert P.n_local == ref.u.size and P.jac_csr().info()["nnz"] == ref.vals.size
    got = device_quantities(P, ref.u, ref.v, dev)
    tag = f"{prob.name} {'x'.join(map(str, shape))}"
    for k in QUANTITIES:
        check(f"{tag} {k}", got[k], getattr(ref, k), getattr(ref, k + "_bound"), exact=exact)
    diff = np.abs(got["spmv"] - got["jv"])
    print(f"{tag} fill·v vs dual JVP: max {diff.max():.3e}")
    assert np.all(diff <= ref.spmv_bound + ref.jv_bound)
    return P, ref
