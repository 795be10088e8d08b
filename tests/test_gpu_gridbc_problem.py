"""Compiled grid problems with a boundary kind per side on the device (csrc/nk_grid.hip, NK_GRID_SIDES): the generated residual,
dual-number JVP and Jacobian-fill kernels under mirror walls, channels and mixed sides, against the NumPy restatement
(tests/grid_core.py, tests/gridbc_reference.py), entry by entry within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

then the direct form of the fill in a fresh process, conservation of an implicit Euler step between zero-flux walls, solves
against a dense NumPy Newton on the restatement, and a packed all-periodic code against the plain one, bit for bit. Every figure
is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_core as GC
import grid_reference as G1
import gridbc_reference as R
from grid_device import (QUANTITIES, assert_parity, check, close_problems, create, device_quantities, problem, to_device,
                         to_numpy)

pytestmark = pytest.mark.gpu

_SOLVE_PROBLEMS = {}   # the problems of the solves, with their own parameters
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ parity with the restatement
_CASES = [(name, shape) for name in sorted(R.PROBLEMS) for shape in R.sizes(R.PROBLEMS[name])]


@pytest.mark.parametrize("name,shape", _CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in _CASES])
def test_parity_with_the_restatement(nls, dev, name, shape):
    """Each stencil's existing shapes — 3 × 3, 5 × 5 at radius 2, 3 × 3 × 3: every row wraps or mirrors, the box's corners merge
    four (eight) points into one entry; 37 × 29 (× 3): five workgroups, the last ragged; 300 × 5. Residual, JVP, the merged fill
    and the transposed product, every entry, then the consistency of fill and JVP: the filled matrix times v against the dual
    JVP within the sum of the two bounds. The merge is plain additions in the restatement's order (ascending stencil point), so
    sources without an elementary function are expected to agree bit for bit; what the MI355X showed is recorded at EXACT
    below and asserted."""
    prob = R.PROBLEMS[name]
    assert problem(nls, prob, shape).boundary == prob.boundary
    assert_parity(nls, dev, prob, shape, exact=name in EXACT)


# The problems whose five quantities agreed BIT FOR BIT with the restatement at all their shapes on the MI355X: every problem
# without an elementary function (80 of 80 comparisons, every entry) — wrap, mirror and the merge feed the same +, −, × in the
# restatement's order, four- and eight-way corner merges included. The Bratu and box sources have an exp: they differ from NumPy
# in its last bits at a few entries (bratu_mirror_node / _mirror_face / _plate 22455 / 22455 / 22461 of 22484 entries equal,
# bratu_channel 22533 of 22558, box_* 104489 and 104484 of 104608; max error 8.9e-16) and are held to the rule.
EXACT = ("box3_mirror", "brusselator_xface_yper", "diamond2_mirror", "star2_mirror", "star3_mixed", "vardiff_mirror_face")


# ------------------------------------------------------------------------------------------------ the direct form of the fill
_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import nonlinearsolve_jl_amd as nls
import grid_core as GC
import gridbc_reference as R
name, shape = sys.argv[2], tuple(int(x) for x in sys.argv[3].split("x"))
prob = R.PROBLEMS[name]
ref = GC.reference(prob, shape)
P = nls.CompiledGridProblem(prob.source, shape[0], shape[1], dof=prob.dof, stencil=prob.stencil, boundary=prob.boundary,
                            params=prob.params)
u = torch.tensor(ref.u, dtype=torch.float64, device="cuda:0")
J = P.jac_csr()
P.jac_values(u, J)
np.save(sys.argv[4], np.array(J.values()))
P.close()
"""


def test_direct_fill_in_a_fresh_process(nls, dev, tmp_path):
    """NK_GRID_FILL_DIRECT=1 (every thread stores its own merged partials, no staging in LDS): the box mirrored in both axes at
    37 × 29, once, in a child process of its own; the values under the restatement's bound and equal to the staged form's"""
    name, shape = "box_mirror", (37, 29)
    ref = GC.reference(R.PROBLEMS[name], shape)
    out = tmp_path / "vals.npy"
    env = dict(os.environ, NK_GRID_FILL_DIRECT="1")
    done = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, "x".join(map(str, shape)), str(out)], env=env,
                          capture_output=True, text=True, timeout=300)
    print(done.stdout[-2000:], done.stderr[-2000:])
    assert done.returncode == 0
    direct = np.load(out)
    check("box_mirror 37x29 vals, direct fill", direct, ref.vals, ref.vals_bound)
    P = problem(nls, R.PROBLEMS[name], shape)
    J = P.jac_csr()
    P.jac_values(to_device(ref.u, dev), J)
    assert np.array_equal(direct, np.array(J.values()))


# ------------------------------------------------------------------------------------------------ conservation
def _heat_fields(shape, level):
    f = GC.seeded_fields(3, shape)
    return np.stack([level, f[1], np.zeros_like(level)])


def test_implicit_euler_between_zero_flux_walls_conserves_the_sum(nls, dev):
    """vardiff as implicit Euler, F(u) = (u − a₀)/dt − Σ_faces ½(κ + κ_nb)(u_nb − u) with mirror-face on all sides, 24 × 20, three
    steps through init / set_field / reinit_ / solve_. Summing F over the grid telescopes the fluxes to zero, so after each
    step |Σu_new − Σa₀| <= dt·‖F(u_new)‖₁ + 8·nn·eps·Σ|u|, F by the restatement. The same problem with Dirichlet-0 walls
    violates that bound by a factor >= 1e6 (also shown without a GPU in tests/test_gridbc_reference.py)."""
    shape, dt = (24, 20), 0.05
    nn, params = 24 * 20, [1.0 / dt, 1.0]
    a_start = 1.0 + 0.5 * np.cos(0.3 * np.arange(nn))
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(), concrete_jac=True)
    worst = {}
    for tag, prob in (("mirror_face", R.PROBLEMS["vardiff_mirror_face"]), ("dirichlet", R.DIRICHLET_TWIN["vardiff_mirror_face"])):
        P = create(nls, prob, shape, params)
        fields = _heat_fields(shape, a_start)
        for k in range(3):
            P.set_field(k, fields[k])
        cache = nls.init(nls.NonlinearProblem(P, to_device(a_start, dev)), alg, abstol=1e-10, maxiters=40)
        ratios = []
        for step in range(3):
            P.set_field(0, cache.u)
            nls.reinit_(cache, u0=cache.u)
            sol = nls.solve_(cache)
            a0, u = to_numpy(P.field(0)), to_numpy(cache.u)
            fields = _heat_fields(shape, a0)
            f = GC.evaluate(prob, shape, u, u, fields, params=params).f
            drift = abs(float(np.sum(u.astype(GC.LD)) - np.sum(a0.astype(GC.LD))))
            bound = dt * float(np.abs(f).sum()) + 8 * nn * GC.EPS * float(np.abs(u).sum())
            print(f"{tag} step {step}: {sol.retcode}; |sum u - sum a0| {drift:.3e}, bound {bound:.3e}, |F|_1 {np.abs(f).sum():.3e}, "
                  f"|u - a0| {np.abs(u - a0).max():.3e}")
            assert sol.retcode == "Success"
            assert np.abs(u - a0).max() > 1e-4          # (the level moved: a step that did nothing would conserve too)
            ratios.append((drift, bound))
        worst[tag] = ratios
        cache.close()
        P.close()
    assert all(d <= b for d, b in worst["mirror_face"])
    assert all(d >= 1e6 * b for d, b in worst["dirichlet"])


# ------------------------------------------------------------------------------------------------ solves
def _algorithms(nls):
    """The left-preconditioned solve measures M⁻¹r: it gets a linear abstol of its own, 1e-12, as the fields tests found
    necessary (tests/test_gpu_gridf_problem.py)."""
    G = nls.KrylovJL_GMRES
    return {
        "newton_assembled": nls.NewtonRaphson(linsolve=G(), concrete_jac=True),
        "newton_matfree": nls.NewtonRaphson(linsolve=G()),
        "newton_ilu0": nls.NewtonRaphson(linsolve=G(abstol=1e-12, precs=nls.ObjectPrecs("ilu0", "left")), concrete_jac=True),
        "trust_region": nls.TrustRegion(linsolve=G()),
    }


_REFERENCE_ROOTS = {}
# The channel is 20 rows between a Dirichlet-0 wall and a symmetry line: the strip 0 < y < 41 of −u″ = c·eᵘ, which has a solution
# only for c < 3.51/41² = 2.1e-3. The table's c = 0.04 (a residual to compare, not a problem to solve) is beyond it; 1e-3 is not.
SOLVE_PARAMS = {"bratu_channel": [1.0, 1e-3], "star3_mixed": None}


def _start(name, shape):
    """the initial guess of the solves: half the case's seeded u, |u0| <= 0.5. Not zero: TrustRegion's largest radius is
    max(‖F(u0)‖₂, max u0 − min u0) (the reference's rule), which at u0 = 0 of the channel is ‖F(0)‖₂ = 0.022 against a root 4
    away in the 2-norm — sixty steps of that length end as MaxIters, as the first device run showed"""
    return 0.5 * GC.inputs(R.PROBLEMS[name], shape)[0]


def _reference_root(name, shape):
    """u_ref with ‖F(u_ref)‖∞ <= 1e-12 by a dense NumPy Newton on the restatement from the same start, ‖F(u_ref)‖∞ and
    ‖J(u_ref)⁻¹‖∞"""
    if (name, shape) not in _REFERENCE_ROOTS:
        prob, par = R.PROBLEMS[name], SOLVE_PARAMS[name]
        u = GC.dense_newton(prob, shape, _start(name, shape), params=par, tol=1e-12, maxiters=40)
        J, f = GC.dense_jacobian(prob, shape, u, params=par)
        assert np.abs(f).max() <= 1e-12
        _REFERENCE_ROOTS[(name, shape)] = (u, float(np.abs(f).max()), float(np.linalg.norm(np.linalg.inv(J), np.inf)))
    return _REFERENCE_ROOTS[(name, shape)]


@pytest.mark.parametrize("algname", ["newton_assembled", "newton_matfree", "newton_ilu0", "trust_region"])
@pytest.mark.parametrize("name,shape", [("bratu_channel", (24, 20)), ("star3_mixed", (7, 6, 5))])
def test_solves_like_a_dense_newton(nls, dev, name, shape, algname):
    """the Bratu channel (x periodic, a Dirichlet-0 wall below, a mirror-node line above) at 24 × 20 and the 3-D star, dof 2, with
    three different axes at 7 × 6 × 5, from a seeded start: |u_dev − u_ref|∞ <= 2·‖J(u_ref)⁻¹‖∞·(‖F(u_dev)‖∞ + ‖F(u_ref)‖∞), both
    residuals by the restatement, the factor 2 for the second-order term — the tolerance of tests/test_gpu_gridf_problem.py"""
    prob, par, abstol = R.PROBLEMS[name], SOLVE_PARAMS[name], 1e-10
    u_ref, f_ref, jinv = _reference_root(name, shape)
    if name not in _SOLVE_PROBLEMS:
        _SOLVE_PROBLEMS[name] = create(nls, prob, shape, par)
    P = _SOLVE_PROBLEMS[name]
    sol = nls.solve(nls.NonlinearProblem(P, to_device(_start(name, shape), dev)), _algorithms(nls)[algname], abstol=abstol, maxiters=60)
    u_dev = to_numpy(sol.u)
    f_dev = float(np.abs(GC.evaluate(prob, shape, u_dev, u_dev, params=par).f).max())
    err, bound = float(np.abs(u_dev - u_ref).max()), 2.0 * jinv * (f_dev + f_ref)
    print(f"{name} {algname}: {sol.retcode} {sol.stats}; |u_dev - u_ref| {err:.3e}, bound {bound:.3e} (|J^-1| {jinv:.3e}, "
          f"|F(u_dev)| {f_dev:.3e}, |F(u_ref)| {f_ref:.3e}); |u_ref| {np.abs(u_ref).max():.3e}")
    assert sol.retcode == "Success"
    assert np.abs(u_ref - _start(name, shape)).max() > 1e-3          # (the root is not the initial guess)
    assert err <= bound
    assert f_dev <= abstol + float(GC.Reference(prob, shape, u_dev, u_dev, params=par).f_bound.max())


# ------------------------------------------------------------------------------------------------ the old paths
def test_a_packed_all_periodic_code_is_the_periodic_problem(nls, dev):
    """created with a kind per side, all periodic: the five arrays of the problem created with "periodic", bit for bit"""
    name, shape = "box_periodic", (37, 29)
    p = G1.PROBLEMS[name]
    ref = GC.reference(p, shape)
    plain = nls.CompiledGridProblem(p.source, *shape, dof=p.dof, stencil=p.stencil, boundary="periodic", params=p.params)
    packed = nls.CompiledGridProblem(p.source, *shape, dof=p.dof, stencil=p.stencil, boundary=("periodic",) * 4, params=p.params)
    assert packed.boundary == ("periodic",) * 4
    a, b = device_quantities(plain, ref.u, ref.v, dev), device_quantities(packed, ref.u, ref.v, dev)
    for k in QUANTITIES:
        print(f"packed vs plain periodic {k}: max difference {np.abs(a[k] - b[k]).max():.3e}")
        assert np.array_equal(a[k], b[k])
        check(f"packed periodic {k}", b[k], getattr(ref, k), getattr(ref, k + "_bound"))
    plain.close()
    packed.close()


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    close_problems()
    for P in _SOLVE_PROBLEMS.values():
        P.close()
        P.close()
    _SOLVE_PROBLEMS.clear()
