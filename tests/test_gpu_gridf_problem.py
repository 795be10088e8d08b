"""Compiled grid problems with fields on the device (csrc/nk_grid.hip, nk_problem_create_grid_fields): the generated residual,
dual-number JVP and Jacobian-fill kernels of sources that read read-only data on the grid, against the NumPy restatement
(tests/grid_core.py, tests/gridf_reference.py), entry by entry within the restatement's own bound

    |device − float64 restatement| <= 16 × |float64 − long double| + 4 eps × Σ|terms of the entry|

then the contract of the fields (zero at creation, set / get, a changed field against a cached linearisation, argument errors,
declared and unread fields) and implicit time stepping through the public interface against a dense NumPy Newton on the
restatement. Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import grid_core as GC
import grid_reference as G1
import gridf_reference as R
from grid_device import (assert_parity, check, close_problems, create, device_quantities, problem, set_fields, to_device,
                         to_numpy)

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ parity with the restatement
_CASES = [(name, shape) for name in sorted(R.PROBLEMS) for shape in R.sizes(R.PROBLEMS[name])]


@pytest.mark.parametrize("name,shape", _CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in _CASES])
def test_parity_with_the_restatement(nls, dev, name, shape):
    """2-D radius 1 — 37 × 29: five workgroups, the last ragged; 3 × 3: every node on the boundary, every periodic row wraps, every
    Dirichlet field read but the centre's is the clamped one; 300 × 5. Radius 2 — 5 × 5 and 37 × 29: at i = nx − 2 the field
    read at +2 is the node's own value. 3-D — 7 × 6 × 5, 3 × 3 × 3, 37 × 29 × 3. Residual, JVP, fill and the transposed product,
    then the consistency of fill and JVP: the filled matrix times v against the dual JVP within the sum of the two bounds.
    Only bratu_f / bratu_f4 have an elementary function: with -ffp-contract=off the device's +, −, × are the restatement's in
    the restatement's order. What the MI355X showed is recorded at EXACT below and asserted."""
    P = problem(nls, R.PROBLEMS[name], shape)
    assert P.nfields == R.PROBLEMS[name].nfields and P.nn == int(np.prod(shape))
    assert_parity(nls, dev, R.PROBLEMS[name], shape, exact=name in EXACT)


# The problems whose five quantities agreed BIT FOR BIT with the restatement at all their shapes on the MI355X: every problem
# without an elementary function (100 of 100 comparisons, every entry) — the field loads, the clamp and the wrap feed the same
# +, −, × in the restatement's order. bratu_f and bratu_f4 differ from NumPy in the last bits of exp at a few entries
# (22458 and 22470 of their 22484 entries equal, max error 8.9e-16 against bounds of 5.7e-16 … 3.2e-14) and are held to the rule.
EXACT = ("react2", "vardiff", "vardiff_r", "vardiff3", "vardiff_box_dirichlet", "vardiff_box_periodic", "vardiff_s2")


# ------------------------------------------------------------------------------------------------ the fields' contract
def test_fields_are_zero_at_creation_and_set_field_stores_what_it_is_given(nls, dev):
    case, shape = R.PROBLEMS["vardiff"], (37, 29)
    P = create(nls, case, shape)
    zero, ref = GC.reference(case, shape, zero_fields=True), GC.reference(case, shape)
    for k in range(3):
        assert np.array_equal(to_numpy(P.field(k)), np.zeros(37 * 29))
    check("residual before any set_field", to_numpy(P.residual(to_device(ref.u, dev))), zero.f, zero.f_bound)
    assert float(np.max(np.abs(zero.f - ref.f))) > 1e6 * float(ref.f_bound.max())   # (the fields matter to this residual)
    P.set_field(0, ref.fields[0])                      # a host array
    P.set_field(1, to_device(ref.fields[1], dev))      # a device tensor
    P.set_field(2, list(ref.fields[2]))                # anything NumPy makes a float64 vector of
    for k in range(3):
        got = P.field(k)
        assert got.is_cuda and np.array_equal(to_numpy(got), ref.fields[k])
    got = P.field(1)
    got.zero_()                                        # a copy: the problem's field is its own
    assert np.array_equal(to_numpy(P.field(1)), ref.fields[1])
    check("residual after set_field", to_numpy(P.residual(to_device(ref.u, dev))), ref.f, ref.f_bound)
    P.close()
    P.close()


def _mixed_reference(case, shape, k, ref, other):
    """the case's reference with field k taken from `other`"""
    fields = np.array(ref.fields)
    fields[k] = other.fields[k]
    return GC.Reference(case, shape, ref.u, ref.v, fields), fields


def test_a_changed_field_is_not_met_by_a_stale_jacobian(nls, dev):
    """fill J at u, set_field(1, other), fill again at the SAME u buffer: the second matrix is the restatement's for the new
    coefficient, not the first matrix; the same for Jᵀv, which goes through the problem's cached linearisation"""
    case, shape = R.PROBLEMS["vardiff"], (37, 29)
    P, ref = problem(nls, case, shape), GC.reference(case, shape)
    new, fields = _mixed_reference(case, shape, 1, ref, GC.reference(case, shape, shift=1.0))
    u, v, J = to_device(ref.u, dev), to_device(ref.v, dev), P.jac_csr()
    try:
        P.jac_values(u, J)
        first = np.array(J.values())
        check("fill with the seeded coefficient", first, ref.vals, ref.vals_bound)
        check("Jᵀv with the seeded coefficient", to_numpy(P.vjp(v, u)), ref.jtv, ref.jtv_bound)
        P.set_field(1, fields[1])
        P.jac_values(u, J)
        second = np.array(J.values())
        check("fill after set_field, same u buffer", second, new.vals, new.vals_bound)
        check("Jᵀv after set_field, same u buffer", to_numpy(P.vjp(v, u)), new.jtv, new.jtv_bound)
        check("J·v after set_field", to_numpy(P.jvp(v, u)), new.jv, new.jv_bound)
        assert float(np.max(np.abs(second - first))) > 1e6 * float(new.vals_bound.max())
    finally:
        P.set_field(1, ref.fields[1])


def test_a_changed_field_reaches_the_solver_cache_step(nls, dev):
    """init at u and one Newton step on the concrete Jacobian; set_field(1, other), reinit_ at the same u, one step. vardiff is
    linear in u, so a Newton step with the Jacobian OF THE NEW FIELD lands on the root up to the linear solve's tolerance:
    GMRES stops at ‖r‖₂ <= 1e-10·‖F‖₂, hence ‖F_new(u₁)‖∞ <= 1e-10·√n·‖F_new(u)‖∞ (n = 72: 8.5e-10) plus rounding; 1e-8 is
    asserted. A step with the Jacobian kept from the old field leaves (I − J_new J_old⁻¹)F_new(u): computed here in NumPy, it
    is more than a million times that."""
    prob, shape = R.PROBLEMS["vardiff"], (9, 8)
    P, ref = problem(nls, prob, shape), GC.reference(prob, shape)
    new, fields = _mixed_reference(prob, shape, 1, ref, GC.reference(prob, shape, shift=1.0))
    alg = nls.NewtonRaphson(linsolve=nls.KrylovJL_GMRES(reltol=1e-10), concrete_jac=True)
    try:
        cache = nls.init(nls.NonlinearProblem(P, to_device(ref.u, dev)), alg, abstol=1e-13)
        nls.step_(cache)
        f_old = GC.evaluate(prob, shape, to_numpy(cache.u), ref.v, ref.fields).f
        print(f"old field: |F(u)| {np.abs(ref.f).max():.3e} -> |F(u1)| {np.abs(f_old).max():.3e}")
        assert np.abs(f_old).max() <= 1e-8 * np.abs(ref.f).max()
        P.set_field(1, fields[1])
        nls.reinit_(cache, u0=to_device(ref.u, dev))
        check("fu after set_field and reinit_", to_numpy(cache.fu), new.f, new.f_bound)
        nls.step_(cache)
        f_new = GC.evaluate(prob, shape, to_numpy(cache.u), ref.v, fields).f
        J_old, _f = GC.dense_jacobian(prob, shape, ref.u, ref.fields)
        stale = GC.evaluate(prob, shape, ref.u - np.linalg.solve(J_old, new.f), ref.v, fields).f
        print(f"new field: |F(u)| {np.abs(new.f).max():.3e} -> |F(u1)| {np.abs(f_new).max():.3e}; a stale Jacobian would leave "
              f"{np.abs(stale).max():.3e}")
        assert np.abs(stale).max() > 1e6 * 1e-8 * np.abs(new.f).max()
        assert np.abs(f_new).max() <= 1e-8 * np.abs(new.f).max()
        cache.close()
    finally:
        P.set_field(1, ref.fields[1])


def test_bad_arguments_name_the_value(nls, dev):
    from nonlinearsolve_jl_amd import _lib as L
    P = problem(nls, R.PROBLEMS["vardiff"], (9, 8))
    good = np.ones(72)
    with pytest.raises(nls.NKError, match="k = 3 outside 0..2"):
        P.set_field(3, good)
    with pytest.raises(nls.NKError, match="k = -1 outside 0..2"):
        P.field(-1)
    with pytest.raises(ValueError, match="expected 72 elements.*got 71"):
        P.set_field(0, np.ones(71))
    with pytest.raises(ValueError, match="expected 72 elements.*got 144"):
        P.set_field(0, to_device(np.ones(144), dev))
    assert np.array_equal(to_numpy(P.field(0)), GC.seeded_fields(3, (9, 8))[0])     # nothing was stored by the refused calls
    Q = nls.CompiledGridProblem(G1.BRATU_SRC, 9, 8, params=[1.0, 0.04])       # a compiled grid problem without fields
    assert Q.nfields == 0
    with pytest.raises(nls.NKError, match="nfields = 0"):
        Q.set_field(0, good)
    with pytest.raises(nls.NKError, match="nfields = 0"):
        Q.field(0)
    Q.close()
    B = nls.Bratu2D(8)                                                        # not a compiled grid problem at all
    buf = (C.c_double * 64)()
    assert L.lib().nk_problem_set_field(B._h, 0, buf, 0) == -1
    assert "not a compiled grid problem" in L.lib().nk_last_error().decode()
    B.close()
    src = R.PROBLEMS["bratu_f"].source
    with pytest.raises(nls.NKError, match="nfields = 5"):
        nls.CompiledGridProblem(src, 9, 8, params=[1.0, 0.04], fields=5)
    with pytest.raises(nls.NKError, match="nfields = -2"):
        nls.CompiledGridProblem(src, 9, 8, params=[1.0, 0.04], fields=-2)


def test_declared_fields_that_are_not_read_change_nothing(nls, dev):
    """the bratu_f source compiled with four fields declared, three of them holding other data: the five quantities of the
    one-field problem, bit for bit (the same instructions on the same data)"""
    shape = (37, 29)
    ref = GC.reference(R.PROBLEMS["bratu_f"], shape)
    P1, P4 = problem(nls, R.PROBLEMS["bratu_f"], shape), problem(nls, R.PROBLEMS["bratu_f4"], shape)
    assert np.array_equal(to_numpy(P4.field(0)), to_numpy(P1.field(0))) and not np.array_equal(to_numpy(P4.field(1)), to_numpy(P1.field(0)))
    g1, g4 = device_quantities(P1, ref.u, ref.v, dev), device_quantities(P4, ref.u, ref.v, dev)
    for k in ("f", "jv", "vals", "jtv", "spmv"):
        print(f"bratu_f4 vs bratu_f {k}: max difference {np.abs(g4[k] - g1[k]).max():.3e}")
        assert np.array_equal(g4[k], g1[k])


# ------------------------------------------------------------------------------------------------ implicit time stepping
def _algorithms(nls):
    """Left preconditioning makes GMRES measure M⁻¹r. The diagonal of these Jacobians is p0 + p1·Σw ≈ 10 (≈ 18 in 3-D), so the
    nonlinear abstol of 1e-10, forwarded as the linear one, would stop the linear solve at a true residual near 1e-9 and the
    Newton iteration could not get below it (it ends as Stalled at ‖F‖∞ = 3e-10, as the reference's left-preconditioned Krylov
    solve would); the preconditioned solves are therefore given a linear abstol of their own, two orders tighter."""
    G = nls.KrylovJL_GMRES
    return {
        "newton_matfree": nls.NewtonRaphson(linsolve=G()),
        "newton_jacobi": nls.NewtonRaphson(linsolve=G(abstol=1e-12, precs=nls.ObjectPrecs("jacobi", "left")), concrete_jac=True),
        "newton_ilu0": nls.NewtonRaphson(linsolve=G(abstol=1e-12, precs=nls.ObjectPrecs("ilu0", "left")), concrete_jac=True),
        "trust_region": nls.TrustRegion(linsolve=G()),
    }


def _dense_newton(prob, shape, u0, fields):
    """u_ref with ‖F(u_ref)‖∞ <= 1e-12 by a dense NumPy Newton on the restatement, ‖F(u_ref)‖∞ and ‖J(u_ref)⁻¹‖∞"""
    u = np.array(u0)
    for _it in range(30):
        J, f = GC.dense_jacobian(prob, shape, u, fields)
        if np.abs(f).max() <= 1e-12:
            break
        u = u - np.linalg.solve(J, f)
    assert np.abs(f).max() <= 1e-12
    return u, float(np.abs(f).max()), float(np.linalg.norm(np.linalg.inv(J), np.inf))


def _time_steps(nls, dev, name, shape, algname, nsteps):
    """nsteps of implicit Euler, F(u) = p0·(u − u_old) + …, with the idiom of the docstring: set_field(0, cache.u), reinit_,
    solve_. After every step |u_dev − u_ref|∞ <= 2·‖J(u_ref)⁻¹‖∞·(‖F(u_dev)‖∞ + ‖F(u_ref)‖∞), u_ref by a dense NumPy Newton on
    the restatement WITH THE FIELDS THE DEVICE HOLDS (the previous level is the device's own, read back with field(0)): both
    residuals by the restatement, the factor 2 for the second-order term, as tests/test_gpu_grid3_problem.py has it."""
    prob, abstol = R.PROBLEMS[name], 1e-10
    P = problem(nls, prob, shape)
    fields = GC.seeded_fields(prob.nfields, shape)
    set_fields(P, fields)
    u_init = 0.5 * fields[0]
    cache = nls.init(nls.NonlinearProblem(P, to_device(u_init, dev)), _algorithms(nls)[algname], abstol=abstol, maxiters=60)
    moved = 0.0
    for step in range(nsteps):
        P.set_field(0, cache.u)
        nls.reinit_(cache, u0=cache.u)
        sol = nls.solve_(cache)
        held = np.stack([to_numpy(P.field(k)) for k in range(prob.nfields)])
        assert np.array_equal(held[1:], fields[1:])
        u_dev = to_numpy(cache.u)
        u_ref, f_ref, jinv = _dense_newton(prob, shape, held[0], held)
        f_dev = float(np.abs(GC.evaluate(prob, shape, u_dev, u_dev, held).f).max())
        err, bound = float(np.abs(u_dev - u_ref).max()), 2.0 * jinv * (f_dev + f_ref)
        moved = max(moved, float(np.abs(u_dev - held[0]).max()))
        print(f"{name} {algname} step {step}: {sol.retcode} {sol.stats}; |u_dev - u_ref| {err:.3e}, bound {bound:.3e} "
              f"(|J^-1| {jinv:.3e}, |F(u_dev)| {f_dev:.3e}, |F(u_ref)| {f_ref:.3e}); |u - u_old| {np.abs(u_dev - held[0]).max():.3e}")
        assert sol.retcode == "Success"
        assert err <= bound
        assert f_dev <= abstol + float(GC.Reference(prob, shape, u_dev, u_dev, held).f_bound.max())
    assert moved > 1e-3   # (the levels differ: a step that kept the old level would show)
    cache.close()
    set_fields(P, fields)


@pytest.mark.parametrize("algname", ["newton_matfree", "newton_jacobi", "newton_ilu0", "trust_region"])
def test_three_implicit_euler_steps_like_a_dense_newton(nls, dev, algname):
    """vardiff with the reaction term p2·u³ at 9 × 8 (72 unknowns)"""
    _time_steps(nls, dev, "vardiff_r", (9, 8), algname, 3)


@pytest.mark.parametrize("algname", ["newton_matfree", "newton_jacobi", "newton_ilu0", "trust_region"])
def test_one_implicit_euler_step_in_three_dimensions(nls, dev, algname):
    """vardiff3 at 6 × 5 × 5 (150 unknowns)"""
    _time_steps(nls, dev, "vardiff3", (6, 5, 5), algname, 1)


def test_close_module_problems(nls):
    """(last in the file) the problems the module shared are freed; a double close is harmless"""
    close_problems()
