"""Restarted GMRES on the device (csrc/nk_gmres.hip, csrc/nk_sstep.hip) against the long-double GMRES of
tests/gmres_reference.py: every orthogonalisation, restart lengths up to the limit of 63, nonsymmetric operators at odd sizes
and past the column-padding threshold, tolerance and maxiters stops, warm starts, exact breakdowns, both preconditioner sides,
the shifted and the normal-form operator, host callbacks, the unfused Chebyshev path, object reuse and degenerate inputs. The
cases, bounds and assertions are gmres_reference's; tests/test_gmres_reference.py shows without a GPU that they accept the
oracle's float64 formulations and reject twelve planted defects."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmres_reference as GR  # noqa: E402
from oracle import reference_restatement as R  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not GR.LONGDOUBLE_OK, reason="np.longdouble has fewer than 64 significand bits")]

_CSR = {}


@pytest.fixture(autouse=True)
def _no_test_after_a_device_fault():
    """a device fault ends the session: nothing more is started on a device that has faulted"""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except Exception as e:  # pragma: no cover
        pytest.exit(f"the device reported a fault after this test: {e}", returncode=3)


def dev_csr(nls, case):
    if case.name not in _CSR:
        _CSR[case.name] = nls.CSRMatrix.from_arrays(case.rowptr, case.colind, case.vals)
    return _CSR[case.name]


def torch_csr(case, dev):
    import torch
    return torch.sparse_csr_tensor(torch.tensor(case.rowptr, dtype=torch.int64), torch.tensor(case.colind, dtype=torch.int64),
                                   torch.tensor(case.vals), size=(case.n, case.n), device=dev)


def solver(nls, n, m, form):
    return nls.GMRES(n, restart=m, **GR.form_args(form))


def lib():
    from nonlinearsolve_jl_amd import _lib as L
    return L


def judge(x, info, ref, tx, tr, **kw):
    print("deviation (x, norms):", GR.deviation(x, info, ref), "bounds:", (tx, tr), info)
    GR.check_iterate(x, info, ref, tx, tr, **kw)


def judge_spec(x, info, s, ref, name):
    tx, tr = GR.group_bounds(name)
    print("deviation (x, norms):", GR.deviation(x, info, ref), "bounds:", (tx, tr), info)
    GR.check_spec(x, info, s, ref, tx, tr)


def block_of(G, form):
    return G.sstep_state()[0] if form.startswith("sstep") else 0


# ------------------------------------------------------------------------------------------------------------- a. fixed work
@pytest.mark.parametrize("m", GR.RESTARTS)
@pytest.mark.parametrize("pe", GR.PES)
@pytest.mark.parametrize("n", GR.FIXED_N)
@pytest.mark.parametrize("form", GR.FORMS)
def test_fixed_work(nls, form, n, pe, m):
    case = GR.convdiff_n(n, pe)
    op = GR.Operator(case)
    G = solver(nls, n, m, form).set_operator(dev_csr(nls, case))
    tx, tr = GR.fixed_bounds(n, pe, m)
    for k in GR.fixed_counts(n, pe, m):
        x, info = G.solve(case.b, fixed_iters=k)
        assert info["iters"] == k and not info["failed"]
        judge(x, info, GR.fixed_reference(n, pe, m, k), tx, tr, op=op, b=case.b)
    G.close()


@pytest.mark.parametrize("m", [64, 200])
def test_restart_above_the_limit_is_rejected(nls, m):
    with pytest.raises(lib().NKError, match="63"):
        nls.GMRES(63, restart=m, ortho="mgs")


@pytest.mark.parametrize("m", [0, -5])
def test_nonpositive_restart_means_30(nls, m):
    case = GR.convdiff_n(99, 2.0)
    x, info = nls.GMRES(99, restart=m, ortho="mgs").set_operator(dev_csr(nls, case)).solve(case.b, fixed_iters=31)
    assert (info["iters"], info["restarts"]) == (31, 1)
    judge(x, info, GR.fixed_reference(99, 2.0, 30, 31), *GR.fixed_bounds(99, 2.0, 30))


# ------------------------------------------------------------------------------------------------------------- b. tolerance stops
@pytest.mark.parametrize("m", GR.STOP_M)
@pytest.mark.parametrize("pe", GR.PES)
@pytest.mark.parametrize("n", GR.STOP_N)
@pytest.mark.parametrize("form", GR.FORMS)
def test_tolerance_stops(nls, form, n, pe, m):
    case = GR.convdiff_n(n, pe)
    op = GR.Operator(case)
    G = solver(nls, n, m, form).set_operator(dev_csr(nls, case))
    for i, stop in enumerate(GR.STOPS):
        tx, tr = GR.group_bounds(GR.stop_name(n, pe, m, i))
        ref, atol, rtol = GR.stop_reference(n, pe, m, stop)
        x, info = G.solve(case.b, abstol=atol, reltol=rtol, maxiters=GR.STOP_ITMAX)
        print(stop, info)
        exact = not form.startswith("sstep")
        GR.check_counts(info, ref, exact=exact, block=block_of(G, form), m=m)
        if info["iters"] == ref.iters:
            judge(x, info, ref, tx, tr, op=op, b=case.b)
        else:   # whole blocks: the iterate of the count the device stopped at
            r2 = GR.gmres(op, case.b, restart=m, fixed_iters=info["iters"])
            judge(x, info, r2, tx, tr, op=op, b=case.b)
    G.close()


@pytest.mark.parametrize("m", GR.STOP_M)
@pytest.mark.parametrize("form", GR.FORMS)
def test_maxiters_stop(nls, form, m):
    n, pe = 99, 2.0
    case = GR.convdiff_n(n, pe)
    G = solver(nls, n, m, form).set_operator(dev_csr(nls, case))
    tx, tr = GR.fixed_bounds(n, pe, m)
    cap = GR.supported_steps(n, pe, m)
    for it in sorted({1, m, m + 1, min(2 * m + 3, cap)}):
        x, info = G.solve(case.b, abstol=0.0, reltol=1e-14, maxiters=it)
        assert (info["iters"], info["converged"], info["failed"]) == (it, False, False), info
        judge(x, info, GR.fixed_reference(n, pe, m, it), tx, tr, op=GR.Operator(case), b=case.b)
    G.close()


# ------------------------------------------------------------------------------------------------------------- c. warm start
@pytest.mark.parametrize("kind", ["csr", "callable"])
@pytest.mark.parametrize("n", [63, 65, 99])
@pytest.mark.parametrize("form", GR.FORMS)
def test_warm_start(nls, dev, form, n, kind):
    import torch
    specs = GR.group_specs()
    case = specs[f"warm-{n}-k17"].case
    G = solver(nls, n, 7, form)
    if kind == "csr":
        G.set_operator(dev_csr(nls, case))
    else:
        Jd = torch_csr(case, dev)
        G.set_operator(lambda z: Jd @ z)
    for name in (f"warm-{n}-k17", f"warm-{n}-stop"):
        s = specs[name]
        ref = GR.solve_spec(s)
        x, info = G.solve(s.b, x0=s.x0, abstol=s.atol, reltol=s.rtol, maxiters=s.itmax, fixed_iters=s.k)
        bnorm = float(np.linalg.norm(s.b))
        assert abs(info["rnorm0"] - bnorm) > 0.1 * bnorm, "rnorm0 is ‖b − A x0‖, not ‖b‖"
        GR.check_counts(info, ref, exact=not form.startswith("sstep") or s.k > 0, block=block_of(G, form), m=7)
        if info["iters"] != ref.iters:
            ref = GR.solve_spec(GR.spec(case, 7, k=info["iters"], x0=s.x0))
        judge_spec(x, info, s, ref, name)
    # … and from the iterate a 5-step solve returned
    x5, _ = G.solve(case.b, fixed_iters=5)
    s = GR.spec(case, 7, k=17, x0=np.array(x5))
    x, info = G.solve(case.b, x0=x5, fixed_iters=17)
    assert info["iters"] == 17
    judge_spec(x, info, s, GR.solve_spec(s), f"warm5-{n}")
    G.close()


def test_warm_start_with_right_preconditioner_is_refused(nls):
    case = GR.convdiff_n(63, 0.5)
    A = dev_csr(nls, case)
    G = nls.GMRES(63, restart=7, ortho="mgs").set_operator(A)
    G.set_preconditioner(nls.JacobiPreconditioner(A), side="right")
    with pytest.raises(lib().NKError, match="not supported"):
        G.solve(case.b, x0=np.ones(63), fixed_iters=3)
    s = GR.group_specs()["prec-right-63-k17"]
    x, info = G.solve(case.b, fixed_iters=17)
    judge_spec(x, info, s, GR.solve_spec(s), "prec-right-63-k17")


# ------------------------------------------------------------------------------------------------------------- d. exact cases
@pytest.mark.parametrize("n", [7, 65])
@pytest.mark.parametrize("form", GR.FORMS)
def test_scaled_identity_breaks_down_at_step_one(nls, form, n):
    case = GR.scaled_identity(n)
    x, info = solver(nls, n, 30, form).set_operator(dev_csr(nls, case)).solve(case.b)
    assert (info["iters"], info["converged"], info["failed"], info["rnorm"]) == (1, True, False, 0.0), info
    GR.check_exact(x, case.b / 2)


@pytest.mark.parametrize("over", [0, 3])
@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("form", GR.COLUMN_FORMS)
def test_cyclic_breaks_down_at_step_n(nls, form, n, over):
    case = GR.cyclic(n)
    x, info = solver(nls, n, n + over, form).set_operator(dev_csr(nls, case)).solve(case.b)
    assert (info["iters"], info["restarts"], info["converged"], info["rnorm"]) == (n, 0, True, 0.0), info
    e = np.zeros(n)
    e[n - 1] = 4.0
    GR.check_exact(x, e)


@pytest.mark.parametrize("form", GR.COLUMN_FORMS)
def test_cyclic_stagnates(nls, form):
    case = GR.cyclic(5)
    x, info = solver(nls, 5, 3, form).set_operator(dev_csr(nls, case)).solve(case.b, maxiters=12)
    assert (info["iters"], info["restarts"], info["converged"], info["failed"], info["rnorm"]) == (12, 3, False, False, 4.0), info
    GR.check_exact(x, np.zeros(5))
    assert not np.any(np.signbit(x)), "x is all +0.0"


@pytest.mark.parametrize("over", [0, 3])
@pytest.mark.parametrize("form", ["sstep0", "sstep4"])
@pytest.mark.parametrize("n", [5, 33])
def test_cyclic_sstep_falls_back(nls, form, n, over):
    """the s-step form meets a rank-deficient block on the permutation and finishes the solve with delayed CGS2"""
    case = GR.cyclic(n)
    G = solver(nls, n, n + over, form).set_operator(dev_csr(nls, case))
    before = G.sstep_state()[2]
    x, info = G.solve(case.b)
    assert (info["converged"], info["failed"], info["rnorm"]) == (True, False, 0.0), info
    e = np.zeros(n)
    e[n - 1] = 4.0
    GR.check_exact(x, e)
    assert G.sstep_state()[2] >= before
    # the next solve on the same object: a convdiff operator of the same size (3 steps: one cycle whatever the restart)
    s = GR.group_specs()[f"line-{n}"]
    G.set_operator(dev_csr(nls, s.case))
    x, info = G.solve(s.b, fixed_iters=s.k)
    assert info["iters"] == s.k
    judge_spec(x, info, s, GR.solve_spec(s), f"line-{n}")


@pytest.mark.parametrize("form", ["sstep0", "sstep4"])
def test_cyclic_sstep_stagnates(nls, form):
    case = GR.cyclic(5)
    G = solver(nls, 5, 3, form).set_operator(dev_csr(nls, case))
    before = G.sstep_state()[2]
    x, info = G.solve(case.b, maxiters=12)
    assert (info["converged"], info["failed"], info["rnorm"]) == (False, False, 4.0), info
    GR.check_exact(x, np.zeros(5))
    assert not np.any(np.signbit(x)), "x is all +0.0"
    assert G.sstep_state()[2] >= before


# ------------------------------------------------------------------------------------------------------------- e. preconditioner sides
PREC_FORMS = ("mgs", "dcgs2", "dcgs2_1r", "sstep4")


@pytest.mark.parametrize("how", ["callable", "object"])
@pytest.mark.parametrize("side", ["left", "right", "both"])
@pytest.mark.parametrize("n", [63, 99])
@pytest.mark.parametrize("form", PREC_FORMS)
def test_preconditioner_sides(nls, dev, form, n, side, how):
    import torch
    specs = GR.group_specs()
    case = specs[f"prec-{side}-{n}-k17"].case
    A = dev_csr(nls, case)
    G = solver(nls, n, 7, form).set_operator(A)
    dg = torch.tensor(GR.diag_of(case), device=dev)
    P = nls.JacobiPreconditioner(A) if how == "object" else None
    if side != "right":
        G.set_left_preconditioner(P if P is not None else (lambda z: z / dg))
    if side != "left":
        if P is not None:
            G.set_preconditioner(P, side="right")
        else:
            G.set_right_preconditioner(lambda z: z / dg)
    for name in (f"prec-{side}-{n}-k17", f"prec-{side}-{n}-stop"):
        s = specs[name]
        ref = GR.solve_spec(s)
        x, info = G.solve(s.b, abstol=s.atol, reltol=s.rtol, maxiters=s.itmax, fixed_iters=s.k)
        GR.check_counts(info, ref, exact=not form.startswith("sstep") or s.k > 0, block=block_of(G, form), m=7)
        if info["iters"] != ref.iters:
            ref = GR.solve_spec(GR.spec(case, 7, k=info["iters"], left=s.left, right=s.right))
        judge_spec(x, info, s, ref, name)   # with Pl the reported norms are the preconditioned ones: check_spec forms ‖Pl⁻¹(b − A x)‖
    # removing the preconditioners restores the unpreconditioned iterates bit for bit
    G.set_left_preconditioner(None)
    G.set_right_preconditioner(None)
    x, info = G.solve(case.b, fixed_iters=17)
    x2, info2 = solver(nls, n, 7, form).set_operator(A).solve(case.b, fixed_iters=17)
    assert np.array_equal(x, x2) and info == info2


# ------------------------------------------------------------------------------------------------------------- f. shift, normal form
SHIFT_FORMS = ("mgs", "dcgs2", "sstep0")


def _dev_vec(v, dev):
    import torch
    return torch.tensor(np.asarray(v, dtype=np.float64), device=dev)


def _plain(G, s_b, k=17):
    return G.solve(s_b, fixed_iters=k)


@pytest.mark.parametrize("kind", ["csr", "callable"])
@pytest.mark.parametrize("n", [63, 65, 4097])
@pytest.mark.parametrize("form", SHIFT_FORMS)
def test_shifted_operator(nls, dev, form, n, kind):
    L = lib()
    specs = GR.group_specs()
    case = specs[f"shift0.75-{n}"].case
    G = solver(nls, n, 7, form)
    if kind == "csr":
        G.set_operator(dev_csr(nls, case))
    else:
        Jd = torch_csr(case, dev)
        G.set_operator(lambda z: Jd @ z)
    x_plain, info_plain = _plain(G, case.b)
    w = _dev_vec(specs[f"shift0.75-w-{n}"].weights, dev)     # alive for the life of the solver
    for sigma in (0.75, -0.25):
        for weighted in (False, True):
            name = f"shift{sigma}-w-{n}" if weighted else f"shift{sigma}-{n}"
            s = specs[name]
            L.check(L.lib().nk_gmres_set_shift(G._h, sigma))
            L.check(L.lib().nk_gmres_set_shift_weights(G._h, C.c_void_p(w.data_ptr()) if weighted else None))
            x, info = G.solve(s.b, fixed_iters=s.k)
            assert info["iters"] == s.k
            judge_spec(x, info, s, GR.solve_spec(s), name)
    L.check(L.lib().nk_gmres_set_shift(G._h, 0.0))
    L.check(L.lib().nk_gmres_set_shift_weights(G._h, None))
    x, info = _plain(G, case.b)
    assert np.array_equal(x, x_plain) and info == info_plain
    G.close()


def _normal_form_solves(G, L, specs, names, dev, b_plain):
    x_plain, info_plain = _plain(G, b_plain)
    keep = []
    for name in names:
        s = specs[name]
        L.check(L.lib().nk_gmres_set_normal_form(G._h, 1))
        if s.damping is not None:
            d = _dev_vec(s.damping[0], dev)
            keep.append(d)
            L.check(L.lib().nk_gmres_set_normal_form_damping(G._h, C.c_void_p(d.data_ptr()), float(s.damping[1])))
        else:
            L.check(L.lib().nk_gmres_set_normal_form_damping(G._h, None, 0.0))
        bn = np.asarray(GR.spec_parts(s)[1], dtype=np.float64)      # Aᵀ b
        x, info = G.solve(bn, fixed_iters=s.k)
        assert info["iters"] == s.k
        judge_spec(x, info, s, GR.solve_spec(s), name)
    L.check(L.lib().nk_gmres_set_normal_form_damping(G._h, None, 0.0))
    L.check(L.lib().nk_gmres_set_normal_form(G._h, 0))
    x, info = _plain(G, b_plain)
    assert np.array_equal(x, x_plain) and info == info_plain


@pytest.mark.parametrize("n", [63, 65, 4097])
@pytest.mark.parametrize("form", SHIFT_FORMS)
def test_normal_form_csr(nls, dev, form, n):
    specs = GR.group_specs()
    case = specs[f"normal-{n}"].case
    G = solver(nls, n, 7, form).set_operator(dev_csr(nls, case))
    _normal_form_solves(G, lib(), specs, [f"normal-{n}", f"normal-damped0.0-{n}", f"normal-damped0.5-{n}"], dev, case.b)
    G.close()


def _brusselator_operator(nls, case):
    prob = nls.NonlinearProblem(nls.Brusselator2D(case.N))
    return nls.StatefulJacobianOperator(nls.JacobianOperator(prob), case.u.copy())


@pytest.mark.parametrize("N", [4, 5])
@pytest.mark.parametrize("form", SHIFT_FORMS)
def test_normal_form_matrix_free(nls, dev, form, N):
    specs = GR.brusselator_specs(R)
    n = 2 * N * N
    case = specs[f"brus-normal-{n}"].case
    G = solver(nls, n, 7, form).set_operator(_brusselator_operator(nls, case))
    _normal_form_solves(G, lib(), specs, [f"brus-normal-{n}", f"brus-normal-damped0.0-{n}", f"brus-normal-damped0.5-{n}"], dev,
                        case.b)
    G.close()


# ------------------------------------------------------------------------------------------------------------- g. host callbacks
def _host_matvec(L, n, fn, calls=None, fail_at=None):
    def cb(user, px, py, stream):
        if calls is not None:
            calls.append(1)
            if fail_at is not None and len(calls) == fail_at:
                return 1
        x = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_double)), shape=(n,))
        y = np.ctypeslib.as_array(C.cast(py, C.POINTER(C.c_double)), shape=(n,))
        y[:] = fn(x)
        return 0
    return L.MATVEC_FN(cb)


@pytest.mark.parametrize("n", [3, 63, 65])
@pytest.mark.parametrize("form", ["mgs", "dcgs2", "sstep4"])
def test_host_callbacks(nls, dev, form, n):
    import torch
    L = lib()
    case = GR.convdiff_n(n, 0.5)
    A = GR.to_scipy(case)
    dg = GR.diag_of(case)
    m, k = (7, 17) if n > 3 else (3, 2)
    keep = [_host_matvec(L, n, lambda z: A @ z), _host_matvec(L, n, lambda z: z / dg)]
    Jd, dd = torch_csr(case, dev), torch.tensor(dg, device=dev)
    for sides in GR.HOST_SIDES:
        name = f"host-{n}-{'+'.join(sides) or 'none'}"
        s = GR.group_specs()[name]
        assert (s.m, s.k) == (m, k)
        ref = GR.solve_spec(s)
        G = solver(nls, n, m, form)
        G._keep += keep
        L.check(L.lib().nk_gmres_set_operator_fn_host(G._h, keep[0], None))
        if "right" in sides:
            L.check(L.lib().nk_gmres_set_right_preconditioner_host(G._h, keep[1], None))
        if "left" in sides:
            L.check(L.lib().nk_gmres_set_left_preconditioner_host(G._h, keep[1], None))
        x, info = G.solve(case.b, fixed_iters=k)
        assert info["iters"] == k
        judge_spec(x, info, s, ref, name)
        # the same operator and preconditioners as device callables
        G2 = solver(nls, n, m, form).set_operator(lambda z: Jd @ z)
        if "right" in sides:
            G2.set_right_preconditioner(lambda z: z / dd)
        if "left" in sides:
            G2.set_left_preconditioner(lambda z: z / dd)
        x2, info2 = G2.solve(case.b, fixed_iters=k)
        judge_spec(x2, info2, s, ref, name)
        G.close()
        G2.close()


def test_failing_host_callback_is_an_error_and_the_object_lives(nls):
    L = lib()
    n = 63
    case = GR.convdiff_n(n, 0.5)
    A = GR.to_scipy(case)
    calls = []
    bad = _host_matvec(L, n, lambda z: A @ z, calls, fail_at=3)
    G = nls.GMRES(n, restart=7, ortho="mgs")
    G._keep.append(bad)
    L.check(L.lib().nk_gmres_set_operator_fn_host(G._h, bad, None))
    with pytest.raises(L.NKError, match="callback"):
        G.solve(case.b, fixed_iters=17)
    x, info = G.solve(case.b, fixed_iters=17)      # the counter is past 3: every call succeeds now
    s = GR.group_specs()["plain-63"]
    judge_spec(x, info, s, GR.solve_spec(s), "plain-63")


# ------------------------------------------------------------------------------------------------------------- h. Chebyshev
@pytest.mark.parametrize("deg", [1, 2, 5])
@pytest.mark.parametrize("n", [63, 65])
@pytest.mark.parametrize("form", ["mgs", "dcgs2"])
def test_chebyshev_unfused_and_fused(nls, dev, form, n, deg):
    """callable and shifted CSR operators take k_cheb_step (double2 body, odd-n tail); the CSR operator with no shift takes the
    update fused into the SpMV: all against the long-double transcription of the oracle's chebyshev_preconditioner"""
    L = lib()
    specs = GR.group_specs()
    name = f"cheb{deg}-{n}"
    s = specs[name]
    case, ref = s.case, GR.solve_spec(s)
    Jd = torch_csr(case, dev)
    for kind in ("callable", "csr"):
        G = solver(nls, n, 7, form)
        G.set_operator(dev_csr(nls, case) if kind == "csr" else (lambda z: Jd @ z))
        G.set_chebyshev_preconditioner(deg, s.cheb[1], s.cheb[2])
        x, info = G.solve(s.b, fixed_iters=s.k)
        assert info["iters"] == s.k
        judge_spec(x, info, s, ref, name)
        G.close()
    s = specs[f"cheb{deg}-shift-{n}"]
    G = solver(nls, n, 7, form).set_operator(dev_csr(nls, case))
    L.check(L.lib().nk_gmres_set_shift(G._h, s.shift))
    G.set_chebyshev_preconditioner(deg, s.cheb[1], s.cheb[2])
    x, info = G.solve(s.b, fixed_iters=s.k)
    judge_spec(x, info, s, GR.solve_spec(s), f"cheb{deg}-shift-{n}")
    G.close()


@pytest.mark.parametrize("deg", [1, 2, 5])
@pytest.mark.parametrize("form", ["mgs", "dcgs2"])
def test_chebyshev_matrix_free(nls, form, deg):
    specs = GR.brusselator_specs(R)
    name = f"brus-cheb{deg}-50"
    s = specs[name]
    G = solver(nls, 50, 7, form).set_operator(_brusselator_operator(nls, s.case))
    G.set_chebyshev_preconditioner(deg, s.cheb[1], s.cheb[2])
    x, info = G.solve(s.b, fixed_iters=s.k)
    assert info["iters"] == s.k
    judge_spec(x, info, s, GR.solve_spec(s), name)
    G.close()


# ------------------------------------------------------------------------------------------------------------- i. object reuse
@pytest.mark.parametrize("form", ["mgs", "dcgs2", "dcgs2_1r", "sstep0"])
def test_object_reuse_is_bit_for_bit(nls, dev, form):
    n, m = 99, 7
    case = GR.convdiff_n(n, 0.5)
    ctx = nls.default_context()
    ctx.set_deterministic(True)
    try:
        A = nls.CSRMatrix.from_arrays(case.rowptr, case.colind, case.vals)
        Jd = torch_csr(case, dev)
        b1, b2 = case.b, GR.rhs(n, "b2")
        vals2 = case.vals * GR.positive(case.vals.size, "vals")

        def fresh(setup, b, **kw):
            G2 = solver(nls, n, m, form)
            setup(G2)
            out = G2.solve(b, **kw)
            G2.close()
            return out

        def same(a, b):
            assert np.array_equal(a[0], b[0]) and a[1] == b[1], (a[1], b[1])

        G = solver(nls, n, m, form).set_operator(A)
        csr_op = lambda g: g.set_operator(A)                      # noqa: E731
        fn_op = lambda g: g.set_operator(lambda z: Jd @ z)        # noqa: E731
        same(G.solve(b1, fixed_iters=17), fresh(csr_op, b1, fixed_iters=17))
        same(G.solve(b2, reltol=1e-8, maxiters=500), fresh(csr_op, b2, reltol=1e-8, maxiters=500))
        A.set_values(vals2)
        same(G.solve(b1, fixed_iters=17), fresh(csr_op, b1, fixed_iters=17))
        fn_op(G)
        same(G.solve(b1, fixed_iters=17), fresh(fn_op, b1, fixed_iters=17))
        csr_op(G)
        same(G.solve(b1, fixed_iters=17), fresh(csr_op, b1, fixed_iters=17))
        if form.startswith("sstep"):
            L = lib()
            for bs, basis in ((4, 1), (0, 0)):
                L.check(L.lib().nk_gmres_set_block_size(G._h, bs))
                L.check(L.lib().nk_gmres_set_sstep_basis(G._h, basis))

                def setup(g, bs=bs, basis=basis):
                    g.set_operator(A)
                    L.check(L.lib().nk_gmres_set_block_size(g._h, bs))
                    L.check(L.lib().nk_gmres_set_sstep_basis(g._h, basis))
                same(G.solve(b1, fixed_iters=17), fresh(setup, b1, fixed_iters=17))
        G.close()
    finally:
        ctx.set_deterministic(False)


# ------------------------------------------------------------------------------------------------------------- j. degenerate inputs
@pytest.mark.parametrize("form", GR.FORMS)
def test_zero_rhs(nls, form):
    n = 63
    case = GR.convdiff_n(n, 0.5)
    G = solver(nls, n, 7, form).set_operator(dev_csr(nls, case))
    x, info = G.solve(np.zeros(n))
    assert (info["iters"], info["converged"], info["failed"], info["rnorm0"]) == (0, True, False, 0.0)
    GR.check_exact(x, np.zeros(n))
    # x0 ≠ 0 iterates towards 0
    s = GR.group_specs()["zero-rhs-63"]
    x, info = G.solve(s.b, x0=s.x0, fixed_iters=s.k)
    assert info["iters"] == s.k and info["rnorm0"] > 1.0 and np.linalg.norm(x) < 0.1 * np.linalg.norm(s.x0)
    judge_spec(x, info, s, GR.solve_spec(s), "zero-rhs-63")


@pytest.mark.parametrize("form", GR.FORMS)
def test_non_finite_inputs_fail_cleanly(nls, dev, form):
    import torch
    n = 63
    case = GR.convdiff_n(n, 0.5)
    G = solver(nls, n, 7, form).set_operator(dev_csr(nls, case))
    for bad in (np.nan, np.inf):
        b = case.b.copy()
        b[5] = bad
        _, info = G.solve(b, maxiters=40)
        assert info["failed"] and not info["converged"], info
    Jd = torch_csr(case, dev)
    calls = []

    def op(z):
        calls.append(1)
        y = Jd @ z
        if len(calls) >= 3:    # from the third application on
            y = y.clone()
            y[7] = float("nan")
        return y
    G.set_operator(op)
    _, info = G.solve(case.b, maxiters=40)
    assert info["failed"] and not info["converged"], info
    # the object is usable afterwards
    G.set_operator(dev_csr(nls, case))
    s = GR.group_specs()["plain-63"]
    x, info = G.solve(case.b, fixed_iters=17)
    judge_spec(x, info, s, GR.solve_spec(s), "plain-63")
    G.close()


@pytest.mark.parametrize("m", [1, 30])
@pytest.mark.parametrize("form", GR.FORMS)
def test_one_unknown(nls, form, m):
    case = GR.convdiff_n(1, 2.0)
    x, info = solver(nls, 1, m, form).set_operator(dev_csr(nls, case)).solve(case.b)
    assert info["converged"] and info["iters"] == 1 and not info["failed"], info
    exact = case.b[0] / case.vals[0]
    assert abs(x[0] - exact) <= np.spacing(abs(exact)), (x[0], exact)


@pytest.mark.parametrize("form", GR.FORMS)
def test_no_unknowns_is_a_converged_empty_solve(nls, form):
    """include/mi355x_nk.h: on one rank n = 0 is a converged solve of zero iterations that launches nothing and touches
    neither b nor x"""
    L = lib()
    G = solver(nls, 0, 7, form)
    info = L.GmresInfo()
    info.iters, info.rnorm = 99, 1.0
    calls = []
    fn = L.MATVEC_FN(lambda *a: calls.append(1) or 0)
    L.check(L.lib().nk_gmres_set_operator_fn(G._h, fn, None))
    L.check(L.lib().nk_gmres_solve(G._h, None, None, L.HOST, 0, 0.0, 1e-8, 10, 0, C.byref(info)))
    assert (info.iters, info.restarts, info.converged, info.failed, info.rnorm0, info.rnorm) == (0, 0, 1, 0, 0.0, 0.0)
    assert not calls
    G.close()
