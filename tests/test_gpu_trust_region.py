"""The trust-region step on the device (csrc/nk_solver.hip: dogleg with k_dogleg_segment, tr_solve with k_tr_trial, tr_defaults,
tr_radii, the accept/reject bookkeeping of internal_step) against the long-double step of tests/tr_reference.py, one step at a
time: every step is judged from the device's OWN previous iterate and radius, for all seven radius-update schemes, on inputs
that reach every decision branch (tests/test_tr_reference.py shows that, and that the same protocol rejects eighteen planted
defects, without a GPU). The cases, bounds and assertions are tr_reference's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tr_reference as TR  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not TR.LONGDOUBLE_OK, reason="np.longdouble has fewer than 64 significand bits"),
              pytest.mark.filterwarnings("ignore::RuntimeWarning")]

CASES = TR.all_cases()
WORST = TR.Worst()


@pytest.fixture(autouse=True)
def _no_test_after_a_device_fault():
    """a device fault ends the session: nothing more is started on a device that has faulted"""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except Exception as e:  # pragma: no cover
        pytest.exit(f"the device reported a fault after this test: {e}", returncode=3)


def device_problem(nls, dev, prob):
    """the torch twin of a tr_reference problem (the built-in kernel for bratu3) and its start"""
    import torch
    if prob.name == "bratu3":
        return nls.NonlinearProblem(nls.Bratu2D(TR.Bratu3.NS, TR.Bratu3.LAM), u0=prob.u0.copy())
    if prob.name.startswith("ros"):
        def f(du, u, p):
            du[:-1] = 10.0 * (u[1:] - u[:-1] * u[:-1])
            du[-1] = 1.0 - u[-1]

        def jac(Jv, u, p):       # values of the upper bidiagonal pattern, row by row
            Jv[0:-1:2] = -20.0 * u[:-1]
            Jv[1:-1:2] = 10.0
            Jv[-1] = -1.0
    else:
        def f(du, u, p):
            du.copy_(TR.nf_parts(u)[0])

        def jac(Jv, u, p):       # values of the diagonal pattern
            Jv.copy_(TR.nf_parts(u)[1])
    proto = nls.CSRMatrix.from_arrays(prob.rowptr.astype(np.int32), prob.colind.astype(np.int32),
                                      np.asarray(prob.jac_values(prob.u0), dtype=np.float64))
    fn = nls.NonlinearFunction(f, jac=jac, jac_prototype=proto)
    return nls.NonlinearProblem(fn, torch.tensor(prob.u0, dtype=torch.float64, device=dev))


def host(x):
    return x.cpu().numpy().astype(np.float64) if hasattr(x, "cpu") else np.array(x, dtype=np.float64)


class Device:
    """the device's cache behind the interface tr_reference.judge_run drives"""

    def __init__(self, nls, dev, c):
        alg = nls.TrustRegion(**c.alg)     # linsolve left at its default: the direct solve
        self.problem = device_problem(nls, dev, TR.problem(c.prob))
        self.cache = nls.init(self.problem, alg, abstol=1e-200, maxiters=1000, store_trace=True)
        self.rows = 0
        self.u0 = self.cache.u       # a copy of the start in the start's own memory space

    def u(self):
        return host(self.cache.u)

    def fu(self):
        return host(self.cache.fu)

    def radius(self):
        return self.cache.trust_region

    def retcode(self):
        return self.cache.retcode

    def step(self):
        self.cache.step()
        trace = self.cache.trace
        assert len(trace) == self.rows + 1, f"{len(trace) - self.rows} new trace rows after one step"
        self.rows += 1
        return trace[-1]

    def reinit(self):
        self.cache.reinit(self.u0)
        self.rows = 0

    def close(self):
        self.cache.close()


@pytest.mark.parametrize("name", list(CASES))
def test_trust_region_step_by_step(nls, dev, name):
    """init, then K single steps; after each: u, fu, the radius, the new trace row and the retcode against the long-double
    step from the device's previous u and radius — ρ, the acceptance, the radius (the initial one too), ‖f‖∞, ‖δu‖₂ of the
    proposed step, u and fu bit-unchanged after a rejection, the decisions those of the float64 twin,
    ShrinkThresholdExceeded at exactly the reference's step."""
    c = CASES[name]
    d = Device(nls, dev, c)
    try:
        labels = TR.judge_run(c, d, worst=WORST)
        assert labels == [s.labels for s in TR.twin_run(name)[1]]
        if c.alg["max_shrink_times"] == 2 and name.endswith("shrink2"):
            assert d.retcode() == "ShrinkThresholdExceeded" and len(labels) < TR.KMAX
            rows = d.rows
            d.cache.step()                 # a stopped cache does not step
            assert len(d.cache.trace) == rows
    finally:
        d.close()


@pytest.mark.parametrize("scheme", range(7), ids=TR.SCHEME_NAMES)
def test_initial_radius_of_every_scheme(nls, dev, scheme):
    """tr_defaults and tr_radii before the first step: the scheme's own defaults (every option 0), the constructor's options, a
    given radius (which Yuan overrides with p1·‖Jᵀf‖) and a given maximum, on every problem"""
    for prob in ("ros9", "nf", "bratu3", "ros2051"):
        for kw in (TR.ALL_ZERO, {}, dict(initial_trust_radius=0.05), dict(max_trust_radius=0.01, **TR.ALL_ZERO)):
            c = TR.case("x", prob, scheme, **kw)
            p = TR.problem(prob)
            want = TR.tr_radii(c.alg, TR.tr_defaults(c.alg), p, np.asarray(p.u0, dtype=TR.LD))[1]
            d = Device(nls, dev, c)
            got = d.radius()
            d.close()
            print(TR.SCHEME_NAMES[scheme], prob, kw, got, float(want))
            # three roundings of a norm's sum, a square root, a product or a power: 1e-13 is the module's floor
            assert abs(TR.LD(got) - want) <= TR.FLOOR * want, (prob, kw, got, float(want))


@pytest.mark.parametrize("name", TR.REINIT_CASES)
def test_reinit_restores_p1_the_radius_and_the_counter(nls, dev, name):
    """Yuan and Fan change p1 as they go; after reinit from the same start a second run repeats the first bit for bit"""
    d = Device(nls, dev, CASES[name])
    try:
        TR.judge_reinit(CASES[name], d)
    finally:
        d.close()


def test_zz_report_largest_deviations():
    """not a check: the largest deviation of the device from the reference per quantity, over everything run above"""
    print("largest device deviation per quantity:", {k: f"{v:.3e}" for k, v in WORST.dev.items()})
