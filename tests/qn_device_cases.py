"""Device twins of the cases of tests/broyden_reference.py, and the step loop the Broyden, Klement and polyalgorithm GPU tests
share: u and fu after every step, the reset count after every step."""
import numpy as np

import broyden_reference as R


def problem(nls, name, dev):
    """(NonlinearProblem, the algorithm object, maxiters) of a restatement case"""
    import torch
    _f, u0, kw, _upto = R.CASES[name]
    kw = dict(kw)
    maxiters = kw.pop("maxiters", 1000)
    klement = kw.pop("method", "broyden") == "klement"
    n = len(u0)
    u0t = torch.tensor(u0, dtype=torch.float64, device=dev)
    if "bratu" in name:
        prob = nls.NonlinearProblem(nls.Bratu2D(int(round(n ** 0.5)), 6.0), u0t)
    elif "nonsym" in name:
        def f(du, u, p):
            torch.mul(u, u, out=du)
            du.sub_(2.0)
            du.add_(torch.roll(u, -1), alpha=0.1)
        prob = nls.NonlinearProblem(nls.NonlinearFunction(f), u0t)
    elif "stall" in name:
        def f(du, u, p):
            torch.mul(u, u, out=du)
            du.sub_(2.0)
            du[-1] = 1.0
            du[-2] = 0.0
        prob = nls.NonlinearProblem(nls.NonlinearFunction(f), u0t)
    elif "reset" in name:
        def f(du, u, p):
            torch.mul(u, u, out=du)
            du.sub_(2.0)
            du[-1] = 1.0
        prob = nls.NonlinearProblem(nls.NonlinearFunction(f), u0t)
    else:
        prob = nls.NonlinearProblem(nls.Quadratic(n, 2.0), u0t)
    alg = nls.Klement(**kw) if klement else nls.Broyden(**kw)
    return prob, alg, maxiters


def run(nls, name, dev, cache=None):
    """steps the cache until it stops (or the case's step limit); (cache, [u], [fu], [nresets after each step])"""
    prob, alg, maxiters = problem(nls, name, dev)
    steps = R.CASES[name][3]
    if cache is None:
        cache = nls.init(prob, alg, abstol=R.ABSTOL, maxiters=maxiters)
    us, fus, resets = [], [], []
    while not cache.force_stop and cache.nsteps < maxiters and (steps is None or cache.nsteps < steps):
        nls.step_(cache)
        resets.append(cache.qn_state["nresets"])
        if cache.retcode != "ConvergenceFailure":
            us.append(cache.u.cpu().numpy())
            fus.append(cache.fu.cpu().numpy())
    return cache, us, fus, resets


def reset_steps(resets):
    return [k for k, (a, b) in enumerate(zip([0] + resets[:-1], resets), start=1) if b > a]


def assert_parity(name, us, fus):
    ref, bnd = R.run(name), R.bounds(name)
    assert len(us) == len(ref.us), (len(us), len(ref.us))
    for k, (u, fu, ur, fr, (bu, bf)) in enumerate(zip(us, fus, ref.us, ref.fus, bnd), start=1):
        eu, ef = float(np.max(np.abs(u - ur))), float(np.max(np.abs(fu - fr)))
        print(f"{name} step {k}: |du| {eu:.3e} (bound {bu:.3e})  |dfu| {ef:.3e} (bound {bf:.3e})")
        assert eu <= bu and ef <= bf, (name, k, eu, bu, ef, bf)


def assert_control_flow(name, cache, resets):
    ref = R.run(name)
    assert cache.nsteps == ref.nsteps and reset_steps(resets) == ref.reset_steps, (cache.nsteps, ref.nsteps, resets, ref.reset_steps)
    assert (cache.retcode if cache.force_stop else None) == ref.retcode, (cache.retcode, ref.retcode)
    assert cache.qn_state["nresets"] == ref.nresets
