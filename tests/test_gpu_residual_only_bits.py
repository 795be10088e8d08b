"""The residual-only solvers' trajectories, bit for bit: LimitedMemoryBroyden, DFSane, Broyden and Klement (csrc/nk_qn.hip and
their drivers in nk_solver.hip) stepped with nls.step_, and after every step the SHA-256 of u and of fu as bytes, compared
with the digests pinned in tests/golden/residual_only_bits.json. Every sum of these solvers has a fixed order — within a thread,
within a wavefront, across the four wavefronts, across the workgroups — so the digests are a property of the code, not of a
run: each case is run twice and must give the same digests both times, and those must be the pinned ones.

The pins were recorded on an MI355X at the commit the JSON names, before the reduction epilogues of nk_qn.hip were merged into
one. They may be re-recorded only by a change whose purpose is to alter a summation order, and never by a refactor: a refactor
that moves a digest has changed an order, and is wrong.

All grids at these sizes are far below the 2·num_cus cap of the reduce passes, so the pins do not depend on the CU count. The
callback cases `stall` and `nonsym` are left out: their residual is computed by torch."""
import hashlib
import json
import os

import pytest

import broyden_reference as RB
import dfsane_reference as RS
import lbroyden_reference as RL
import qn_device_cases as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "residual_only_bits.json")
CASES = [("lbroyden", "quadratic4099_spread"), ("lbroyden", "quadratic64_t3"), ("lbroyden", "bratu16_t10"),
         ("dfsane", "quadratic4099_spread"), ("dfsane", "quadratic64_nexp1"),
         ("broyden", "broyden65_good"), ("broyden", "broyden1000_bad"), ("broyden", "broyden2049_good"),
         ("broyden", "broyden4099_diagonal"), ("klement", "klement4099"), ("klement", "klement_reset64")]


def _cache(nls, family, name, dev):
    """(a fresh cache of the case, the step limit or None)"""
    import torch
    if family in ("broyden", "klement"):
        prob, alg, maxiters = D.problem(nls, name, dev)
        return nls.init(prob, alg, abstol=RB.ABSTOL, maxiters=maxiters), RB.CASES[name][3]
    R = RL if family == "lbroyden" else RS
    _f, u0, kw, upto = R.CASES[name]
    u0t = torch.tensor(u0, dtype=torch.float64, device=dev)
    if name.startswith("bratu"):
        prob = nls.NonlinearProblem(nls.Bratu2D(int(round(len(u0) ** 0.5)), 6.0), u0t)
    else:
        prob = nls.NonlinearProblem(nls.Quadratic(len(u0), 2.0), u0t)
    alg = nls.LimitedMemoryBroyden(**kw) if family == "lbroyden" else nls.DFSane(**kw)
    return nls.init(prob, alg, abstol=R.ABSTOL), upto


def digests(nls, family, name, dev):
    """{"u": [digest after each step], "fu": [...]} of one run of the case"""
    cache, upto = _cache(nls, family, name, dev)
    out = {"u": [], "fu": []}
    while not cache.force_stop and cache.nsteps < 1000 and (upto is None or cache.nsteps < upto):
        nls.step_(cache)
        out["u"].append(hashlib.sha256(cache.u.cpu().numpy().tobytes()).hexdigest())
        out["fu"].append(hashlib.sha256(cache.fu.cpu().numpy().tobytes()).hexdigest())
    cache.close()
    return out


@pytest.mark.parametrize("family,name", CASES)
def test_trajectory_bits_are_the_pinned_ones(nls, dev, family, name):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    pinned = golden["cases"][f"{family}/{name}"]
    first, second = digests(nls, family, name, dev), digests(nls, family, name, dev)
    print(f"{family}/{name}: {len(first['u'])} steps (pinned {len(pinned['u'])}), recorded at {golden['recorded_at_commit']}")
    assert len(first["u"]) == len(first["fu"]) > 0
    assert first == second        # two runs, the same bits
    assert first == pinned        # and they are the recorded ones
