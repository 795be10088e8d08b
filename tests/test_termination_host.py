"""The termination cache (csrc/nk_termination.h: nine modes, two norms, patience test, stall test, protective threshold, best
objective) is plain host arithmetic on four reduced quantities, so it is checked here without a GPU: tests/solver_host_dump.cpp
is compiled with g++ against the header and fed, as hex floats, the quantities numpy computes from sequences of small vectors
(fu, u, uprev); oracle/reference_restatement.py's TerminationCache is fed the vectors themselves. After every call the verdict
(stop, whether the best iterate moved), the retcode, the step count and the best objective must be equal — exactly: the
objective goes through one square root and one division on both sides, both correctly rounded."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import reference_restatement as R  # noqa: E402
from test_linesearch_host import dump  # noqa: E402,F401  (the fixture that builds tests/solver_host_dump.cpp)

N = 4
ABSTOL, RELTOL, PATIENCE, MULTIPLIER, MIN_MAX, STALLED_STEPS, PROTECTIVE = 1e-8, 1e-6, 3, 3.0, 1.3, 4, 10.0
REL_MODES = (R.TM_RELNORM_SAFE, R.TM_RELNORM_SAFEBEST)
SAFE_MODES = (R.TM_ABSNORM_SAFEBEST, R.TM_ABSNORM_SAFE) + REL_MODES


# ----------------------------------------------------------------------------- sequences of (fu, u) ; uprev is the u before
def _sequence(objectives, steps, seed, norm, rel, poison=None):
    """iterates near u = (1, 1, 1, 1)/2 whose residual makes the mode's objective (‖fu‖, or ‖fu‖ / ‖fu + u‖ to first order)
    what is given at each step and which move by about the given step lengths; poison = (step, value) puts a NaN or ∞ into fu"""
    nrm = R.Linf_NORM if norm == "inf" else R.L2_NORM
    rng = np.random.default_rng(seed)
    u = 0.5 + 0.01 * rng.standard_normal(N)
    out = []
    for k, (obj, st) in enumerate(zip(objectives, steps)):
        u = u + st * rng.uniform(0.2, 0.5, N) * rng.choice([-1.0, 1.0], N)
        fu = rng.uniform(0.5, 1.0, N) * rng.choice([-1.0, 1.0], N)
        fu = fu * (obj * (nrm(u) if rel else 1.0) / nrm(fu))
        if poison is not None and poison[0] == k:
            fu[1] = poison[1]
        out.append((fu, u.copy()))
    return out


def sequences(mode, norm):
    """name → [(fu, u) …]; the first pair initialises the cache"""
    rel = mode in REL_MODES
    crit = RELTOL if rel else ABSTOL      # the mode's tolerance

    def _seq(objectives, steps, seed, poison=None):
        return _sequence(objectives, steps, seed, norm, rel, poison)
    wiggle = [2.0 * crit * (1.0 + 0.05 * (k % 3)) for k in range(9)]
    return {
        "converges": _seq([1.0, 1e-2, 1e-4, 1e-12, 1e-14], [0.1] * 5, 1),
        "nan": _seq([1.0, 0.5, 0.25, 0.1, 0.05], [0.1] * 5, 2, poison=(3, float("nan"))),
        "inf": _seq([1.0, 0.5, 0.25, 0.1, 0.05], [0.1] * 5, 3, poison=(2, float("inf"))),
        "blows_up": _seq([1e-3 * 7.0 ** k for k in range(6)], [0.1] * 6, 4),
        # just above the tolerance, within the patience multiplier of it, hardly changing: the patience test — with a trace
        # shorter than the ring (3 checks: no verdict yet) and longer (the ring wraps)
        "hovers_short": _seq([1.0] + wiggle[:3], [0.1] * 4, 5),
        "hovers_long": _seq([1.0] + wiggle, [0.1] * 10, 5),
        # far above the tolerance, and u hardly moves: the stall test on ‖u − uprev‖₂, absolute (≤ abstol) and relative
        "creeps": _seq([100.0 * crit] * 10, [0.1] + [1e-9] * 9, 6),
        # far above the tolerance, u keeps moving: Failure after every check, both rings wrap
        "wanders": _seq([100.0 * crit * (1.0 + 0.3 * ((k * 5) % 7)) for k in range(12)], [0.1] * 12, 7),
        # up and down: the best objective moves on some checks only
        "up_and_down": _seq([1.0, 0.5, 0.7, 0.3, 0.4, 0.35, 0.1, 0.2, 0.05], [0.1] * 9, 8),
    }


def quantities(fu, u, uprev, norm, reltol):
    nrm = R.Linf_NORM if norm == "inf" else R.L2_NORM
    with np.errstate(invalid="ignore"):   # ∞ − ∞ where fu holds an ∞: NaN, as on the device
        viol = float(np.max(np.abs(fu) - reltol * np.abs(u + fu)))
    return [nrm(fu), nrm(fu + u), viol, R.Linf_NORM(fu), R.L2_NORM(u - uprev)]


def run_both(exe, mode, norm, protective, stalled_steps, seq, reinit_at=None):
    """[(stop, best moved, retcode, nsteps, best objective)] after the (re)initialisation and after every check: the header's and
    the restatement's; reinit_at: that pair re-initialises both caches instead of being checked"""
    lines, want = [], []
    tc = None
    for k, (fu, u) in enumerate(seq):
        if k == 0 or k == reinit_at:
            if tc is None:
                tc = R.TerminationCache(fu, u, ABSTOL, RELTOL, mode=mode, norm=norm, patience_steps=PATIENCE,
                                        patience_objective_multiplier=MULTIPLIER, min_max_factor=MIN_MAX,
                                        max_stalled_steps=stalled_steps, protective_threshold=protective)
            else:
                tc.reinit(fu, u)
            q = quantities(fu, u, u, norm, RELTOL)
            lines.append("reset " + " ".join(float(x).hex() for x in q[:4] + [R.L2_NORM(u)]))
            want.append((False, False, tc.retcode, tc.nsteps, float(tc.best_objective_value).hex()))
        else:
            uprev = seq[k - 1][1]
            before = tc.best_objective_value
            stop = tc(fu, u, uprev)
            lines.append("check " + " ".join(float(x).hex() for x in quantities(fu, u, uprev, norm, RELTOL)))
            want.append((bool(stop), tc.best_objective_value != before, tc.retcode, tc.nsteps,
                         float(tc.best_objective_value).hex()))
    args = [exe, "tc", str(mode), float(ABSTOL).hex(), float(RELTOL).hex(), str(PATIENCE), float(MULTIPLIER).hex(),
            float(MIN_MAX).hex(), str(-1 if stalled_steps is None else stalled_steps),
            float(0.0 if protective is None else protective).hex(), str(N)]
    out = subprocess.run(args, input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    got = []
    for ln in out:
        stop, new_best, retcode, nsteps, best = ln.split()
        got.append((bool(int(stop)), bool(int(new_best)), int(retcode), int(nsteps), float.fromhex(best).hex()))
    return got, want


@pytest.mark.filterwarnings("ignore:invalid value")   # the restatement's ∞ / ∞ in the sequence `inf`
@pytest.mark.parametrize("norm", ["inf", "l2"])
@pytest.mark.parametrize("mode", range(9))
def test_same_verdicts(dump, mode, norm):
    """every mode and norm, the protective threshold off and on, the stall test on and off, every sequence, and a
    re-initialisation in the middle of one: the header says what the restatement says after every call — and the sequences
    make the safe modes end in every way the cache knows"""
    seqs = sequences(mode, norm)
    ends = {}
    for protective, stalled_steps, (name, seq) in itertools.product((None, PROTECTIVE), (STALLED_STEPS, None), seqs.items()):
        got, want = run_both(dump, mode, norm, protective, stalled_steps, seq)
        assert got == want, (name, protective, stalled_steps)
        first_stop = next((w for w in want if w[0]), None)
        ends[name, protective, stalled_steps] = (first_stop[2], first_stop[3]) if first_stop else (want[-1][2], None)
    for reinit_at in (2, 5):
        got, want = run_both(dump, mode, norm, PROTECTIVE, STALLED_STEPS, seqs["wanders"][:reinit_at] + seqs["converges"] +
                             seqs["creeps"], reinit_at=reinit_at)
        assert got == want, reinit_at
        assert want[reinit_at][2:4] == (R.DEFAULT, 0) and any(w[2] == R.SUCCESS for w in want)

    on, off = PROTECTIVE, None
    assert ends["converges", off, STALLED_STEPS][0] == R.SUCCESS
    if mode not in SAFE_MODES:      # the plain modes only ever say Success
        assert {e[0] for e in ends.values()} <= {R.DEFAULT, R.SUCCESS}
        return
    # Unstable: a NaN or ∞ objective ; the protective threshold, only where it is set
    assert ends["nan", off, STALLED_STEPS][0] == ends["inf", off, STALLED_STEPS][0] == R.UNSTABLE
    assert ends["blows_up", on, STALLED_STEPS][0] == R.UNSTABLE and ends["blows_up", off, STALLED_STEPS] == (R.FAILURE, None)
    # Stalled by the patience test: on the first check after `patience_steps` of them (the stall test needs one more, and is off
    # in the second run); three checks fill the ring and decide nothing
    assert ends["hovers_long", off, STALLED_STEPS] == ends["hovers_long", off, None] == (R.STALLED, PATIENCE + 1)
    assert ends["hovers_short", off, STALLED_STEPS] == (R.FAILURE, None)
    # Stalled by the stall test, absolute or relative with the mode: only where it is on
    assert ends["creeps", off, STALLED_STEPS] == (R.STALLED, STALLED_STEPS + 1) and ends["creeps", off, None] == (R.FAILURE, None)
    # Failure: twelve checks, nothing decided
    assert ends["wanders", on, STALLED_STEPS] == (R.FAILURE, None)


def test_the_best_objective_moves_only_in_the_best_modes(dump):
    for mode in range(9):
        got, _want = run_both(dump, mode, "inf", None, STALLED_STEPS, sequences(mode, "inf")["up_and_down"])
        moved = [g[1] for g in got]
        if mode in (R.TM_ABSNORM_SAFEBEST, R.TM_RELNORM_SAFEBEST):
            assert True in moved[1:] and False in moved[1:]
        else:
            assert not any(moved)
