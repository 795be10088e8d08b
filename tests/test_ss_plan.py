"""The s-step cycle's dispatch (csrc/nk_ss_plan.h: which sweeps and scalar launches build each block, in which form, on which
grid) is plain host arithmetic, so it is checked here without a GPU: tests/ss_plan_dump.cpp is compiled with g++ against the
header and prints the plans of a cycle. The block list and the launch list must be the ones tools/step_model.py charges for —
which tests/test_step_model.py ties to the committed rocprofv3 timeline — and the invariants nk_ss_cycle states as NK_REQUIREs
must hold under every combination of forms."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import step_model  # noqa: E402

N, NNZ = 1024 * 1024, 5 * 1024 * 1024 - 4 * 1024


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ss_plan") / "ss_plan_dump")
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
                    "-I", os.path.join(ROOT, "nonlinearsolve.jl_amd", "csrc"), os.path.join(ROOT, "tests", "ss_plan_dump.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def _clean_env(**switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NK_SS_")}
    env.update(switches)
    return env


def _cycle(exe, env=None, **cfg):
    """the plans of one cycle: the blocks, then what closes the cycle"""
    r = subprocess.run([exe, "cycle"] + [f"{k}={v}" for k, v in cfg.items()], env=_clean_env(**(env or {})), check=True,
                       capture_output=True, text=True)
    plans = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert plans and plans[-1]["what"] == "finish" and all(p["what"] == "block" for p in plans[:-1])
    return plans[:-1], plans[-1]


def test_block_list_is_the_models(dump):
    for arnoldi in range(1, 65):
        for s in range(1, 16):
            blocks, _ = _cycle(dump, steps=arnoldi, s=s, grow=0)
            assert [(b["k"], b["sb"]) for b in blocks] == step_model.sstep_blocks(arnoldi, s), (arnoldi, s)


@pytest.mark.parametrize("newton,s,widths", [(1, 15, [4, 8, 15, 15]), (0, 6, [2, 4, 6, 6, 6])])
def test_automatic_block_sizes_double(dump, newton, s, widths):
    """a solve that stops on a tolerance: 4, 8, 15, 15 … with the Newton basis, 2, 4, 6, 6 … with the monomial one"""
    steps = sum(widths)
    blocks, _ = _cycle(dump, steps=steps, s=s, grow=1, fixed=0, newton=newton)
    assert [b["sb"] for b in blocks] == widths
    assert [b["k"] for b in blocks] == [1 + sum(widths[:i]) for i in range(len(widths))]


_SSTEP_NAMES = ("k_ss_block<A>", "k_ss_block<B>", "k_ss_block<C>", "k_ss_job", "k_ss_reduce_factor", "k_ss_hess", "k_backsolve")
_OP_NAMES = {"A": "k_ss_block<A>", "B": "k_ss_block<B>", "C": "k_ss_block<C>", "job": "k_ss_job", "tail1": "k_ss_reduce_factor",
             "tail2": "k_ss_reduce_factor", "hess": "k_ss_hess"}


def _plan_launches(blocks, finish):
    """[(model name, HBM bytes)] of a planned cycle; a cycle whose closing launch does not back-substitute leaves that to the
    caller's k_backsolve"""
    out = []
    for p in blocks + [finish]:
        for l in p["launches"]:
            k, w = p["k"], p["sb"]
            by = {"A": 8.0 * N * (k + w), "B": 8.0 * N * (k + (1 if l["nostore"] else 2) * w), "C": 8.0 * N * (k + 2 * w)}.get(l["op"], 0.0)
            out.append((_OP_NAMES[l["op"]], by))
    if not finish["backsolved"]:
        out.append(("k_backsolve", 0.0))
    return out


@pytest.mark.parametrize("model_kw,env", [({}, {}), (dict(implicit=False), dict(NK_SS_IMPLICIT="0")),
                                          (dict(deferred=False), dict(NK_SS_DEFER="0")),
                                          (dict(last_block_unstored=False), dict(NK_SS_NOSTORE="0"))])
def test_default_dispatch_is_what_the_model_charges_for(dump, model_kw, env):
    """bench.py's default step: one rank, fixed work, Newton basis, 30 steps in blocks of 15 at 1024² on 256 CUs, two workgroups
    per CU, an aligned basis with an even leading dimension. Names and bytes of the sweeps and scalar launches, in order."""
    model = [(nm, hbm) for nm, hbm, _alg in step_model.step_launches(N, NNZ, arnoldi=30, s=15, **model_kw) if nm in _SSTEP_NAMES]
    plan = _plan_launches(*_cycle(dump, env, steps=30, s=15, n=N, ldv=N, cus=256, occ=2, single=1, fixed=1, newton=1, back=1))
    if not (model_kw.get("deferred", True) and model_kw.get("implicit", True)):
        # without the deferred factorisation the model still lists round 4's kernel set (k_ss_reduce_factor after every sweep)
        # where the code launches k_ss_job: the scalar launches are compared by position
        scalar = {"k_ss_reduce_factor": "scalar", "k_ss_job": "scalar"}
        model = [(scalar.get(nm, nm), by) for nm, by in model]
        plan = [(scalar.get(nm, nm), by) for nm, by in plan]
    assert plan == model


def test_default_second_block(dump):
    blocks, finish = _cycle(dump, steps=30, s=15, n=N, ldv=N, cus=256, occ=2, single=1, fixed=1, newton=1, back=1)
    assert len(blocks) == 2
    first, second = blocks
    assert first["defer_this"] and first["implicit"] and not first["host_a"] and not first["raw_last"]
    assert second["host_a"] and second["grid_a"] == 256 - 20
    assert second["last_block"] and second["raw_last"] and second["grid_b"] == 256
    a = second["launches"][0]   # sweep A: 20 extra workgroups close the first block
    assert (a["op"], a["grid"], a["host_wgs"], a["who"], a["wk"], a["wsb"]) == ("A", 236, 20, "deferred", 1, 15)
    assert finish["backsolved"] and finish["launches"][-1]["raw_last"]


def _sweep(exe, *args):
    r = subprocess.run([exe, "sweep", *args], env=_clean_env(), capture_output=True, text=True)
    out = json.loads(r.stdout.splitlines()[-1])
    assert r.returncode == 0 and out["violations"] == 0, (args, r.stdout[-3000:], r.stderr[-1000:])
    return out["cycles"]


def test_invariants_hold_under_every_combination_of_forms(dump):
    """steps 1..60 × s 1..15 × automatic growth × {one rank, peers, no peers} × basis × fixed work or tolerance ×
    back-substitution accepted or not × every on/off combination of the switches the planner reads × a host that stops after
    any block; under each: the widths add up, the fix list and the factor slots hold, a block whose sweep B stores nothing is
    closed by a job that back-substitutes, a hosting sweep B has a second workgroup, host_a only on one rank with fixed work,
    nothing pending after the finish, every job mode has an instance, no launch list outgrows its capacity
    (ss_plan_dump.cpp::check_cycle; the header's own assert is live in this build).

    The complete product runs (≈ 7 CPU-minutes on the program's threads, 16 at the most) with two of the thirteen on/off
    switches held at their defaults: NK_SS_RO and NK_SS_RO_GRID. Each is read in one expression of ss_plan_block, the one that
    chooses between two values for sweep B's grid; that grid goes into the sweep's launch and into the count of partial sums
    its reduction is told, and into no flag, mode or other launch. The second pass checks exactly that — a cycle planned
    with them off equals the cycle planned with them on but for that grid, block by block and finish by finish — together
    with the invariants, under every setting with at most two switches off their defaults at every number of steps, and under
    the complete product of all thirteen at steps = 30. NK_SS_GRID_A stays in the product: sweep A's grid is compared with a
    threshold (host_a).

    Every grid of these passes is 256 or more (n = 2²⁰ on 256 CUs), so two more passes at the reduced product run where the
    grids are small: one tile (n = 200: every grid is 1, nothing can be hosted) and 60 tiles (fewer than the 4 · 20 a sweep A
    must exceed to give workgroups up). Factor slots: the workspace has steps + 2 at least; the passes ask for steps, the
    most blocks a cycle can have."""
    cfgs = 15 * (2 * 3 * 2 * 2 * 2)
    at_most_two = 1 + 13 + 13 * 12 // 2 + 2 * (1 + 13)
    assert _sweep(dump, "slots=0", "hold=24") == 60 * cfgs * 2 ** 11 * 3
    assert _sweep(dump, "slots=0", "flips=2", "full_at=30", "grids=1") == cfgs * (59 * at_most_two + 2 ** 13 * 3)
    for n in (200, 60 * 256):
        assert _sweep(dump, "slots=0", "flips=2", f"n={n}") == 60 * cfgs * at_most_two
