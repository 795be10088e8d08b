"""The Julia generator tests/golden/make_reference_golden.jl cannot run here (no Julia). What CAN be checked without Julia:
every keyword it passes to the reference's constructors and entry points, and every internal symbol it touches, exists in the
reference — a generator that dies on its first `init` because of a misspelt keyword is worth nothing on the day someone runs it
(Next #3). What the reference accepts and defines was read from its source into tests/golden/reference_api.json
(tests/golden/make_reference_api.py), so the check needs no copy of the reference."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "tests", "golden", "reference_api.json")
GEN = os.path.join(ROOT, "tests", "golden", "make_reference_golden.jl")


def _split_top(s):
    """split at top-level commas / semicolons"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch in ",;" and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    out.append(cur)
    return [x.strip() for x in out if x.strip()]


def _calls(src, name):
    """argument strings of every call `name(...)` in src"""
    out = []
    for m in re.finditer(r"(?<![\w.!])" + re.escape(name) + r"\(", src):
        i, depth = m.end(), 1
        while depth and i < len(src):
            depth += src[i] in "([{"
            depth -= src[i] in ")]}"
            i += 1
        out.append(src[m.end():i - 1])
    return out


def _kwargs_used(src, name):
    ks = set()
    for args in _calls(src, name):
        for a in _split_top(args):
            m = re.match(r"^([A-Za-z_Ͱ-Ͽ₀-ₜ][\wͰ-Ͽ₀-ₜ!]*)\s*=(?!=)", a)
            if m:
                ks.add(m.group(1))
    return ks


@pytest.fixture(scope="module")
def gen():
    return open(GEN, encoding="utf-8").read()


@pytest.fixture(scope="module")
def api():
    return json.load(open(API, encoding="utf-8"))


@pytest.mark.parametrize("ctor", ["NewtonRaphson", "TrustRegion", "EisenstatWalkerForcing2"])
def test_constructor_keywords_exist_in_the_reference(gen, api, ctor):
    # lib/NonlinearSolveFirstOrder/src/{raphson,trust_region,eisenstat_walker}.jl
    used = _kwargs_used(gen, ctor)
    sig = set(api["constructor_keywords"][ctor])
    assert sig, f"no keyword signature of {ctor} in {API}"
    assert used <= sig, f"{ctor}: the generator passes {sorted(used - sig)}; the reference accepts {sorted(sig)}"


def test_init_and_reinit_keywords_exist_in_the_reference(gen, api):
    # init(prob, alg; kwargs...) → SciMLBase.__init(prob, alg::GeneralizedFirstOrderAlgorithm, args...; …) (solve.jl:140-150)
    sig = set(api["init_keywords"])
    used = set()
    for args in _calls(gen, "run_case"):
        # keywords behind the top-level ';' of run_case(...) are forwarded to init
        depth, cut = 0, None
        for i, ch in enumerate(args):
            depth += ch in "([{"
            depth -= ch in ")]}"
            if ch == ";" and depth == 0:
                cut = i
        if cut is not None:
            for a in _split_top(args[cut + 1:]):
                m = re.match(r"^(\w+)\s*=(?!=)", a)
                if m:
                    used.add(m.group(1))
    used.discard("kwargs")
    assert used and used <= sig, f"init: the generator forwards {sorted(used - sig)}; __init takes {sorted(sig)}"
    rsig = set(api["reinit_keywords"])   # InternalAPI.reinit_self!
    rused = _kwargs_used(gen, "reinit!")
    assert rused and rused <= rsig, (sorted(rused), sorted(rsig))


def test_external_keywords_and_internal_symbols_are_the_ones_the_reference_uses(gen, api):
    """KrylovJL_GMRES / NonlinearFunction live in LinearSolve.jl / SciMLBase.jl [EXT, not in the tree]: their keywords are
    checked against the reference's own call sites (tests, docs); internal accessors against their definitions."""
    # `gmres_restart` is LinearSolve.jl's own keyword (KrylovJL(…; gmres_restart = 0, window = 0, …) [EXT]); the
    # reference never sets it, so the tree cannot confirm it — it is the ONE keyword of the generator taken on trust
    ext_on_trust = {"gmres_restart"}
    for kw in _kwargs_used(gen, "KrylovJL_GMRES") - ext_on_trust:
        assert kw in api["KrylovJL_GMRES_call_site_keywords"], f"KrylovJL_GMRES({kw} = …) is used nowhere in the reference"
    for kw in _kwargs_used(gen, "NonlinearFunction"):
        assert kw in api["NonlinearFunction_keywords"], f"NonlinearFunction(…; {kw} = …) is used nowhere in the reference"
    defs = api["NonlinearSolveBase_definitions"]
    assert {"not_terminated", "get_fu", "get_u", "step!"} <= set(defs)
    for sym, found in defs.items():
        if sym.split()[0].rstrip("!") in gen or sym.startswith("NLStats"):
            assert found, f"{sym}: not defined in lib/NonlinearSolveBase"
    for fld in ("nsteps", "nf", "njacs", "nfactors", "nsolve"):
        assert re.search(r"st\." + fld + r"\b", gen) and fld in api["NonlinearSolveBase_stats_fields"]
