#!/usr/bin/env python
"""Generates tests/golden/reference_api.json: the facts about NonlinearSolve.jl's API that tests/test_golden_generator.py and
tests/test_abi.py check the repository against, read once from a checkout of the reference so that the tests need no copy of it.

    python tests/golden/make_reference_api.py <NonlinearSolve.jl checkout> [out.json]

The file holds names only (keyword names of the constructors and entry points the Julia generator
tests/golden/make_reference_golden.jl calls, keywords found at the reference's own call sites, whether the internal accessors it
touches are defined, package UUIDs and one [compat] bound) — no code of the reference."""
import json
import os
import re
import sys

import tomli

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_golden_generator import _calls, _split_top  # noqa: E402

FO = os.path.join("lib", "NonlinearSolveFirstOrder", "src")
NSB = os.path.join("lib", "NonlinearSolveBase")
# internal symbols of lib/NonlinearSolveBase the generator may use, and how a definition of each is recognised
DEFINITIONS = (("not_terminated", r"function not_terminated|not_terminated\(cache\)\s*="),
               ("get_fu", r"get_fu\(cache"), ("get_u", r"get_u\(cache"), ("step!", r"function CommonSolve\.step!|step!\("),
               ("NLStats fields (SciMLBase [EXT]; reset field by field in abstract_types.jl:43-50)", r"stats\.nf\s*=\s*0"))
STATS_FIELDS = ("nsteps", "nf", "njacs", "nfactors", "nsolve")
ASSIGNED = re.compile(r"\b(\w+)\s*=")


def signature_kwargs(path, fname):
    """keyword names of `function fname(...; kw...)` (first method with keywords) in a reference file"""
    src = open(path, encoding="utf-8").read()
    for args in _calls(src, "function " + fname) + _calls(src, fname):
        depth, cut = 0, None
        for i, ch in enumerate(args):
            depth += ch in "([{"
            depth -= ch in ")]}"
            if ch == ";" and depth == 0:
                cut = i
                break
        if cut is None:
            continue
        names = set()
        for a in _split_top(args[cut + 1:]):
            m = re.match(r"^([^\s=:.]+)", a)
            if m:
                names.add(m.group(1))
        if names:
            return sorted(names)
    return []


def sources(ref, sub=""):
    for dp, _dn, fn in os.walk(os.path.join(ref, sub)):
        if "/.git" in dp:
            continue
        for f in sorted(fn):
            if f.endswith((".jl", ".md")):
                try:
                    yield open(os.path.join(dp, f), encoding="utf-8", errors="ignore").read()
                except OSError:
                    pass


def main(ref, out):
    fo = os.path.join(ref, FO)
    facts = {"constructor_keywords": {c: signature_kwargs(os.path.join(fo, f), c) for c, f in
                                      (("NewtonRaphson", "raphson.jl"), ("TrustRegion", "trust_region.jl"),
                                       ("EisenstatWalkerForcing2", "eisenstat_walker.jl"))},
             "init_keywords": signature_kwargs(os.path.join(fo, "solve.jl"), "SciMLBase.__init"),
             "reinit_keywords": signature_kwargs(os.path.join(fo, "solve.jl"), "InternalAPI.reinit_self!")}
    gmres, nlf = set(), set()
    for src in sources(ref):
        for m in re.finditer(r"KrylovJL_GMRES\([^)]*", src):     # keywords set at the reference's KrylovJL_GMRES(…) call sites
            gmres.update(ASSIGNED.findall(m.group(0)))
        for m in re.finditer(r"NonlinearFunction\{?[^\n]*", src):  # … and on the lines of its NonlinearFunction(…) calls
            nlf.update(ASSIGNED.findall(m.group(0)))
    for src in sources(ref, "lib"):
        nlf.update(re.findall(r"\bf\.(\w+)\b", src))                # fields read off a NonlinearFunction
    facts["KrylovJL_GMRES_call_site_keywords"] = sorted(gmres)
    facts["NonlinearFunction_keywords"] = sorted(nlf)
    nsb = list(sources(ref, NSB))
    facts["NonlinearSolveBase_definitions"] = {s: any(re.search(p, src) for src in nsb) for s, p in DEFINITIONS}
    nsb_src = list(sources(ref, os.path.join(NSB, "src")))
    facts["NonlinearSolveBase_stats_fields"] = [f for f in STATS_FIELDS if any(re.search(r"\b" + f + r"\b", s) for s in nsb_src)]
    known = {}
    for rel in ("Project.toml", "lib/NonlinearSolveBase/Project.toml", "lib/SciMLJacobianOperators/Project.toml"):
        t = tomli.load(open(os.path.join(ref, rel), "rb"))
        known[t["name"]] = t["uuid"]
        for sec in ("deps", "weakdeps", "extras"):
            known.update(t.get(sec, {}))
    facts["manifest_uuids"] = dict(sorted(known.items()))
    facts["LinearSolve_compat"] = tomli.load(open(os.path.join(ref, "Project.toml"), "rb"))["compat"]["LinearSolve"]
    with open(out, "w", encoding="utf-8") as fh:
        json.dump(facts, fh, indent=1, ensure_ascii=False)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                          "reference_api.json"))
