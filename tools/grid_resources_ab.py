"""Resource notes of every generated grid kernel (csrc/nk_grid.hip) of this build against another build of the package, without
a GPU: every problem of the five PROBLEMS tables under tests/, both programs, both forms of the fill. The fifth table
(tests/gridbc_reference.py) has a boundary kind per side, which a parent from before NK_GRID_SIDES refuses: its kernels are new,
and are listed with this build's figures alone.

    python tools/grid_resources_ab.py --parent <root of the other checkout, built> [--out profiles/<name>.txt]

For each kernel: LDS bytes equal, private segment and spilled VGPRs 0 in both, and the waves-per-SIMD step that VGPRs + AGPRs
allow (allocation granule 8, min(8, 512 // allocation)) no lower than the parent's; for a new kernel: no private segment, no
spills. Exit status 1 if a row fails.

Each build is read in a child process of its own (two libraries of one name do not share a process); the problems are this
checkout's tables in both.

    python tools/grid_resources_ab.py --slab [--out profiles/<name>.txt]

The programs of a grid split over several ranks (nk_grid_slab_code_object) beside the one-rank program of the same problem, this
build alone: VGPRs and LDS of rank 0, the middle rank and the last rank of three and of rank 0 of two. A cut adds the address
select of the points that can leave through it and, in the fill, the zone counting; the table shows what that costs in
registers. Exit status 1 if a cut program has a private segment or spills, or more LDS than its one-rank program."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/llvm/bin/llvm-readelf"
KERNELS = {2: {0: ("nk_grid_residual", "nk_grid_jvp"), 1: ("nk_grid_jac",)},
           3: {0: ("nk_grid3_residual", "nk_grid3_jvp"), 1: ("nk_grid3_jac",)}}
STENCIL_ID = {"star": 0, "box": 1, "star2": 16, "diamond2": 17}
BOUNDARY_ID = {"dirichlet": 0, "periodic": 1}
SIDE_KIND_ID = {"dirichlet": 0, "periodic": 1, "mirror_node": 2, "mirror_face": 3}


def problems():
    """(table, name, source, dim, dof, stencil, boundary, nparams, nfields) of every problem of the five tables; boundary is
    one of the two old names or a tuple of kinds, one per side"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import grid3_reference as G3
    import grid_r2_reference as G2
    import grid_reference as G1
    import gridf_reference as GF
    import gridbc_reference as GB
    out = []
    for table, mod, dim in (("grid", G1, 2), ("grid3", G3, 3), ("grid_r2", G2, None), ("gridf", GF, None), ("gridbc", GB, None)):
        for name in sorted(mod.PROBLEMS):
            p = mod.PROBLEMS[name]
            out.append((table, name, p.source, dim or p.dim, p.dof, p.stencil, p.boundary, len(p.params), getattr(p, "nfields", 0)))
    return out


def boundary_code(boundary):
    """the library's int: 0 / 1 for the old names, NK_GRID_SIDES for a tuple of kinds"""
    if isinstance(boundary, str):
        return BOUNDARY_ID[boundary]
    code = 1 << 24
    for s, k in enumerate(boundary):
        code |= SIDE_KIND_ID[k] << (4 * s)
    return code


def waves(vgprs, agprs):
    alloc = -(-(vgprs + agprs) // 8) * 8
    return min(8, 512 // max(alloc, 8))


def collect(root):
    """in a child: the notes of every kernel of the build at `root` → JSON on stdout"""
    import ctypes as C
    sys.path.insert(0, root)
    from nonlinearsolve_jl_amd import _lib as L
    lib, rows = L.lib(), {}
    with tempfile.TemporaryDirectory() as tmp:
        for direct in (0, 1):
            os.environ["NK_GRID_FILL_DIRECT"] = str(direct)
            for table, name, source, dim, dof, stencil, boundary, nparams, nfields in problems():
                for jac in (0, 1):
                    if jac == 0 and direct == 1:
                        continue   # (the residual / JVP program does not depend on the form of the fill)
                    args = (source.encode(), dim, dof, STENCIL_ID[stencil], boundary_code(boundary), nparams, nfields, jac)
                    nb = C.c_int64()
                    st = lib.nk_grid_fields_code_object(*args, None, 0, C.byref(nb))
                    if st != 0 and not isinstance(boundary, str) and b"boundary" in lib.nk_last_error():
                        continue   # (a build from before the kinds per side: it has no such kernel)
                    assert st == 0, lib.nk_last_error()
                    buf = C.create_string_buffer(nb.value)
                    assert lib.nk_grid_fields_code_object(*args, buf, nb.value, C.byref(nb)) == 0
                    path = os.path.join(tmp, "k.co")
                    with open(path, "wb") as fh:
                        fh.write(buf.raw[:nb.value])
                    notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
                    for block in re.split(r"\n\s*- \.", notes)[1:]:
                        get = lambda key: re.search(r"\.%s:\s+(\w+)" % key, block)
                        if not (get("name") and get("private_segment_fixed_size")) or get("name").group(1) not in KERNELS[dim][jac]:
                            continue
                        program = "fill, direct" if jac and direct else ("fill, staged" if jac else "residual + JVP")
                        rows[f"{table}/{name}|{get('name').group(1)}|{program}"] = {
                            k: int(get(key).group(1)) if get(key) else 0
                            for k, key in (("private", "private_segment_fixed_size"), ("vgprs", "vgpr_count"),
                                           ("agprs", "agpr_count"), ("spills", "vgpr_spill_count"),
                                           ("lds", "group_segment_fixed_size"))}
    json.dump(rows, sys.stdout)


def notes_of(code, names, tmp):
    """{kernel: {private, vgprs, agprs, spills, lds}} of a code object"""
    path = os.path.join(tmp, "k.co")
    with open(path, "wb") as fh:
        fh.write(code)
    notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.", notes)[1:]:
        get = lambda key: re.search(r"\.%s:\s+(\w+)" % key, block)
        if get("name") and get("private_segment_fixed_size") and get("name").group(1) in names:
            out[get("name").group(1)] = {k: int(get(key).group(1)) if get(key) else 0
                                         for k, key in (("private", "private_segment_fixed_size"), ("vgprs", "vgpr_count"),
                                                        ("agprs", "agpr_count"), ("spills", "vgpr_spill_count"),
                                                        ("lds", "group_segment_fixed_size"))}
    return out


def slab_table(out_path):
    """cut programs beside the one-rank program of every problem of the five tables (the staged fill)"""
    import ctypes as C
    sys.path.insert(0, ROOT)
    from nonlinearsolve_jl_amd import _lib as L
    lib = L.lib()
    ranks = ((1, 0), (3, 0), (3, 1), (3, 2), (2, 0))
    lines = ["# problem | kernel | one rank: VGPRs, LDS | " + " | ".join(f"rank {r} of {R}: VGPRs, LDS" for R, r in ranks[1:]) +
             " | verdict"]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for table, name, source, dim, dof, stencil, boundary, nparams, nfields in problems():
            for jac in (0, 1):
                rows = []
                for R, r in ranks:
                    args = (source.encode(), dim, dof, STENCIL_ID[stencil], boundary_code(boundary), nparams, nfields, R, r, jac)
                    nb = C.c_int64()
                    assert lib.nk_grid_slab_code_object(*args, None, 0, C.byref(nb)) == 0, lib.nk_last_error()
                    buf = C.create_string_buffer(nb.value)
                    assert lib.nk_grid_slab_code_object(*args, buf, nb.value, C.byref(nb)) == 0
                    rows.append(notes_of(buf.raw[:nb.value], KERNELS[dim][jac], tmp))
                for kernel in KERNELS[dim][jac]:
                    ok = all(x[kernel]["private"] == 0 and x[kernel]["spills"] == 0 and x[kernel]["lds"] <= rows[0][kernel]["lds"]
                             for x in rows)
                    bad += not ok
                    lines.append(f"{table}/{name} | {kernel} | " + " | ".join(f"{x[kernel]['vgprs']}, {x[kernel]['lds']}" for x in rows)
                                 + f" | {'ok' if ok else 'FAIL'}")
    lines.append(f"# {len(lines) - 1} kernels, {bad} failed (a private segment, spills, or more LDS than on one rank)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out_path:
        with open(out_path, "w", encoding="utf-8") as fh:
            fh.write(text)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slab", action="store_true", help="the cut programs beside the one-rank programs of this build")
    ap.add_argument("--parent", help="root of the other checkout (built)")
    ap.add_argument("--out", help="write the table here as well")
    ap.add_argument("--collect", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.collect:
        return collect(a.collect)
    if a.slab:
        return slab_table(a.out)
    if not a.parent:
        ap.error("--parent is required")
    both = [json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--collect", os.path.abspath(r)],
                                      capture_output=True, text=True, check=True).stdout) for r in (a.parent, ROOT)]
    old, new = both
    assert old and set(old) <= set(new) and all(k.startswith("gridbc/") for k in set(new) - set(old)), \
        "the two builds do not have the same old kernels"
    lines = ["# problem | kernel | program | parent VGPRs (+AGPRs) -> waves/SIMD | new VGPRs (+AGPRs) -> waves/SIMD | LDS parent / new "
             "| private, spills (new) | verdict"]
    bad = 0
    for key in sorted(old):
        o, n = old[key], new[key]
        wo, wn = waves(o["vgprs"], o["agprs"]), waves(n["vgprs"], n["agprs"])
        ok = (o["lds"] == n["lds"] and n["private"] == 0 and n["spills"] == 0 and o["private"] == 0 and o["spills"] == 0
              and wn >= wo)
        bad += not ok
        lines.append(f"{' | '.join(key.split('|'))} | {o['vgprs']} (+{o['agprs']}) -> {wo} | {n['vgprs']} (+{n['agprs']}) -> {wn} | "
                     f"{o['lds']} / {n['lds']} | {n['private']}, {n['spills']} | {'ok' if ok else 'FAIL'}")
    for key in sorted(set(new) - set(old)):   # the kernels the parent does not have
        n = new[key]
        ok = n["private"] == 0 and n["spills"] == 0
        bad += not ok
        lines.append(f"{' | '.join(key.split('|'))} | - | {n['vgprs']} (+{n['agprs']}) -> {waves(n['vgprs'], n['agprs'])} | "
                     f"- / {n['lds']} | {n['private']}, {n['spills']} | {'new, ok' if ok else 'FAIL'}")
    lines.append(f"# {len(old)} kernels of both builds, {len(new) - len(old)} new, {bad} failed")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
