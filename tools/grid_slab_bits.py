"""Are the one-rank programs of the compiled grid problems (csrc/nk_grid.hip) the parent's? Every problem of the five PROBLEMS
tables under tests/, both programs, both forms of the fill, compiled by this build and by another build of the package, without
a GPU, and compared section by section: .text (the instructions), .rodata (the kernel descriptors) and .note (the kernels'
metadata: registers, LDS, arguments). The whole files are compared too; they may differ where the compiler names a symbol after
a hash of the translation unit (__hip_cuid_…), which changes with any edit of the device text.

    python tools/grid_slab_bits.py --parent <root of the other checkout, built> [--out profiles/<name>.txt]

Exit status 1 if .text, .rodata or .note of any program differ. Each build is read in a child process of its own."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJCOPY = "/opt/rocm/llvm/bin/llvm-objcopy"
SECTIONS = (".text", ".rodata", ".note")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import grid_resources_ab as gab   # noqa: E402  (the tables and the codes)


def collect(root):
    import ctypes as C
    sys.path.insert(0, root)
    from nonlinearsolve_jl_amd import _lib as L
    lib, rows = L.lib(), {}
    with tempfile.TemporaryDirectory() as tmp:
        for direct in (0, 1):
            os.environ["NK_GRID_FILL_DIRECT"] = str(direct)
            for table, name, source, dim, dof, stencil, boundary, nparams, nfields in gab.problems():
                for jac in (0, 1):
                    if jac == 0 and direct == 1:
                        continue
                    args = (source.encode(), dim, dof, gab.STENCIL_ID[stencil], gab.boundary_code(boundary), nparams, nfields, jac)
                    nb = C.c_int64()
                    assert lib.nk_grid_fields_code_object(*args, None, 0, C.byref(nb)) == 0, lib.nk_last_error()
                    buf = C.create_string_buffer(nb.value)
                    assert lib.nk_grid_fields_code_object(*args, buf, nb.value, C.byref(nb)) == 0
                    path = os.path.join(tmp, "k.co")
                    with open(path, "wb") as fh:
                        fh.write(buf.raw[:nb.value])
                    row = {"file": hashlib.sha256(buf.raw[:nb.value]).hexdigest(), "bytes": nb.value}
                    for sec in SECTIONS:
                        out = os.path.join(tmp, "sec.bin")
                        subprocess.run([OBJCOPY, "-O", "binary", "--only-section=" + sec, path, out], check=True)
                        with open(out, "rb") as fh:
                            row[sec] = hashlib.sha256(fh.read()).hexdigest()
                    program = "fill, direct" if jac and direct else ("fill, staged" if jac else "residual + JVP")
                    rows[f"{table}/{name} | {program}"] = row
    json.dump(rows, sys.stdout)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="root of the other checkout (built)")
    ap.add_argument("--out", help="write the table here as well")
    ap.add_argument("--collect", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.collect:
        return collect(a.collect)
    if not a.parent:
        ap.error("--parent is required")
    old, new = [json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--collect", os.path.abspath(r)],
                                          capture_output=True, text=True, check=True).stdout) for r in (a.parent, ROOT)]
    assert old and set(old) == set(new), "the two builds do not have the same programs"
    lines = ["# problem | program | bytes parent / new | " + " | ".join(SECTIONS) + " | whole file | verdict"]
    bad = whole = 0
    for key in sorted(old):
        o, n = old[key], new[key]
        same = [o[s] == n[s] for s in SECTIONS]
        bad += not all(same)
        whole += o["file"] == n["file"]
        lines.append(f"{key} | {o['bytes']} / {n['bytes']} | " + " | ".join("equal" if s else "DIFFERENT" for s in same) +
                     f" | {'equal' if o['file'] == n['file'] else 'differs'} | {'ok' if all(same) else 'FAIL'}")
    lines.append(f"# {len(old)} programs: {len(old) - bad} with equal {', '.join(SECTIONS)}; {whole} equal as whole files; {bad} failed")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            fh.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
