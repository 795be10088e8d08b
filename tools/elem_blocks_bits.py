"""Are the one-block programs of the compiled element problems (csrc/nk_elem.hip) the parent's? The kernel text gained a block
form under -DNK_ELEM_BLOCKS=1 and every program the option -DNK_BLOCK; without the first the compiler must see the text it saw
before. Every problem of the table tests/elem_reference.py, both programs (residual + JVP; the element matrices), through
nk_elem_code_object of this build and of another build of the package, without a GPU, compared section by section: .text (the
instructions), .rodata (the kernel descriptors) and .note (the kernels' metadata: registers, LDS, arguments). The whole files
are compared too; they may differ where the compiler names a symbol after a hash of the translation unit.

    python tools/elem_blocks_bits.py --parent <root of the other checkout, built> [--out profiles/elem_blocks_bits.txt]

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


def collect(root):
    import ctypes as C
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))   # (the table is this checkout's: the same sources for both builds)
    import elem_reference as R
    from nonlinearsolve_jl_amd import _lib as L
    lib, rows = L.lib(), {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(R.PROBLEMS):
            p = R.PROBLEMS[name]
            for jac in (0, 1):
                args = (p.source.encode(), p.npe, p.dof, len(p.params), p.nnode, p.nelem, jac)
                nb = C.c_int64()
                assert lib.nk_elem_code_object(*args, None, 0, C.byref(nb)) == 0, lib.nk_last_error()
                buf = C.create_string_buffer(nb.value)
                assert lib.nk_elem_code_object(*args, buf, nb.value, C.byref(nb)) == 0
                path = os.path.join(tmp, "k.co")
                with open(path, "wb") as fh:
                    fh.write(buf.raw[:nb.value])
                row = {"file": hashlib.sha256(buf.raw[:nb.value]).hexdigest(), "bytes": nb.value}
                for sec in SECTIONS:
                    out = os.path.join(tmp, "sec.bin")
                    subprocess.run([OBJCOPY, "-O", "binary", "--only-section=" + sec, path, out], check=True)
                    with open(out, "rb") as fh:
                        row[sec] = hashlib.sha256(fh.read()).hexdigest()
                rows[f"{name} | {'element matrices' if jac else 'residual + JVP'}"] = row
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
