"""One line per gfx950 kernel of the library: a digest of its machine code and the figures of its kernel descriptor.

    python scripts/kernel_isa_digest.py [-o table.txt]        write the table (default: stdout)
    python scripts/kernel_isa_digest.py --check table.txt     compare with a table written earlier; exit 1 on any difference

Needs hipcc only, no GPU.  Every .hip entry of build.py's LIB_SOURCES is compiled with the build's own flags (and that
entry's extra ones) to assembly, `-S --cuda-device-only`; the files without a kernel (the host side of the C ABI) add
nothing.  Lines are keyed by the kernel's mangled name and sorted, so a kernel that moves to another file, or up and down
in its file, stays the same line:

    <mangled name> <sha256 of the instruction stream> vgpr=<n> sgpr=<n> scratch=<bytes> lds=<bytes>

The instruction stream is the kernel's text from its label to the end of the function with labels and instructions kept,
comments and assembler directives dropped, white space squeezed, and the function's ordinal taken out of the local labels
(.LBB<ordinal>_<n>): what depends on where the kernel stands in its file, and nothing else.  A refactor that is to leave
the kernels alone is checked by comparing its table with the parent commit's.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from course5_amd import build  # noqa: E402

DESCRIPTOR = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
              ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))


def assembly(src, extra, tmp):
    out = os.path.join(tmp, os.path.splitext(src)[0] + ".s")
    subprocess.run([build.HIPCC] + build.COMMON + extra + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", os.path.join(build.CSRC, src), "-o", out], check=True)
    with open(out) as f:
        return f.read().split("\n")


def kernels_of(lines):
    """{mangled name: table line} of one assembly file"""
    found = {}
    descriptors = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        fig = {}
        for j in range(i + 1, len(lines)):
            t = lines[j].split()
            if t and t[0] == ".end_amdhsa_kernel":
                break
            if len(t) >= 2:
                fig[t[0]] = t[1]
        descriptors[m.group(1)] = fig
    for name, fig in descriptors.items():
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        h = hashlib.sha256()
        for ln in lines[start:]:
            if ln.startswith(".Lfunc_end"):
                break
            text = " ".join(ln.split(";")[0].split())
            if not text or (text.startswith(".") and not text.endswith(":")):
                continue  # comment, blank or directive (a local label starts with a dot too, and ends with a colon)
            h.update(re.sub(r"\.LBB\d+_", ".LBB_", text).encode() + b"\n")
        found[name] = f"{name} {h.hexdigest()} " + " ".join(f"{k}={fig[d]}" for k, d in DESCRIPTOR)
    return found


def table():
    units = [(s, x) for s, x in build.LIB_SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        listings = list(pool.map(lambda u: assembly(u[0], u[1], tmp), units))
    rows = {}
    for (src, _), lines in zip(units, listings):
        for name, row in kernels_of(lines).items():
            if name in rows:
                raise SystemExit(f"{name} is defined in two translation units ({src})")
            rows[name] = row
    return [rows[k] for k in sorted(rows)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output")
    ap.add_argument("--check", metavar="TABLE")
    args = ap.parse_args()
    rows = table()
    if args.output:
        with open(args.output, "w") as f:
            f.write("\n".join(rows) + "\n")
    elif not args.check:
        print("\n".join(rows))
    if args.check:
        with open(args.check) as f:
            old = {ln.split()[0]: ln.strip() for ln in f if ln.strip()}
        new = {r.split()[0]: r for r in rows}
        moved = sorted(k for k in old.keys() | new.keys() if old.get(k) != new.get(k))
        for k in moved:
            print(f"- {old.get(k, '(no such kernel)')}\n+ {new.get(k, '(no such kernel)')}")
        print(f"{len(new)} kernels, {len(moved)} differ")
        sys.exit(1 if moved else 0)
