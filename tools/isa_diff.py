#!/usr/bin/env python
"""Kernel-by-kernel gfx950 ISA comparison of translation units between two trees (a refactor's proof that no kernel changed).

    python tools/isa_diff.py OLD_TREE [--tuning UNIT ...] UNIT.hip ... > profiles/<name>_isa.txt

Each unit is compiled in OLD_TREE and in this tree as build.py compiles it, plus -save-temps=obj (the units after --tuning with
-DSIGE_HIP_TUNING as well), the assembly is normalised -- lines that are only comments or .file / .ident / .loc
directives dropped, `;` comments and trailing blanks stripped -- and cut into kernels.  Kernels are paired in order of appearance
(the mangled name of a kernel carries its argument types, which a refactor may rename: a kernel's own name is replaced by KERNEL
in its text).  Per kernel: the number of differing instruction lines and the metadata row (VGPR, AGPR, SGPR, LDS bytes, scratch,
kernarg bytes).  Exit status 1 if anything differs."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from sige_amd import build  # noqa: E402

DROP = re.compile(r"^\s*(;|\.file\b|\.ident\b|\.loc\b|$)")
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")


def compile_to_asm(tree: str, unit: str, defs) -> str:
    with tempfile.TemporaryDirectory() as work:
        csrc = os.path.join(tree, "sige_amd", "csrc")
        cmd = [build._hipcc(), *build.FLAGS, "-DSIGE_TU_ID=%d" % build.SOURCES.index(unit), *defs, "-I" + os.path.join(tree, "include"), "-I" + csrc, "-c", os.path.join(csrc, unit),
               "-o", os.path.join(work, "out.o"), "-save-temps=obj"]
        subprocess.run(cmd, check=True, cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        (asm,) = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
        return open(os.path.join(work, asm)).read()


def kernels(asm: str):
    """[(mangled name, [normalised instruction lines], metadata row)] in order of appearance."""
    lines = [re.sub(r"\s*;.*$", "", ln).rstrip() for ln in asm.split("\n") if not DROP.match(ln)]
    meta = {}
    for block in asm.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1)) for key in META)
    out = []
    for name in meta:
        start = lines.index(name + ":")
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        out.append((name, [ln.replace(name, "KERNEL") for ln in lines[start:end]], meta[name]))
    return out


def main(argv):
    old_tree, units, tuning = argv[0], [], False
    for arg in argv[1:]:
        if arg == "--tuning":
            tuning = True
        else:
            units.append((arg, ["-DSIGE_HIP_TUNING"] if tuning else []))
    bad = 0
    print("# %s: old tree against new tree, flags %s" % (os.path.basename(__file__), " ".join(build.FLAGS)))
    print("# metadata row = (VGPR, AGPR, SGPR, LDS bytes, scratch bytes, kernarg bytes)")
    for unit, defs in units:
        old, new = kernels(compile_to_asm(old_tree, unit, defs)), kernels(compile_to_asm(REPO, unit, defs))
        names = subprocess.run(["c++filt"], input="\n".join(n for n, _, _ in new), capture_output=True, text=True).stdout.split("\n")
        rows, differing = [], 0
        for (_, ta, ma), (_, tb, mb), shown in zip(old, new, names):
            d = sum(1 for ln in difflib.unified_diff(ta, tb, lineterm="", n=0) if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
            differing += d + (ma != mb)
            rows.append("  %-6s %5d lines  %s%s  %s" % ("same" if d == 0 and ma == mb else "DIFFER", len(tb), mb,
                                                     "" if ma == mb else " (old %s)" % (ma,), shown.split("(")[0]))
        if len(old) != len(new):
            differing += 1
        print("%s %s: %d kernels compared (old tree %d), %d differing lines" % (unit, " ".join(defs), len(new), len(old), differing))
        print("\n".join(rows))
        bad += differing
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
