"""Compare two builds' gfx950 assembly kernel by kernel (CPU only).

    hipcc --offload-arch=gfx950 <COMMON_FLAGS> --cuda-device-only -S unit.hip -o unit.s   (each unit, both builds)
    python tools/kernel_diff.py --a old/*.s --b new/*.s

Each side is a set of `-S` outputs; a kernel may sit in any file of its side.
For every kernel symbol (`.amdhsa_kernel`) prints `same`, or the two
instruction counts, the number of differing lines and the first few of them.
Comments are stripped and the labels `.LBB<n>_`, `.Ltmp<n>` and
`.Lpost_getpc<n>` (a long branch's) normalised: their numbering depends on
what else shares the file.  Nothing else is interpreted.  Exit status 1 if a
symbol is missing, doubled or differs.
"""
from __future__ import annotations

import argparse
import difflib
import re
import sys

LABELS = re.compile(r"\.LBB\d+_|\.(Ltmp|Lpost_getpc)\d+")


def kernels(paths):
    """{symbol: [instruction lines]}, and the symbols defined more than once."""
    out, doubled = {}, []
    for path in paths:
        with open(path, errors="replace") as fh:
            lines = fh.read().split("\n")
        names = {ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")}
        cur = None
        for ln in lines:
            code = ln.split(";", 1)[0].rstrip()
            if not code.strip():
                continue
            if not code[0].isspace():  # a label at column 0
                label = code.rstrip(":")
                if label in names:
                    if label in out:
                        doubled.append(label)
                    cur = out[label] = []
                elif label.startswith(".Lfunc_end"):
                    cur = None
                continue
            code = code.strip()
            if cur is not None and not code.startswith("."):
                cur.append(LABELS.sub(lambda m: ".LBB_" if m.group().startswith(".LBB") else "." + m.group(1), code))
    return out, doubled


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--a", nargs="+", required=True, help="-S outputs of the first build")
    ap.add_argument("--b", nargs="+", required=True, help="-S outputs of the second build")
    ap.add_argument("--show", type=int, default=4, help="differing lines to print per kernel")
    a = ap.parse_args(argv)
    ka, da = kernels(a.a)
    kb, db = kernels(a.b)
    bad = 0
    for side, doubled in (("a", da), ("b", db)):
        for name in doubled:
            print(f"{name}: defined more than once in {side}")
            bad += 1
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print(f"{name}: only in {'a' if name in ka else 'b'}")
            bad += 1
            continue
        x, y = ka[name], kb[name]
        if x == y:
            print(f"{name}: same ({len(x)} instructions)")
            continue
        bad += 1
        if len(x) == len(y):  # line against line: substitutions
            pairs = [(p, q) for p, q in zip(x, y) if p != q]
            print(f"{name}: {len(x)} / {len(y)} instructions, {len(pairs)} lines differ, one for one")
            for p, q in pairs[:a.show]:
                print(f"    - {p}\n    + {q}")
        else:
            delta = [d for d in difflib.unified_diff(x, y, lineterm="", n=0) if d[0] in "+-" and d[:3] not in ("+++", "---")]
            print(f"{name}: {len(x)} / {len(y)} instructions, {len(delta)} lines differ")
            for d in delta[:a.show]:
                print(f"    {d[0]} {d[1:]}")
    print(f"{len(set(ka) | set(kb))} kernels, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
