#!/usr/bin/env python3
"""Per-kernel resource table from the compiler's own report (no GPU needed).

    python tools/kernel_resources.py table [--csrc DIR] > branch.tsv
    python tools/kernel_resources.py diff parent.tsv branch.tsv

`table` compiles every device source of datago_amd/build.py for gfx950 with
-Rpass-analysis=kernel-resource-usage and prints one line per kernel
instantiation: demangled name, SGPRs, VGPRs, AGPRs, scratch bytes per lane,
occupancy (waves per SIMD) and static LDS bytes.  --csrc points at another
checkout's datago_amd/csrc (the parent commit's, say).

`diff` prints the kernels whose figures differ, and those only one side has.
Template arguments that a commit adds with a default (k_huff_sync<false> ->
k_huff_sync<false, 3>) change a name, not a kernel: --alias OLD=NEW maps them.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def short(name: str) -> str:
    """dg::k_x<8, true>(args...) -> k_x<8, true>"""
    name = name.replace("void ", "", 1) if name.startswith("void ") else name
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            name = name[:i]
            break
    return name.replace("dg::", "")


def table(csrc: str) -> list[tuple]:
    sys.path.insert(0, ROOT)
    from datago_amd.build import COMMON, SOURCES, ARCH
    flags = [f for f in COMMON if not f.startswith("-I")]
    inc = [f"-I{csrc}", f"-I{os.path.join(os.path.dirname(os.path.dirname(csrc)), 'include')}"]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for src, device in SOURCES:
            if not device:
                continue
            cmd = [HIPCC] + flags + inc + [f"--offload-arch={ARCH}", "-x", "hip", "-c", os.path.join(csrc, src), "-o",
                                           os.path.join(tmp, "o.o"), "-Rpass-analysis=kernel-resource-usage"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode:
                raise SystemExit(r.stderr)
            cur = None
            for line in r.stderr.splitlines():
                m = re.search(r"remark: Function Name: (\S+)", line)
                if m:
                    cur = {"name": m.group(1), "src": src}
                    rows.append(cur)
                    continue
                for key, col in FIELDS:
                    m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
                    if m and cur is not None:
                        cur[col] = int(m.group(1))
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout
    out = []
    for r, n in zip(rows, names.splitlines()):
        out.append((r["src"], short(n)) + tuple(r.get(col, -1) for _, col in FIELDS))
    return sorted(out)


def load(path: str) -> dict:
    d = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        f = line.rstrip("\n").split("\t")
        d[(f[0], f[1])] = tuple(int(x) for x in f[2:])
    return d


def main() -> int:
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("table")
    t.add_argument("--csrc", default=os.path.join(ROOT, "datago_amd", "csrc"))
    d = sub.add_parser("diff")
    d.add_argument("old")
    d.add_argument("new")
    d.add_argument("--alias", action="append", default=[])
    a = ap.parse_args()
    if a.cmd == "table":
        print("# source\tkernel\t" + "\t".join(col for _, col in FIELDS))
        for row in table(os.path.abspath(a.csrc)):
            print("\t".join(str(x) for x in row))
        return 0
    alias = dict(x.split("=", 1) for x in a.alias)
    old, new = load(a.old), load(a.new)
    changed = 0
    for (src, k), v in sorted(old.items()):
        k2 = alias.get(k, k)
        if (src, k2) not in new:
            print(f"missing in new: {src} {k}")
            changed += 1
        elif new[(src, k2)] != v:
            print(f"changed: {src} {k}: {v} -> {new[(src, k2)]}")
            changed += 1
    known = {(s, alias.get(k, k)) for s, k in old}
    for key in sorted(set(new) - known):
        print(f"new: {key[0]} {key[1]}: {new[key]}")
    print(f"{len(old)} kernels at the old side, {changed} differ")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
