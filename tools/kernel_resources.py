"""Registers, spills and code size of every kernel in hipcc object files, from the gfx950 code object's metadata.

    python tools/kernel_resources.py genvox_amd/csrc/attention.o genvox_amd/csrc/attn_persist.o [--json out.json]
    python tools/kernel_resources.py --diff before.json after.json

One line per kernel symbol: VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, bytes of code (the symbol's size).  --diff lists the
symbols of `before` whose numbers differ in `after` (or that are gone) and the symbols that are new; exit status 1 if a symbol of
`before` differs.  Symbols are compared by their demangled names with trailing `false` template arguments dropped, so that a
kernel that gained a defaulted `bool VARIANT = false` parameter is matched with what it was.  Used for the "the existing instantiations did not change" tables of EXPERIMENTS.md.
"""
from __future__ import annotations

import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "code_bytes")


def _code_objects(obj: str, tmp: str) -> list[str]:
    local = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, stdout=subprocess.DEVNULL)
    return sorted(p for p in glob.glob(local + ".*") if "gfx950" in p)


def kernels_of(obj: str) -> dict[str, dict[str, int]]:
    out: dict[str, dict[str, int]] = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in _code_objects(obj, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", co], check=True, capture_output=True, text=True).stdout
            size = {}
            for line in syms.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    size[f[7]] = int(f[2], 0) if not f[2].isdigit() else int(f[2])
            cur: dict[str, int] = {}
            name = None

            def flush():
                if name is not None:
                    out[name] = {k: cur.get(k, 0) for k in FIELDS[:-1]} | {"code_bytes": size.get(name, -1)}

            keys = {"agpr_count": "agpr", "sgpr_count": "sgpr", "sgpr_spill_count": "sgpr_spill", "vgpr_count": "vgpr", "vgpr_spill_count": "vgpr_spill"}
            for line in notes.splitlines():
                m = re.match(r"\s*(- )?\.(\w+):\s*(\S+)\s*$", line)
                if not m:
                    continue
                key, val = m.group(2), m.group(3)
                if key == "agpr_count":   # first key of a kernel's block (keys are in alphabetical order)
                    flush()
                    cur, name = {}, None
                if key in keys:
                    cur[keys[key]] = int(val)
                elif key == "symbol":
                    name = val[:-3] if val.endswith(".kd") else val
            flush()
    return out


def _canonical(table: dict[str, dict[str, int]]) -> dict[str, dict[str, int]]:
    names = list(table)
    dem = subprocess.run([shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
    out = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        while True:
            e = re.sub(r"(, false>|<false>)\(", lambda m: (">(" if m.group(1).startswith(",") else "("), d, count=1)
            if e == d:
                break
            d = e
        out[d] = table[n]
    return out


def main(argv: list[str]) -> int:
    if argv and argv[0] == "--diff":
        before, after = (_canonical(json.load(open(p))) for p in argv[1:3])
        bad = 0
        for k, v in sorted(before.items()):
            if after.get(k) != v:
                bad += 1
                print(f"CHANGED {k}: {v} -> {after.get(k)}")
        for k in sorted(set(after) - set(before)):
            print(f"NEW     {k}: {after[k]}")
        print(f"{len(before)} symbols before, {len(before) - bad} of them identical after, {len(set(after) - set(before))} new")
        return 1 if bad else 0
    out_json = None
    if "--json" in argv:
        i = argv.index("--json")
        out_json = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    table: dict[str, dict[str, int]] = {}
    for obj in argv:
        table.update(kernels_of(obj))
    for k, v in sorted(table.items()):
        print(" ".join(f"{f}={v[f]}" for f in FIELDS), k)
    if out_json:
        json.dump(table, open(out_json, "w"), indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
