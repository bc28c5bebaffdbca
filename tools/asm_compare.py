#!/usr/bin/env python3
"""Compare two directories of device-only assembly (csrc/Makefile: `make asm`) kernel by kernel.

    python tools/asm_compare.py BEFORE_DIR AFTER_DIR [--moved KERNEL_SUBSTRING=UNIT ...]
                                [--renamed OLD=NEW ...] > report.md

For every unit (<unit>.s in either directory) and every kernel in it the script compares
  - the body: the lines between the kernel's symbol label and its `.Lfunc_end<k>` label, with
    comments stripped, the kernel's own symbol and the function's index k within the unit normalised
    away (local labels `.LBB<k>_12`, `.Lfunc_end<k>`, `.Ltmp...` are positional: kernels that leave a
    unit renumber them);
  - the metadata: VGPR / AGPR / SGPR counts, spill counts, private segment (scratch) and LDS size.
A kernel that moved to another unit (--moved simplex_kernel=kmpc_solve_simplex) is compared across
the two units. A kernel that was renamed (--renamed bt_run_kernel=bt_kernel) is paired with the
kernel whose demangled name is the same after the substitution — same parameter list, same template
arguments, those plus an added trailing pack, or those with one argument inserted — and both names
are reported. Prints a markdown
report; exit status 1 if any kernel present on both sides differs.
"""
import argparse
import functools
import os
import re
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".private_segment_fixed_size", ".group_segment_fixed_size")


def parse_unit(path):
    """-> {kernel symbol: (body lines, metadata dict)}"""
    with open(path) as f:
        lines = f.read().split("\n")
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    bodies = {}
    i = 0
    while i < len(lines):
        m = re.match(r"(\S+):\s*(;.*)?$", lines[i])
        if m and m.group(1) in names:
            name, body = m.group(1), []
            i += 1
            while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
                ln = lines[i].split(";")[0].rstrip()
                # the function's index within the unit, out of every local label
                ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
                ln = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1", ln)
                if ln.strip():
                    body.append(ln.replace(name, "<self>"))
                i += 1
            bodies[name] = body
        i += 1
    # the metadata: one item of the amdhsa.kernels list per kernel, its own keys at four columns
    meta, block, in_meta = {}, [], False
    for ln in lines:
        in_meta = in_meta or ln.strip() == ".amdgpu_metadata"
        if not in_meta:
            continue
        if ln.startswith("  - .") or not ln.startswith("  "):
            _close(block, meta)
            block = []
        block.append(ln)
    _close(block, meta)
    return {n: (bodies.get(n, []), meta.get(n, {})) for n in names}


def _close(block, meta):
    d = {}
    for ln in block:
        m = re.match(r"  [ -] (\.[a-z_]+):\s*(\S+)\s*$", ln)
        if m:
            d[m.group(1)] = m.group(2)
    if ".name" in d and ".symbol" in d:
        meta[d[".name"]] = {k: d.get(k, "-") for k in META_KEYS}


@functools.lru_cache(maxsize=None)
def short(name):
    try:
        import subprocess
        out = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        return out.replace("kmpc::", "").replace("(anonymous namespace)::", "") or name
    except OSError:
        return name


def split_name(dem):
    """demangled `void f<targs>(params)` -> (`void f`, targs, params)"""
    m = re.match(r"([^<(]*)(?:<(.*)>)?\((.*)\)$", dem)
    return m.groups(default="") if m else (dem, "", "")


def one_inserted(targs, t2):
    """t2 is targs with one template argument inserted (a new parameter ahead of a trailing pack)"""
    a, b = targs.split(", "), t2.split(", ")
    return len(b) == len(a) + 1 and any(b[:i] + b[i + 1:] == a for i in range(len(b)))


def renamed_to(k, renamed, candidates):
    """The symbol among candidates that kernel k is called after --renamed, or None"""
    for old, new in renamed.items():
        if old not in short(k):
            continue
        name, targs, params = split_name(short(k))
        name = name.replace(old, new)
        for k2 in candidates:
            n2, t2, p2 = split_name(short(k2))
            if n2 == name and p2 == params and (t2 == targs or t2.startswith(targs + ", ") or one_inserted(targs, t2)):
                return k2
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--moved", action="append", default=[], metavar="SUBSTR=UNIT",
                    help="kernels whose symbol contains SUBSTR are looked up in UNIT on the after side")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW",
                    help="kernels whose name contains OLD are paired with the one named with NEW in its place")
    a = ap.parse_args()
    moved = dict(m.split("=", 1) for m in a.moved)
    renamed = dict(m.split("=", 1) for m in a.renamed)
    units = sorted({f[:-2] for d in (a.before, a.after) for f in os.listdir(d) if f.endswith(".s")})
    parsed = {side: {u: parse_unit(os.path.join(d, u + ".s")) if os.path.exists(os.path.join(d, u + ".s")) else {}
                     for u in units} for side, d in (("b", a.before), ("a", a.after))}
    n_same = n_diff = 0
    gone, new = [], []
    print("| unit | kernel | body lines | VGPR / AGPR / SGPR | spills V / S | scratch B | LDS B | verdict |")
    print("|---|---|---|---|---|---|---|---|")
    claimed = set()
    for u in units:
        for k, (body, meta) in parsed["b"][u].items():
            u2 = next((dst for sub, dst in moved.items() if sub in k), u)
            after = parsed["a"].get(u2, {})
            k2 = k if k in after else renamed_to(k, renamed, after)
            if k2 is None:
                gone.append((u, k))
                continue
            other = after[k2]
            claimed.add((u2, k2))
            same = body == other[0] and meta == other[1] and len(body) > 0
            n_same += same
            n_diff += not same
            where = u if u2 == u else f"{u} -> {u2}"
            verdict = "identical" if same else "**DIFFERS** (after: %d lines, %s)" % (len(other[0]), other[1])
            print("| %s | `%s` | %d | %s / %s / %s | %s / %s | %s | %s | %s |" % (
                where, short(k) if k2 == k else "%s` -> `%s" % (short(k), short(k2)), len(body),
                meta[".vgpr_count"], meta[".agpr_count"], meta[".sgpr_count"],
                meta[".vgpr_spill_count"], meta[".sgpr_spill_count"], meta[".private_segment_fixed_size"],
                meta[".group_segment_fixed_size"], verdict))
    for u in units:
        new += [(u, k) for k in parsed["a"][u] if (u, k) not in claimed]
    print()
    print("%d kernels identical, %d differ." % (n_same, n_diff))
    print()
    print("Kernels only in the first directory (%d):" % len(gone))
    for u, k in gone:
        print("- %s: `%s`" % (u, short(k)))
    print()
    print("Kernels only in the second directory (%d):" % len(new))
    for u, k in new:
        print("- %s: `%s`" % (u, short(k)))
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
