#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of the same sources, kernel by kernel.

    hipcc <flags of anoddpm_amd/build.py> --cuda-device-only -S csrc/X.hip -o DIR/X.s      (once per build)
    python tools/isa_diff.py BEFORE_DIR AFTER_DIR [-o table.txt]

Per kernel: the resource fields of the code object's metadata (registers, spills, scratch, LDS) and the opcode histogram.  The
fields and the counts of the matrix, LDS, memory, barrier and wait instructions are the "must be equal" set of a refactor that is
meant to change no machine code; other opcodes are listed where they differ.  Exit status 1 if a must-be-equal figure differs or
the kernel sets differ.
"""
import argparse
import collections
import os
import re
import subprocess
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")
STRICT = ("v_mfma_", "ds_", "buffer_", "global_", "s_barrier", "s_waitcnt")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """-> {kernel symbol: (fields dict, opcode Counter, instruction lines)}"""
    text = open(path).read().split("\n")
    meta, cur = {}, None
    for line in text:                                  # metadata: a YAML list of kernels, keys in alphabetical order
        s = line.strip()
        if s.startswith("- .agpr_count:") or s.startswith("- .args:"):
            cur = {}
        if cur is not None:
            m = re.match(r"-?\s*(\.\w+):\s*(\S+)$", s)
            if m:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == ".name":
                    meta[m.group(2)] = cur
    body, name = {}, None
    for line in text:
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and m.group(1) in meta:
            name = m.group(1)
            body[name] = []
            continue
        if name and line.startswith(".Lfunc_end"):
            name = None
        if name and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            body[name].append(line.split(";")[0].strip())
    out = {}
    for k, f in meta.items():
        ops = collections.Counter(l.split()[0] for l in body.get(k, []))
        out[k] = ({x: f.get(x, "?") for x in FIELDS}, ops, body.get(k, []))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("-o", "--out")
    args = ap.parse_args()
    lines, bad = [], False
    for f in sorted(x for x in os.listdir(args.before) if x.endswith(".s")):
        a, b = parse(os.path.join(args.before, f)), parse(os.path.join(args.after, f))
        names = demangle(sorted(set(a) | set(b)))
        lines.append(f"== {f}: {len(a)} kernels before, {len(b)} after")
        if set(a) != set(b):
            bad = True
            lines += [f"   ONLY BEFORE: {names[k]}" for k in sorted(set(a) - set(b))]
            lines += [f"   ONLY AFTER:  {names[k]}" for k in sorted(set(b) - set(a))]
        for k in sorted(set(a) & set(b)):
            fa, oa, la = a[k]
            fb, ob, lb = b[k]
            strict = lambda o: {x: n for x, n in o.items() if x.startswith(STRICT)}
            same_f, same_s = fa == fb, strict(oa) == strict(ob)
            verdict = "identical" if la == lb else ("same opcode counts, order or operands differ" if oa == ob else
                                                    ("strict counts equal, other opcodes differ" if same_f and same_s else "DIFFERENT"))
            bad |= not (same_f and same_s)
            lines.append(f"   {names[k]}")
            lines.append("      " + " ".join(f"{x[1:]}={fb[x]}" for x in FIELDS) + f"  instructions={sum(ob.values())}  -> {verdict}")
            for x in FIELDS:
                if fa[x] != fb[x]:
                    lines.append(f"      FIELD {x}: {fa[x]} -> {fb[x]}")
            for x in sorted(set(oa) | set(ob)):
                if oa[x] != ob[x]:
                    lines.append(f"      {'STRICT ' if x.startswith(STRICT) else ''}{x}: {oa[x]} -> {ob[x]}")
    lines.append("RESULT: " + ("a must-be-equal figure differs" if bad else "all resource fields and strict opcode counts equal"))
    text = "\n".join(lines) + "\n"
    if args.out:
        open(args.out, "w").write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
