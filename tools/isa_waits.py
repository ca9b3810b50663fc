#!/usr/bin/env python3
"""Memory-request / wait sequence of the kernels in a hipcc assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-fast-math --cuda-device-only -S -Iinclude anoddpm_amd/csrc/X.hip -o /tmp/X.s
    python tools/isa_waits.py /tmp/X.s <substring of the mangled kernel name> [--loops] [--mem] [--all]

Per basic block (label to label) one line: the order in which vector-memory loads (`L`, `Lk` when the address register pair is
derived from the kernarg base s[0:1]), stores (`S`), LDS reads / writes (`r` / `w`), MFMAs (`M`), barriers (`|`) and
`s_waitcnt vmcnt(n)` (`v<n>`) appear, run-length compressed.  `--loops` prints only blocks that branch back to themselves, `--mem` only blocks with a vector-memory request or a vmcnt wait,
`--all` every kernel whose name contains the substring (default: the first).  A reading aid next to isa_blocks.py: vmcnt retires
in order, so a `v0` in the middle of a block drains every request in flight, whatever the source meant to keep ahead."""
import re
import sys


def kernels(lines, key):
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z[\w$.]*):", lines[i])
        if m and key in m.group(1):
            j = i + 1
            while j < len(lines) and not lines[j].strip().startswith(".Lfunc_end"):
                j += 1
            yield m.group(1), lines[i + 1:j]
            i = j
        i += 1


def token(op, s, karg):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "M"
    if op.startswith(("buffer_load", "global_load", "flat_load", "scratch_load")):
        if op.startswith("global_load"):
            m = re.search(r"v\[(\d+):\d+\]", s.split(",", 1)[1] if "," in s else "")
            if m and int(m.group(1)) in karg:
                return "Lk"
        return "L"
    if op.startswith(("buffer_store", "global_store", "flat_store", "scratch_store", "buffer_atomic", "global_atomic")):
        return "S"
    if op.startswith(("ds_read", "ds_load")):
        return "r"
    if op.startswith("ds_"):
        return "w"
    if op == "s_barrier":
        return "|"
    if op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", s)
        if m:
            return "v" + m.group(1)
    return None


def compress(seq):
    out, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        out.append(seq[i] if j - i == 1 else f"{seq[i]}x{j - i}")
        i = j
    return " ".join(out)


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    loops_only, mem_only, every = "--loops" in sys.argv, "--mem" in sys.argv, "--all" in sys.argv
    lines = open(args[0]).read().split("\n")
    found = False
    for name, body in kernels(lines, args[1]):
        found = True
        print(f"kernel {name}")
        label, seq, back, karg = "entry", [], False, set()
        nk, base_live = 0, True                  # s[0:1] holds the kernarg base until something (in listing order) writes it

        def flush():
            if seq and (back or not loops_only) and (not mem_only or any(t[0] in "LSv" for t in seq)):
                print(f"  {label:>10}{' LOOP' if back else '     '}  {compress(seq)}")

        for l in body:
            s = l.strip()
            m = re.match(r"^(\.LBB[0-9_]+):", s)
            if m:
                flush()
                label, seq, back = m.group(1), [], False
                continue
            if not s or s.startswith((";", ".")):
                continue
            s = s.split(";")[0].strip()
            if not s:
                continue
            op = s.split()[0]
            if re.match(r"^s_\S+\s+(s\[0:1\]|s0|s1)\b", s) and not op.startswith(("s_cmp", "s_cbranch", "s_waitcnt")):
                base_live = False
            # a VGPR pair formed from the kernarg base (tracked until overwritten)
            md = re.match(r"^\S+\s+v\[(\d+):\d+\]", s)
            if md:
                if base_live and re.search(r"\bs\[0:1\]", s) and op.startswith(("v_lshl_add_u64", "v_mov_b64", "v_add")):
                    karg.add(int(md.group(1)))
                elif not op.startswith(("global_load", "global_store")):
                    karg.discard(int(md.group(1)))
            t = token(op, s, karg)
            if t:
                nk += t == "Lk"
                seq.append(t)
            if op.startswith("s_cbranch") or op == "s_branch":
                if s.split()[-1] == label:
                    back = True
        flush()
        print(f"  loads addressed from the kernarg base: {nk}")
        if not every:
            break
    if not found:
        sys.exit(f"no kernel matching {args[1]!r}")


if __name__ == "__main__":
    main()
