"""Canonical text dump of the op lists the plan compilers emit (unet._Plan, train_plan.TrainPlan), built on CPU tensors: no
device needed, only the host-side helpers of the compiled library.

One line per op of `ops` (inference) or `pack_ops`, `ops`, `bops` (training): the op code and every field of its ctypes
struct.  Integers and floats are printed as they are; a pointer is printed as "owner+byte offset", the owner being a parameter
or its gradient by name, the plan's gradient arena, or a plan buffer numbered by FIRST APPEARANCE in the op stream with its
size in bytes -- so the order of allocation may change between two trees and nothing else may.  A pointer that resolves to
nothing is an error.  The device-resident job tables (PackBatchArgs.jobs / block0, the LinearBwdArgs array of
linear_bwd_batch) are read back and printed the same way, followed by igemm_log, attention_log, igemm_flops, bwd_marks and
block_out.

A plan change that must not change a launch is checked by running THIS file against two trees and comparing the text:

    python tools/plan_dump.py --tree <parent checkout> --matrix --jobs 16 > parent.txt
    python tools/plan_dump.py --tree .                 --matrix --jobs 16 > branch.txt
    python tools/plan_dump.py --compare parent.txt branch.txt > profiles/plan_walk_equivalence.txt

(`--matrix`: one line per cell -- model, batch, plan options, environment switch -- with its op counts and the SHA-256 of its dump;
a cell that cannot be built is an error.  `--compare`: the two summaries joined cell by cell, exit status 1 unless every hash is
equal.  Without either, the full dump of the one cell the options name.)  The models are the CASES of tests/test_gpu_unet.py."""
import argparse
import ast
import bisect
import ctypes
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SWITCHES = ["ANODDPM_CSUM=1", "ANODDPM_CSUM=1 ANODDPM_CSUM_NOFOLD=1", "ANODDPM_ARITH=bf16split3", "ANODDPM_NO_POOL_ACT=1",
            "ANODDPM_NO_RES_UP=1", "ANODDPM_NO_STEM_STATS=1", "ANODDPM_NO_FUSED_ATTENTION=1", "ANODDPM_NO_GN_TAIL=1",
            "ANODDPM_NO_GNB_FUSE=1", "ANODDPM_PACK_BATCH=0", "ANODDPM_BATCH_EMB_FWD=0", "ANODDPM_BATCH_EMB_BWD=0",
            "ANODDPM_NO_WINOGRAD=1",
            # the kernel-selection switches (unet.choose_conv_cfg / smallmap_ok / wino23s_ok and the statistics routes of _Plan.igemm)
            "ANODDPM_NO_SMALLMAP=1", "ANODDPM_NO_WINO23S=1", "ANODDPM_WINO23S_MAXK=128", "ANODDPM_SMALLMAP_CONV_MAXM=64",
            "ANODDPM_NO_F43=1", "ANODDPM_F43_32=0", "ANODDPM_F43_DEEP_SPLITK=0", "ANODDPM_F43_MIN_PIXELS=1024",
            "ANODDPM_NO_STREAM1X1=1", "ANODDPM_NO_WINOGRAD_SPLITK=1", "ANODDPM_SPLITK_TARGET=256", "ANODDPM_GN_TAIL_MAX_P=64",
            "ANODDPM_CSUM=1 ANODDPM_CSUM_MAX_ATOMICS=0", "ANODDPM_CSUM=1 ANODDPM_ARITH=bf16split3"]
# (batch 1 of c2_256_b128: the configuration whose 16x16 maps move between cfg 5 and the Winograd kernels)
SWITCH_MODELS = [("c2_256_b128", 4), ("c2_256_b128", 1), ("i32_b32_h2_a16_8", 2)]
FROZEN_PREFIX = "down."          # the frozen-subset cells freeze every parameter of the down path
IGEMM_HEAD_MODEL = ("i32_b32_c5", dict(img_size=32, base_channels=32, in_channels=5))     # inference only: train_plan.eligible() refuses it


def cases(tree):
    """CASES of tests/test_gpu_unet.py (its CASES expression alone is evaluated: the module itself needs pytest's conftest), plus one model whose head
    takes the igemm + layout route of the inference plan."""
    src = open(os.path.join(tree, "tests", "test_gpu_unet.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "CASES":
            try:
                out = eval(compile(ast.Expression(node.value), "CASES", "eval"), {"__builtins__": {}, "dict": dict})
            except Exception as e:
                raise SystemExit(f"tests/test_gpu_unet.py: CASES must stay a literal of dict(...) calls and constants ({e!r})")
            break
    else:
        raise SystemExit("tests/test_gpu_unet.py: CASES not found")
    out[IGEMM_HEAD_MODEL[0]] = IGEMM_HEAD_MODEL[1]
    return out


def matrix(tree):
    """Every cell as a dict(model, batch, plan, p_drop, want_dx, flat, frozen, env)."""
    cells = []
    names = list(cases(tree))
    for name in names:
        for B in (1, 4, 16):
            cells.append(dict(model=name, batch=B, plan="infer"))
    for name in names[:-1]:                                  # (all but the inference-only model)
        for B in (1, 4, 15, 16):
            for p_drop in (0.0, 0.3):
                for want_dx in (False, True):
                    for flat in (False, True):
                        cells.append(dict(model=name, batch=B, plan="train", p_drop=p_drop, want_dx=want_dx, flat=flat))
        cells.append(dict(model=name, batch=4, plan="train", flat=True, frozen=True))
    for env in SWITCHES:
        for name, B in SWITCH_MODELS:
            cells.append(dict(model=name, batch=B, plan="infer", env=env))
            cells.append(dict(model=name, batch=B, plan="train", flat=True, env=env))
    return cells


def cell_name(c):
    s = f"{c['plan']}/{c['model']}/B{c['batch']}"
    if c["plan"] == "train":
        s += f"/p{c.get('p_drop', 0.0):g}/dx{int(c.get('want_dx', False))}/{'flat' if c.get('flat') else 'separate'}"
        if c.get("frozen"):
            s += "/frozen"
    if c.get("env"):
        s += "/" + c["env"].replace(" ", ",")
    return s


class Resolver:
    """Pointer -> "owner+offset".  Named owners (parameters, gradients, the arena) are fixed; plan buffers get their number when
    a pointer into them is first printed."""

    def __init__(self, plan, model):
        import torch
        self.named, self.bufs, self.by_ptr, self.number = [], {}, {}, {}
        for k, p in model.named_parameters():
            self.named.append((p.data_ptr(), p.numel() * 4, "param:" + k))
            if p.grad is not None:
                self.named.append((p.grad.data_ptr(), p.grad.numel() * 4, "grad:" + k))
        arena = getattr(plan, "arena", None)
        if arena is not None:
            self.named.append((arena.data_ptr(), arena.numel() * 4, "arena"))
        self.named.sort()
        for t in plan.keep:
            if isinstance(t, torch.Tensor) and t.numel():
                st = t.untyped_storage()
                self.bufs[st.data_ptr()] = st.nbytes()
                self.by_ptr.setdefault(t.data_ptr(), t)
        self.starts = sorted(self.bufs)
        self.named_starts = [n[0] for n in self.named]

    def __call__(self, ptr):
        if not ptr:
            return "0"
        i = bisect.bisect_right(self.named_starts, ptr) - 1
        if i >= 0 and ptr < self.named[i][0] + self.named[i][1]:
            return f"{self.named[i][2]}+{ptr - self.named[i][0]}"
        i = bisect.bisect_right(self.starts, ptr) - 1
        if i >= 0 and ptr < self.starts[i] + self.bufs[self.starts[i]]:
            start = self.starts[i]
            n = self.number.setdefault(start, len(self.number))
            return f"buf{n}({self.bufs[start]})+{ptr - start}"
        raise SystemExit(f"plan_dump: pointer {ptr:#x} resolves to no parameter, gradient or plan buffer")

    def table(self, ptr, ctype, count):
        """The `count` elements of `ctype` a plan tensor holds at `ptr` (a job table uploaded at build time)."""
        t = self.by_ptr.get(ptr)
        if t is None:
            raise SystemExit(f"plan_dump: job table at {ptr:#x} is not a plan tensor")
        raw = t.cpu().contiguous().numpy().tobytes()
        return (ctype * count).from_buffer_copy(raw[:ctypes.sizeof(ctype) * count])


def fields(st, res, skip=()):
    out = []
    for name, ctype in st._fields_:
        if name not in skip:
            v = getattr(st, name)
            out.append(f"{name}={res(v) if ctype is ctypes.c_void_p else repr(v)}")
    return " ".join(out)


def dump_ops(label, ops, res, _lib, lines):
    names = {v: k for k, v in vars(_lib).items() if k.startswith("OP_") and k != "OP_MAX" and isinstance(v, int)}
    for i, (code, st) in enumerate(ops):
        lines.append(f"{label}[{i}] {names[code]} {fields(st, res)}")
        if code == _lib.OP_PACK_BATCH:
            for j, job in enumerate(res.table(st.jobs, _lib.PackArgs, st.njobs)):
                lines.append(f"  job[{j}] {fields(job, res)}")
            b0 = res.table(st.block0, ctypes.c_int32, st.njobs + 1)
            lines.append("  block0 " + " ".join(str(v) for v in b0))
        elif code == _lib.OP_LINEAR_BWD_BATCH:
            for j, job in enumerate(res.table(st.jobs, _lib.LinearBwdArgs, st.njobs)):
                lines.append(f"  job[{j}] {fields(job, res)}")


def dump_cell(tree, c):
    """(text, counts) of one cell; `tree` must already be first on sys.path."""
    import torch
    from anoddpm_amd import _lib, train_plan
    from anoddpm_amd.training import FlatBuffers
    from anoddpm_amd.unet import UNetModel, _Plan
    saved = dict(os.environ)
    for kv in (c.get("env") or "").split():
        k, v = kv.split("=")
        os.environ[k] = v
    try:
        torch.manual_seed(0)
        kw = cases(tree)[c["model"]]
        model = UNetModel(**kw)
        B, S, dev = c["batch"], kw["img_size"], torch.device("cpu")
        lines = [cell_name(c)]
        if c["plan"] == "infer":
            plan = _Plan(model, B, S, dev)
            res = Resolver(plan, model)
            dump_ops("ops", plan.ops, res, _lib, lines)
            for i, (key, st) in enumerate(plan._pack_jobs):       # refresh_weights fills in w: the address of parameter `key`
                lines.append(f"pack_job[{i}] {key} {fields(st, res, skip=('w',))}")
            for i, (key, dst, N, K) in enumerate(plan._bf16_jobs):
                lines.append(f"bf16_job[{i}] {key} {res(dst.data_ptr())} N={N} K={K}")
            lines.append(f"csum_mode={plan.csum_mode} csum_used={plan._csum_used} arith={plan.arith}")
            counts = f"ops={len(plan.ops)}"
        else:
            if not train_plan.eligible(model, B, S):
                raise SystemExit(f"plan_dump: {cell_name(c)} is outside the training plan (train_plan.eligible)")
            if c.get("frozen"):
                for k, p in model.named_parameters():
                    p.requires_grad_(not k.startswith(FROZEN_PREFIX))
            flat = FlatBuffers(model) if c.get("flat") else None      # (alive until the dump is written)
            plan = train_plan.TrainPlan(model, B, S, dev, want_dx=c.get("want_dx", False), p_drop=c.get("p_drop", 0.0))
            res = Resolver(plan, model)
            dump_ops("pack", plan.pack_ops, res, _lib, lines)
            dump_ops("fwd", plan.fwd_list, res, _lib, lines)
            dump_ops("bwd", plan.bops, res, _lib, lines)
            lines.append(f"drop_ops={[(i, b is not None) for _, b, i in plan._drop_ops]} p_drop={plan.p_drop} csum_mode={plan.csum_mode}")
            for end, keys in plan.bwd_marks:
                lines.append(f"bwd_mark {end} {' '.join(keys)}")
            counts = f"pack={len(plan.pack_ops)} fwd={len(plan.fwd_list)} bwd={len(plan.bops)}"
            del flat
        for e in plan.igemm_log:
            lines.append("igemm_log " + " ".join(f"{k}={e[k]!r}" for k in sorted(e)))
        for e in getattr(plan, "attention_log", []):
            lines.append("attention_log " + " ".join(f"{k}={e[k]!r}" for k in sorted(e)))
        lines.append(f"igemm_flops={plan.igemm_flops!r}")
        for k, (buf, C, H) in plan.block_out.items():
            lines.append(f"block_out {k} {res(buf.data_ptr())} C={C} H={H} numel={buf.numel()}")
        lines.append(f"y {res(plan.y.data_ptr())} temb {res(plan.temb.data_ptr())}")
        return "\n".join(lines) + "\n", counts
    finally:
        os.environ.clear()
        os.environ.update(saved)


def run_cell(arg):
    tree, c = arg
    if sys.path[0] != tree:
        sys.path.insert(0, tree)
    import torch
    torch.set_num_threads(1)
    text, counts = dump_cell(tree, c)
    return cell_name(c), text, counts


def compare(a, b):
    """Join two --matrix summaries cell by cell; returns the process exit status."""
    la, lb = ([ln.split("  ") for ln in open(f).read().splitlines()] for f in (a, b))
    if [x[0] for x in la] != [x[0] for x in lb]:
        raise SystemExit("plan_dump --compare: the two summaries do not list the same cells")
    same = 0
    for x, y in zip(la, lb):
        eq = x[1:] == y[1:]
        same += eq
        print(f"{x[0]}  {x[1]}  {x[2].replace('sha256=', 'first=')}  {y[2].replace('sha256=', 'second=')}  {'identical' if eq else 'DIFFERENT: ' + y[1]}")
    print(f"# {len(la)} cells, {same} identical, {len(la) - same} different")
    return 0 if same == len(la) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="checkout whose anoddpm_amd package is dumped (library built)")
    ap.add_argument("--matrix", action="store_true", help="one summary line per cell of the whole matrix")
    ap.add_argument("--only", default="", help="with --matrix: only the cells whose name contains this")
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--dump-dir", default="", help="with --matrix: also write every cell's full dump there")
    ap.add_argument("--model", default="i32_b32_h1")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--plan", default="infer", choices=["infer", "train"])
    ap.add_argument("--p-drop", type=float, default=0.0)
    ap.add_argument("--want-dx", action="store_true")
    ap.add_argument("--flat", action="store_true", help="parameters homed in training.FlatBuffers")
    ap.add_argument("--frozen", action="store_true", help=f"freeze the parameters under {FROZEN_PREFIX}")
    ap.add_argument("--env", default="", help='environment switches for the build, e.g. "ANODDPM_CSUM=1"')
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="join two --matrix outputs; exit 1 unless all cells are identical")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    tree = os.path.abspath(a.tree)
    if not a.matrix:
        c = dict(model=a.model, batch=a.batch, plan=a.plan, p_drop=a.p_drop, want_dx=a.want_dx, flat=a.flat, frozen=a.frozen, env=a.env)
        name, text, counts = run_cell((tree, c))
        sys.stdout.write(text)
        return
    cells = [c for c in matrix(tree) if a.only in cell_name(c)]
    if a.jobs > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(a.jobs, maxtasksperchild=8) as pool:
            results = pool.map(run_cell, [(tree, c) for c in cells], chunksize=1)
    else:
        results = [run_cell((tree, c)) for c in cells]
    for name, text, counts in results:
        if a.dump_dir:
            os.makedirs(a.dump_dir, exist_ok=True)
            with open(os.path.join(a.dump_dir, name.replace("/", "__").replace("=", "-") + ".txt"), "w") as f:
                f.write(text)
        print(f"{name}  {counts}  sha256={hashlib.sha256(text.encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
