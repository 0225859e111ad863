#!/usr/bin/env python3
"""Opcode-class census of the step loop of a pooled kernel on gfx950, from the compiler's assembly (no GPU needed).

    python tools/pool_step_census.py [--kernel 'render_pt_pool_kernelILj256ELj112ELj6ELb0ELb0ELj3ELb0ELb0EE'] [--extra=-DMIRT_X] [--asm FILE]

Runs `make asm` in csrc (with EXTRA, if given; --asm reads an assembly file that exists already), finds the kernel
whose mangled name contains --kernel inside the exact build's namespace, and counts its instructions by the classes of
tools/isa_mix.py, folded to VALU / SALU / branch / wait-nop / LDS / VMEM / SMEM -- for the whole kernel text and for the
STEP LOOP: the longest span from a label the compiler annotates "This Loop Header: Depth=2" (depth 1 is the strip loop) to the
last backward branch to it.  Blocks the compiler placed behind that back edge (rare out-of-line paths) are outside the
span.  The counts are static: what the text holds, not what a step executes.
"""
import argparse
import collections
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "weekend-raytracer-wgpu_amd" / "csrc"
sys.path.insert(0, str(Path(__file__).resolve().parent))
from isa_mix import classify  # noqa: E402

DEFAULT = "render_pt_pool_kernelILj256ELj112ELj6ELb0ELb0ELj3ELb0ELb0EE"
FOLD = {"salu": "SALU", "branch": "branch", "wait_nop": "wait/nop", "lds": "LDS", "vmem": "VMEM", "smem": "SMEM", "other": "other"}
COLS = ["VALU", "SALU", "branch", "wait/nop", "LDS", "VMEM", "SMEM"]
DETAIL = ["s_nop", "s_waitcnt", "s_cbranch_execz", "s_cbranch_execnz", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0", "s_cbranch_scc1",
          "s_branch", "s_and_saveexec_b64", "v_readfirstlane_b32", "v_cmp", "v_cndmask_b32"]         # opcode prefixes


def kernel_text(asm: list, needle: str):
    """(name, [(opcode, operands)] with labels as ('L', name)) of the first exact-build kernel whose name contains needle"""
    start = None
    for i, ln in enumerate(asm):
        m = re.match(r"^(_ZN4mirt11exact_build\S*):", ln)
        if m and needle in m.group(1):
            start, name = i, m.group(1)
            break
    if start is None:
        raise SystemExit(f"no kernel matching {needle!r} in the assembly")
    items = []
    for ln in asm[start + 1:]:
        t = ln.split(";")[0].strip()
        if not t and "This Loop Header: Depth=2" in ln and items and items[-1][0] == "L":
            items[-1] = ("L", items[-1][1], 2)              # the annotation follows its label
            continue
        if t.endswith(":"):
            items.append(("L", t[:-1]))
            continue
        if not t or t.startswith((".", "//")):
            continue
        op, _, rest = t.partition(" ")
        items.append((op, rest.strip()))
        if op == "s_endpgm":
            break
    return name, items


def census(items) -> dict:
    c = collections.Counter()
    for op, *_ in items:
        if op == "L":
            continue
        k = classify(op)
        c["VALU" if k.startswith("valu") else FOLD[k]] += 1
        c[op] += 1
    return c


def step_loop(items):
    """index range [a, b] of the longest depth-2 loop: its header .. the last backward branch to it"""
    label_at = {it[1]: i for i, it in enumerate(items) if it[0] == "L" and len(it) == 3}
    last_back = {}
    for i, it in enumerate(items):
        if it[0].startswith(("s_cbranch", "s_branch")) and it[1] in label_at and label_at[it[1]] < i:
            last_back[it[1]] = i
    if not last_back:
        raise SystemExit("no depth-2 loop found")
    return max(((label_at[n], e) for n, e in last_back.items()), key=lambda ab: ab[1] - ab[0])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default=DEFAULT)
    ap.add_argument("--extra", default="")
    ap.add_argument("--asm", default=None)
    a = ap.parse_args()
    if a.asm is None:
        subprocess.run(["make", "asm", f"EXTRA={a.extra}"], cwd=CSRC, check=True, capture_output=True)
        a.asm = CSRC / "build" / "mirt_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"
    name, items = kernel_text(Path(a.asm).read_text().splitlines(), a.kernel)
    lo, hi = step_loop(items)
    whole, loop = census(items), census(items[lo:hi + 1])
    print(f"kernel {name}")
    print(f"step loop: {items[lo][1]} .. its last back edge, {sum(1 for it in items[lo:hi + 1] if it[0] != 'L')} of "
          f"{sum(1 for it in items if it[0] != 'L')} instructions")
    print("| span | " + " | ".join(COLS) + " |")
    print("|---|" + "---|" * len(COLS))
    for tag, c in (("kernel", whole), ("step loop", loop)):
        print(f"| {tag} | " + " | ".join(str(c[k]) for k in COLS) + " |")
    by_prefix = {k: sum(n for op, n in loop.items() if op not in COLS and op.startswith(k)) for k in DETAIL}
    print("step loop, by opcode: " + ", ".join(f"{k} {n}" for k, n in by_prefix.items() if n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
