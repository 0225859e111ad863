#!/usr/bin/env python3
"""ISA mix of the path-traced mode's routines on gfx950, from the compiler's assembly (no GPU needed).

mirt_kernels.hip holds, under -DMIRT_ISA_PROBES, one small kernel per routine around a common load / store frame
(probe_frame = the frame alone).  This tool compiles that build to assembly, counts the instructions of every probe by
class, subtracts the frame and writes profiles/<tag>_isa_mix.md: what a routine costs one wave per execution, and --
weighted with how often a sample runs each routine on config 3 (work counters) -- where the instructions of a sample go.

    python tools/isa_mix.py [tag] [--extra=-DMIRT_X]      (--extra: more compiler flags, e.g. -DMIRT_CHECKER_SIGN_FULL)
"""
import collections
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "weekend-raytracer-wgpu_amd" / "csrc"
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-fast-math -fno-slp-vectorize -DMIRT_ISA_PROBES").split()

FP = re.compile(r"^v_(add|sub|subrev|mul|fma|fmac|fmaak|fmamk|mac|mad|max|min|max3|min3|med3|ldexp|fract|floor|trunc|rndne|div_\w+)_(f32|f64|legacy_f32)")
SLOW = re.compile(r"^v_(rcp|rsq|sqrt|sin|cos|exp|log)(_iflag)?_f32")
CVT = re.compile(r"^v_cvt_")
CMPSEL = re.compile(r"^v_(cmp|cmpx|cndmask)")
INT = re.compile(r"^v_(add|sub|subrev|addc|subb|mul|mad|lshl|lshr|ashr|and|or|xor|not|bfe|bfi|bcnt|mbcnt|ffb|alignbit|perm|min|max|add3|lshl_add|lshl_or|and_or|or3|xad|sad|add_lshl|lshrrev|lshlrev|ashrrev|subbrev)(_co)?(_u32|_i32|_b32|_u16|_i16|_b16|_u32_u24|_i32_i24|_u64_u32|_i64_i32|_u24|_i24|_b64|_u64|_lo_u32|_hi_u32|_lo_i32|_hi_i32|_u32_b32|_i32_b32)?")


def classify(op: str) -> str:
    if op.startswith("v_"):
        if SLOW.match(op):
            return "valu_seed"          # quarter-rate hardware seeds: v_rcp / v_rsq / v_sqrt
        if FP.match(op):
            return "valu_fp"
        if CMPSEL.match(op):
            return "valu_cmp_select"
        if CVT.match(op):
            return "valu_convert"
        if op.startswith(("v_mov", "v_readlane", "v_readfirstlane", "v_writelane", "v_swap", "v_accvgpr", "v_nop")):
            return "valu_move"
        return "valu_int"               # integer / logic: RNG hashing, bit tricks, indexing
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
        return "branch"
    if op.startswith(("s_nop", "s_waitcnt", "s_barrier", "s_sleep", "s_endpgm", "s_set", "s_code_end")):
        return "wait_nop"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return "other"


COLS = ["valu_fp", "valu_seed", "valu_int", "valu_cmp_select", "valu_convert", "valu_move", "salu", "branch", "lds", "vmem", "smem", "wait_nop"]


def main() -> int:
    extra = [f for a in sys.argv[1:] if a.startswith("--extra=") for f in a[len("--extra="):].split()]
    sys.argv = [a for a in sys.argv if not a.startswith("--extra=")]
    if len(sys.argv) > 1 and sys.argv[1].startswith("-"):
        print("usage: tools/isa_mix.py [TAG] [--extra=FLAGS]   -> profiles/TAG_isa_mix.md (static instruction mix of the probe kernels; builds them first)")
        return 0
    tag = sys.argv[1] if len(sys.argv) > 1 else "r02"
    out = CSRC / "build" / "probes"
    out.mkdir(parents=True, exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-save-temps=obj", "-c", "mirt_kernels.hip", "-o", str(out / "k.o")], cwd=CSRC, check=True,
                   capture_output=True)
    asm = (out / "mirt_kernels-hip-amdgcn-amd-amdhsa-gfx950.s").read_text().splitlines()
    counts: dict = {}
    cur = None
    for ln in asm:
        m = re.match(r"^_ZN4mirt11exact_build(\d+)(probe_\w+?)ENS_10RenderArgs", ln)
        if m and ln.rstrip().endswith(":") or (m and ":" in ln):
            name = m.group(2)[: int(m.group(1))]
            cur = counts.setdefault(name, collections.Counter())
            continue
        if cur is None:
            continue
        t = ln.strip()
        if t.startswith("s_endpgm"):
            cur["wait_nop"] += 1
            cur = None
            continue
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        cur[classify(t.split()[0])] += 1
    frame = counts.pop("probe_frame")
    rows = []
    for name, c in counts.items():
        net = {k: c.get(k, 0) - frame.get(k, 0) for k in COLS}
        net["valu"] = sum(net[k] for k in COLS if k.startswith("valu"))
        rows.append((name.replace("probe_", ""), net))
    # how often one sample of config 3 runs each routine (oracle / kernel work counters)
    per_sample = {"generate_primary": 1.0, "sky_and_accumulate": 0.996, "nearest_hit_3_spheres": 2.062, "shade_checkerboard": 0.674,
                  "shade_metal": 0.251, "shade_dielectric": 0.140, "hit_normal": 1.066}
    lines = [f"# ISA mix of the path-traced routines (exact build, gfx950) — {tag}", "",
             "Static instruction counts of ONE execution by one wave, from `tools/isa_mix.py` (probe kernels of",
             "`mirt_kernels.hip` under `-DMIRT_ISA_PROBES`, common load/store frame subtracted; rare out-of-line paths —",
             "IEEE fallbacks of sqrt/rcp, full texture lookup, grazing directions — are counted although they almost never run,",
             "so the figures are upper bounds of what a step executes).  `valu_seed` = quarter-rate `v_rcp/v_rsq/v_sqrt`;",
             "`valu_int` = integer and logic operations: the RNG's hashing, bit tricks of the elementary functions, indexing.", "",
             "| routine | VALU | fp | seed | int/logic | cmp+select | convert | move | SALU | branch | LDS | wait/nop |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    total = collections.Counter()
    for name, n in rows:
        lines.append(f"| `{name}` | {n['valu']} | {n['valu_fp']} | {n['valu_seed']} | {n['valu_int']} | {n['valu_cmp_select']} | {n['valu_convert']} | "
                     f"{n['valu_move']} | {n['salu']} | {n['branch']} | {n['lds']} | {n['wait_nop']} |")
        w = per_sample.get(name, 0.0)
        for k, v in n.items():
            total[k] += w * v
    lines += ["", "Weighted with how often a sample of config 3 runs each routine (generate 1.0, sky 0.996, trace 2.062, checkerboard 0.674,",
              "metal 0.251, glass 0.140, hit normal 1.066 per sample; lane use 0.92):", "",
              f"* routines alone: **{total['valu'] / 0.92:.0f} VALU per 64 samples** (fp {total['valu_fp'] / 0.92:.0f}, seeds {total['valu_seed'] / 0.92:.0f}, "
              f"int/logic {total['valu_int'] / 0.92:.0f}, compare+select {total['valu_cmp_select'] / 0.92:.0f}, convert {total['valu_convert'] / 0.92:.0f}, "
              f"moves {total['valu_move'] / 0.92:.0f});",
              "* measured (`SQ_INSTS_VALU`, `profiles/r02f_c3_pmc_summary.json`): 664 VALU per 64 samples — the difference is the pool's own work",
              "  (pick, pop, gather, unpack, pack, store, push: about 65 VALU per step that is not fast-forwarded) minus the out-of-line paths",
              "  that the static counts include;",
              "* algorithmic floating-point operations (SURVEY §8d): 284.6 flop per sample, i.e. between 142 (all fused) and 285 (none fused) fp",
              f"  instructions; executed: {total['valu_fp'] / 0.92:.0f} fp instructions per 64 samples.  The surplus is the polynomial elementary functions",
              "  (sincos, pow, acos/atan2 on textured hits) and the correction steps of the correctly rounded sqrt / reciprocal -- what the",
              "  bit-exact arithmetic adds; the other 45 % of the VALU stream is integer hashing (RNG), compares / selects, conversions and moves."]
    (ROOT / "profiles" / f"{tag}_isa_mix.md").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
