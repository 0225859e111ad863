"""The plan of a query launch -- ray queries, feature frames, radiance queries, adaptive steps and runs (csrc/mirt_launch_plan.h: QueryPlan,
plan_trace / plan_features / plan_radiance / plan_adapt, query_plan_blocks, query_kernel_name) -- against what the four launch functions
of mirt_api.hip decided inline before the plan was split out of them, and the kernel the plan names against the one that is dispatched
(query_kernel).  No GPU: host/plan_check --queries / --query-kernels reads tests/golden/query_plan_cases_v1.txt, one case per line.

  query_plans_v1.txt      per case family, template bits, block size, LDS bytes, stack entries, units, blocks (plan_check's line format)
  query_kernels_v1.txt    per case the name mirt_ctx_last_kernel reports
                          both recorded from the library as it was while each launch function decided these between its HIP calls and the
                          name was a hand-kept mirror of nine ternary ladders (profiles/r23_query_plan.md says how)

The cases are the product that reaches every build -- trace x sorted x bvh x any x count; features x bvh; radiance x sorted x hosek x bvh;
radiance-pool and adapt-pool x the four slot choices x hosek x sorted / run; adapt x run x hosek x bvh; adapt-lds x run x hosek x grid -- and
the edges that decide a plan (the first word of a line in all three files):

  tree depth 0 / 1 / 20 / 32        trace-dep*, trace-flat-dep*, features-dep*, radiance-dep*, adapt-dep*; the pooled geometry by depth:
                                    radiance-pool-dep*-h*, adapt-pool-dep*-h*
  the pooled gate                   255 / 256 bounces: *-pool-nb255 / -nb256; the flat scan: radiance-pool-flat, adapt-pool-nogrid; no geometry
                                    beside a 32-deep tree in the block's LDS: *-pool-dep32-ldsblk* (falls back below 47 KB), in the CU's: *-ldscu40000
  counts                            1, 16, 17, 63 - 65, 255 - 257, 2^32 - 1 rays or pixels: trace-n*, radiance-n*, radiance-pool-n*, adapt-px*,
                                    adapt-pool-px*, adapt-lds-px*; feature frames with bands and parts: features-*x*
  the block caps                    below, at, above the uncapped grid: radiance-pool-cap15 / 16 / 17, adapt-pool-cap47 / 48 / 49, adapt-lds-cap11 / 12 /
                                    13, adapt-lds-1080p-cap1279 / 1280 / 1281; ignored without the pool: *-cap*-unpooled
  the LDS step's grid               the occupancy answer 0, below and above the layout's bound: adapt-lds-rtiow-1080p-res*, adapt-lds-three-1080p-res*;
                                    fewer pixels than one resident grid, and one more: adapt-lds-px393215-res6 .. px393217-res6; CUs: adapt-lds-cu*
  the LDS layouts                   NO_GRID: adapt-lds-nogrid; the grid beyond a block's LDS, flat tables that fit: adapt-lds-grid-beyond-block-h*; neither:
                                    adapt-lds-neither-refused, -neither-flat-refused, adapt-lds-nogrid-refused; 12-bit ids: adapt-lds-ids-4095 / -4096-refused;
                                    not one block per CU: adapt-lds-small-cu-lds; forced groups: adapt-lds-groups*
"""
import subprocess
from functools import lru_cache
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "weekend-raytracer-wgpu_amd" / "host"
LIB = ROOT / "weekend-raytracer-wgpu_amd" / "csrc" / "libmirt.so"
GOLDEN = ROOT / "tests" / "golden"
CASES = GOLDEN / "query_plan_cases_v1.txt"

# the query kernels of libmirt.so: the seven families' templates (the select and resolve stages of an adaptive step are no templates)
QUERY_KERNELS = ("trace_rays_kernelI", "trace_rays_sorted_kernelI", "feature_frame_kernelI", "radiance_rays_kernelI", "radiance_rays_sorted_kernelI",
                 "radiance_rays_pool_kernelI", "adapt_pixels_kernelI", "adapt_pixels_run_kernelI", "adapt_pixels_pool_kernelI", "adapt_pixels_pool_run_kernelI",
                 "adapt_pixels_lds_kernelI", "adapt_pixels_lds_run_kernelI")
# 16 trace + 2 features + 8 radiance + 16 pooled + 8 adapt + 16 pooled + 8 LDS
N_QUERY_KERNELS = 74


def plan_check(*args):
    # always through make (a no-op when up to date), as test_cpp_host.py does
    subprocess.run(["make", "-C", str(HOST), "plan_check"], check=True, capture_output=True)
    r = subprocess.run([str(HOST / "plan_check"), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def refused(line):
    return line.split(" ", 2)[1].startswith("status=")


@lru_cache(maxsize=None)
def kernels():
    """the lines of plan_check --query-kernels, and of the accepted cases the words: (case, reported name, selected instance, its symbol)"""
    lines = plan_check("--query-kernels", CASES)
    return lines, [tuple(l.split(" ")) for l in lines if not refused(l)]


def assert_same(got, want, what):
    assert len(want) >= 250 and len(got) == len(want)
    differ = [f"{g}\n   recorded: {w}" for g, w in zip(got, want) if g != w]
    assert not differ, f"{len(differ)} of {len(want)} {what} differ from the recorded ones; the first:\n" + "\n".join(differ[:5])


def test_query_plans_are_those_recorded_from_the_launch_functions():
    assert_same(plan_check("--queries", CASES), (GOLDEN / "query_plans_v1.txt").read_text().splitlines(), "plans")


def test_reported_names_are_those_recorded():
    lines, _ = kernels()
    got = [l if refused(l) else " ".join(l.split(" ")[:2]) for l in lines]
    assert_same(got, (GOLDEN / "query_kernels_v1.txt").read_text().splitlines(), "names")


def test_reported_name_is_the_instance_selected():
    # no padding rule: the demangler prints every template argument of these kernels and the names have always had them all
    _, accepted = kernels()
    assert len(accepted) >= 250
    none = [case for case, _, _, symbol in accepted if symbol == "-"]
    assert not none, f"query_kernel selects no instance for {none[:5]}"
    differ = [f"{case}: reported {name}, selected {instance}" for case, name, instance, _ in accepted if name != instance]
    assert not differ, f"{len(differ)} names are not the kernel dispatched; the first:\n" + "\n".join(differ[:5])


def test_every_query_kernel_of_the_library_is_some_plans_kernel():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], check=True, capture_output=True, text=True).stdout
    # a kernel's handle is an 8-byte object under the kernel's own mangled name (the host stub carries __device_stub__)
    handles = {sym for _, kind, sym in (l.split() for l in nm.splitlines())
               if kind == "V" and "__device_stub__" not in sym and any(f"exact_build{len(k) - 1}{k}" in sym for k in QUERY_KERNELS)}
    assert len(handles) == N_QUERY_KERNELS
    selected = {symbol for _, _, _, symbol in kernels()[1]}
    assert selected <= handles, f"not query kernel handles: {sorted(selected - handles)[:5]}"
    assert not handles - selected, f"kernels no case selects: {sorted(handles - selected)[:5]}"
