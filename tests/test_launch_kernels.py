"""The kernel of a launch plan: the name mirt_ctx_last_kernel reports (plan_kernel_name) and the template instance that is dispatched
(render_kernel of the plan's build) are the same thing, for every build the library carries.  No GPU: host/plan_check --kernels prints,
per case, the reported name and the instance render_kernel selects (the symbol of its kernel handle in libmirt.so, resolved with dladdr).

  launch_kernels_v1.txt / _v2.txt    the reported name of every case of launch_plan_cases_v1.txt / _v2.txt, recorded from the library as it was
                                     while the name was a hand-kept mirror of the dispatch (profiles/r22_one_kernel_selector.md)
  launch_plan_cases_v2.txt           cases chosen so that, with v1's, every render kernel of both builds is some case's kernel: every pool
                                     geometry x queue count x Hosek x frame and its counting build, the grid pool's four slot choices x flat-y,
                                     the pooled HBM kernel's four x counting x fast, and every strip, HBM and parity build
  launch_plans_v2.txt                their plans, recorded like v1's (test_launch_plan.py)
"""
import subprocess
from functools import lru_cache
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "weekend-raytracer-wgpu_amd" / "host"
LIB = ROOT / "weekend-raytracer-wgpu_amd" / "csrc" / "libmirt.so"
GOLDEN = ROOT / "tests" / "golden"
VERSIONS = ("v1", "v2")

# Kernel handles of libmirt.so that no case of v1 or v2 selects, each with its reason.  None: a new one is a build nothing can launch
# (or a case missing from v2), and one that has become reachable no longer belongs here.
UNREACHED = {}


def plan_check(*args):
    # always through make (a no-op when up to date), as test_cpp_host.py does
    subprocess.run(["make", "-C", str(HOST), "plan_check"], check=True, capture_output=True)
    r = subprocess.run([str(HOST / "plan_check"), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@lru_cache(maxsize=None)
def kernels(version):
    """the lines of plan_check --kernels, and of the accepted cases (a refused one prints its status) the words: (case, reported name,
    selected instance written as a reported name, its symbol)"""
    lines = plan_check("--kernels", GOLDEN / f"launch_plan_cases_{version}.txt")
    return lines, [tuple(l.split(" ")) for l in lines if not l.split(" ", 2)[1].startswith("status=")]


def with_defaults(reported):
    # the tile kernel's reported name has always stopped at GRID, seven arguments; the instance has FLATY = false behind it
    return reported[:-1] + ",false>" if "render_pt_pool_tile" in reported else reported


def test_v2_plans_are_those_recorded():
    got, want = plan_check(GOLDEN / "launch_plan_cases_v2.txt"), (GOLDEN / "launch_plans_v2.txt").read_text().splitlines()
    assert len(want) >= 300 and got == want


@pytest.mark.parametrize("version", VERSIONS)
def test_reported_names_are_those_recorded(version):
    lines, _ = kernels(version)
    got = [l if l.split(" ", 2)[1].startswith("status=") else " ".join(l.split(" ")[:2]) for l in lines]
    want = (GOLDEN / f"launch_kernels_{version}.txt").read_text().splitlines()
    assert len(want) >= 300 and len(got) == len(want)
    differ = [f"{g}\n   recorded: {w}" for g, w in zip(got, want) if g != w]
    assert not differ, f"{len(differ)} of {len(want)} names differ from the recorded ones; the first:\n" + "\n".join(differ[:5])


@pytest.mark.parametrize("version", VERSIONS)
def test_reported_name_is_the_instance_selected(version):
    _, accepted = kernels(version)
    assert len(accepted) >= 300
    none = [case for case, _, _, symbol in accepted if symbol == "-"]
    assert not none, f"render_kernel selects no instance for {none[:5]}"
    differ = [f"{case}: reported {name}, selected {instance}" for case, name, instance, _ in accepted if with_defaults(name) != instance]
    assert not differ, f"{len(differ)} names are not the kernel dispatched; the first:\n" + "\n".join(differ[:5])


def test_every_render_kernel_of_the_library_is_some_plans_kernel():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], check=True, capture_output=True, text=True).stdout
    # a kernel's handle is an 8-byte object under the kernel's own mangled name (the host stub carries __device_stub__)
    handles = {sym for _, kind, sym in (l.split() for l in nm.splitlines()) if kind == "V" and "render_" in sym and "_kernelI" in sym and "__device_stub__" not in sym}
    assert len(handles) >= 396
    selected = {symbol for version in VERSIONS for _, _, _, symbol in kernels(version)[1]}
    assert selected <= handles, f"not kernel handles: {sorted(selected - handles)[:5]}"
    unreached = handles - selected
    assert unreached == set(UNREACHED), (f"kernels no case selects, beyond the listed ones: {sorted(unreached - set(UNREACHED))[:5]}; "
                                         f"listed but selected: {sorted(set(UNREACHED) & selected)[:5]}")
    assert not [sym for sym in UNREACHED if "render_pt_pool" in sym], "every pool build must be reachable"
