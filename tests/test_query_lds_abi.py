"""MIRT_QUERY_LDS without a device: the constant through every layer, the wrappers' `lds` keyword, the plans of the three LDS query
families (host/plan_check on tests/golden/query_lds_plan_cases_v1.txt, checked against the formula restated here, not against recorded
output), and the preconditions of tests/test_gpu_query_lds.py -- which worlds have which layout, and that the ray sets reach what they
are meant to reach."""
import inspect
import re
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import weekend_raytracer_wgpu_amd as m
from weekend_raytracer_wgpu_amd import _abi, raytracer
import grid_rounding as gr
import query_lds_worlds as qw
import ray_query_ref as rq

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "weekend-raytracer-wgpu_amd" / "host"
LIB = ROOT / "weekend-raytracer-wgpu_amd" / "csrc" / "libmirt.so"
CASES = ROOT / "tests" / "golden" / "query_lds_plan_cases_v1.txt"
HEADER = (ROOT / "include" / "mirt.h").read_text()
BIT = 1 << 8


# ---- 1. the layers ----

def _enums():
    """Every anonymous enum of the header: a list of {name: value}."""
    out = []
    text = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        names = {}
        for item in body.split(","):
            mt = re.fullmatch(r"\s*(MIRT_\w+)\s*=\s*(-?\d+)u?\s*(?:<<\s*(\d+))?\s*", item)       # 1u << 8 and plain numbers
            if mt:
                names[mt.group(1)] = int(mt.group(2)) << int(mt.group(3) or 0)
        if names:
            out.append(names)
    return out


def test_the_constant_is_the_same_in_every_layer_and_sits_in_an_enum_of_its_own():
    own = [e for e in _enums() if "MIRT_QUERY_LDS" in e]
    assert own == [{"MIRT_QUERY_LDS": BIT}]
    assert _abi.MIRT_QUERY_LDS == m.MIRT_QUERY_LDS == BIT
    crate = (ROOT / "rust" / "mirt-sys" / "src" / "lib.rs").read_text()
    assert re.search(r"pub const MIRT_QUERY_LDS: u32 = 1 << 8;", crate)
    mirror = (HOST / "mirt_host.hpp").read_text()
    assert re.search(r"kQueryLds = MIRT_QUERY_LDS;\s*static_assert\(kQueryLds == 1u << 8", mirror)


def test_the_family_enums_and_the_version_are_unchanged():
    names = {}
    for e in _enums():
        names.update(e)
    rays = {k: v for k, v in names.items() if k.startswith("MIRT_RAYS_")}
    feats = {k: v for k, v in names.items() if k.startswith("MIRT_FEATURES_")}
    radiance = {k: v for k, v in names.items() if k.startswith("MIRT_RADIANCE_")}
    assert rays == {"MIRT_RAYS_FLAT": 1, "MIRT_RAYS_ANY_HIT": 2, "MIRT_RAYS_COUNT": 4, "MIRT_RAYS_SORT": 16}
    assert feats == {"MIRT_FEATURES_FLAT": 1}
    assert radiance == {"MIRT_RADIANCE_FLAT": 1, "MIRT_RADIANCE_ACCUMULATE": 2, "MIRT_RADIANCE_SKY_HOSEK": 4, "MIRT_RADIANCE_SORT": 16, "MIRT_RADIANCE_POOL": 64}
    assert not any(v & BIT for v in {**rays, **feats, **radiance}.values())
    assert not [k for k in names if re.match(r"MIRT_(FLAG|MODE)_\w*LDS", k)]
    assert m.lib().mirt_version() == (0 << 16 | 4 << 8 | 0)


class _NoLibrary:
    """A context whose handle must never be used: any attribute the wrappers would pass to the library fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper went on to use .{name} with an lds that is no bool")


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, m.MIRT_QUERY_LDS])
def test_the_wrappers_refuse_an_lds_that_is_no_bool(bad):
    ctx = m.Context.__new__(m.Context)
    ctx._h = None                                   # (mirt_ctx_* with a null context would answer MIRT_ERR_NULL_POINTER, a MirtError)
    rays = m.make_rays(np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32), 1000.0)
    rrays = m.make_radiance_rays(np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32), np.arange(2))
    p = m.make_params(8, 4, 0, mode=m.MIRT_MODE_PT)
    calls = [lambda: ctx.trace_rays(rays, lds=bad), lambda: ctx.trace_rays_device(16, 2, 16, lds=bad),
             lambda: ctx.render_features(p, lds=bad), lambda: ctx.render_features_device(p, 16, 1024, lds=bad),
             lambda: ctx.trace_radiance(rrays, 4, lds=bad), lambda: ctx.trace_radiance_device(16, 2, 16, 4, lds=bad)]
    cam = m.GpuCamera.new(m.scenes.three_spheres()[1], (8, 4)).c
    owner = _NoLibrary()
    calls += [lambda: raytracer._pick(owner, 1, 1, 8, 4, cam, None, bad), lambda: raytracer._features(owner, 0, 0, 8, 4, cam, None, bad),
              lambda: raytracer._radiance(owner, rrays, 4, 0, 8, False, None, False, False, bad)]
    for call in calls:
        with pytest.raises(ValueError, match="lds must be a bool"):
            call()


def test_every_query_method_has_the_keyword_and_the_default_is_off():
    for cls, names in ((m.Context, ("trace_rays", "trace_rays_device", "render_features", "render_features_device", "trace_radiance", "trace_radiance_device")),
                       (m.Layer, ("pick", "features", "radiance")), (m.Raytracer, ("pick", "features", "radiance"))):
        for name in names:
            par = inspect.signature(getattr(cls, name)).parameters
            assert "lds" in par and par["lds"].default is False, (cls.__name__, name)


# ---- 2. the plans ----

def _plan_check(mode):
    subprocess.run(["make", "-C", str(HOST), "plan_check"], check=True, capture_output=True)
    r = subprocess.run([str(HOST / "plan_check"), mode, str(CASES)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@lru_cache(maxsize=None)
def _cases():
    """[(name, {key: value})] of the case file, numbers as integers (qf: hexadecimal)."""
    out = []
    for line in CASES.read_text().splitlines():
        line = line.split("#")[0].strip()
        if not line:
            continue
        kv = dict(w.split("=", 1) for w in line.split())
        out.append((kv.pop("name"), kv))
    return out


CAMERA, SKY, SPHERE, MATERIAL = 96, 144, 32, 48        # sizeof MirtGpuCamera, MirtSkyState, PreparedSphere, PreparedMaterial
BUDGET = 120 * 1024                                    # kMaxLdsBytes


def _layout(ns, nm, gb, hosek, ldscu):
    """mirt_adapt_lds_plan restated: (block bytes, blocks per CU) or None."""
    tables = gb if gb else ns * SPHERE + nm * MATERIAL
    if CAMERA + SKY + tables > BUDGET or (gb and ns > 4095):
        return None
    block = CAMERA + (SKY if hosek else 0) + tables
    per_cu = ldscu // block
    return (block, min(per_cu, 8)) if per_cu else None


def _expect(kv):
    """What the header's MIRT_QUERY_LDS section says a case plans: None for a refusal, else (family, name, threads, lds, blocks)."""
    g = lambda k, d=0: int(kv.get(k, d))
    q, qf = kv["q"], int(kv.get("qf", "0"), 16)
    assert qf & BIT and not g("hbm")
    flat_bit = bool(qf & 1)
    hosek = q == "radiance" and bool(qf & 4)
    lay, grid = None, False
    if g("gb") and not flat_bit:
        lay, grid = _layout(g("ns"), g("nm"), g("gb"), hosek, g("ldscu")), True
        if lay and lay[0] > g("ldsblk"):
            lay = None
    if lay is None and g("flat"):
        lay, grid = _layout(g("ns"), g("nm"), 0, hosek, g("ldscu")), False
        if lay and lay[0] > g("ldsblk"):
            lay = None
    if lay is None:
        return None
    if q == "features":
        p = m.make_params(g("w"), g("h"), g("spp"), mode=g("mode"), row_begin=g("rb"), row_end=g("re"), tile_rows=g("tr"), n_parts=g("np"), part=g("part"))
        items = m.params_out_rows(p) * g("w")
    else:
        items = g("n")
    per_cu = max(1, min(g("res"), lay[1]))
    blocks = min(-(-items // 256), g("cu") * per_cu)
    if g("t.query_lds_blocks"):
        blocks = min(blocks, g("t.query_lds_blocks"))
    tf = ("false", "true")
    name = {"trace": f"trace_rays_lds_kernel<{tf[grid]},{tf[bool(qf & 2)]},{tf[bool(qf & 4)]}>", "features": f"feature_frame_lds_kernel<{tf[grid]}>",
            "radiance": f"radiance_rays_lds_kernel<{tf[hosek]},{tf[grid]}>"}[q]
    return q + "-lds", name, 256, lay[0], blocks


def _lds_cases():
    return [(n, kv) for n, kv in _cases() if not int(kv.get("hbm", 0))]


def test_the_plans_follow_the_formula():
    lines = {l.split(" ", 1)[0]: l for l in _plan_check("--queries")}
    names = {l.split(" ", 1)[0]: l for l in _plan_check("--query-kernels")}
    seen = {"grid": 0, "flat": 0, "refused": 0, "capped by the knob": 0, "occupancy below the bound": 0, "occupancy above the bound": 0}
    for case, kv in _lds_cases():
        want, line = _expect(kv), lines[case]
        if want is None:
            assert line.startswith(f"{case} status={_abi.MIRT_ERR_SCENE_TOO_LARGE} ") and names[case].startswith(f"{case} status="), line
            seen["refused"] += 1
            continue
        family, kernel, threads, lds, blocks = want
        got = dict(w.split("=", 1) for w in line.split()[2:])
        assert line.split()[1] == family and got["geo"] == f"{threads}/0/0" and int(got["lds"]) == lds and int(got["blocks"]) == blocks, (line, want)
        assert got["bse"] == "0" and got["row"] == "0" and got["id"][3] == "0", f"{line}: no tree, no sorted launch"
        reported, selected, symbol = names[case].split(" ")[1:4]
        assert reported == kernel == selected and symbol != "-", (names[case], kernel)
        seen["grid" if ",true>" in kernel.replace("<true>", ",true>") and got["id"][5] == "1" else "flat"] += 1
        bound = int(got["cap"].split("/")[1])
        res = int(kv.get("res", 0))
        seen["capped by the knob"] += "t.query_lds_blocks" in kv and blocks == int(kv["t.query_lds_blocks"])
        seen["occupancy below the bound"] += 0 < res < bound
        seen["occupancy above the bound"] += res > bound
    assert all(v >= 3 for v in seen.values()), seen
    # the _FLAT bit on a grid-only scene is refused, in every family
    for q in ("trace", "features", "radiance"):
        assert lines[f"{q}-lds-4000-flatbit-refused"].split(" ")[1] == f"status={_abi.MIRT_ERR_SCENE_TOO_LARGE}"
        assert " id=0000010 " in lines[f"{q}-lds-4000-grid"] and lines[f"{q}-lds-4000-grid"].endswith("cap=256/1/0")


def test_an_hbm_scene_ignores_the_flag():
    plans = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in _plan_check("--queries")}
    names = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in _plan_check("--query-kernels")}
    pairs = [("trace-hbm-flag", "trace-hbm-noflag"), ("features-hbm-flag", "features-hbm-noflag"), ("radiance-hbm-flag", "radiance-hbm-noflag"),
             ("radiance-hbm-flag-pool", "radiance-hbm-noflag-pool")]
    for a, b in pairs:
        assert plans[a] == plans[b] and names[a] == names[b] and "_lds_" not in names[a], (a, plans[a], names[a])
    assert names["trace-hbm-flag-sort-any"].startswith("trace_rays_sorted_kernel<true,true,false> ")


def test_every_new_kernel_of_the_library_is_some_cases_kernel():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], check=True, capture_output=True, text=True).stdout
    kernels = ("trace_rays_lds_kernelI", "feature_frame_lds_kernelI", "radiance_rays_lds_kernelI")
    handles = {sym for _, kind, sym in (l.split() for l in nm.splitlines())
               if kind == "V" and "__device_stub__" not in sym and any(f"exact_build{len(k) - 1}{k}" in sym for k in kernels)}
    assert len(handles) == 14
    selected = {l.split(" ")[3] for l in _plan_check("--query-kernels") if not l.split(" ")[1].startswith("status=") and "_lds_kernel<" in l.split(" ")[1]
                and not l.split(" ")[1].startswith("adapt")}
    assert selected == handles, (sorted(handles - selected)[:3], sorted(selected - handles)[:3])


# ---- 3. the preconditions of the GPU worlds ----

def test_which_worlds_have_which_layout():
    for name, (_, grid, flat) in qw.WORLDS.items():
        sd = qw.world(name)
        plan = gr.grid_plan(sd)
        n, nm = len(sd.spheres), len(sd.materials)
        fits = CAMERA + SKY + n * SPHERE + nm * MATERIAL <= BUDGET
        print(f"{name}: {n} spheres, blob {plan.blob_bytes} bytes, flat tables {'fit' if fits else 'do not fit'}")
        assert (plan.blob_bytes != 0) == grid and fits == flat, name
        if grid:
            assert CAMERA + SKY + plan.blob_bytes <= BUDGET and n <= 4095, name
    big = gr.grid_plan(qw.world("field 4000"))
    assert big.blob_bytes > 80 * 1024 and 163840 // (CAMERA + big.blob_bytes) == 1          # one block per CU
    assert len(qw.world("main.rs").spheres) == 5


def test_the_long_t_rays_hit_beyond_the_renderers_max_t():
    for name in ("field 484", "main.rs", "fixture"):
        inf = qw.reference(name, "long t", np.inf)
        hit = inf["sphere"] != rq.MISS
        assert hit.sum() >= 32 and (inf["t"][hit] > 1000.0).sum() >= 32, name
        at_1000 = qw.reference(name, "long t", 1000.0)
        assert (at_1000["sphere"] == rq.MISS)[inf["t"] > 1000.0].all()
        o, d, _ = qw.ray_sets(name)["long t"]
        assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1e-3, rtol=1e-5)


def test_the_adversarial_rays_meet_ties_on_equal_f():
    f = qw.roots("copies", "aimed")
    best = f.min(1)
    ties = (np.isfinite(best) & ((f == best[:, None]).sum(1) >= 2)).sum()
    assert ties >= 16, ties
    # ... and the far origins of the aimed sets lie beyond the guard of their grids (hundreds of units from a field a few units wide)
    o, _ = qw.aimed_rays("far origins")
    assert (np.linalg.norm(o - qw._eye("far origins"), axis=1) > 200.0).sum() >= 32
