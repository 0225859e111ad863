#!/usr/bin/env python3
"""Developer tool: what the node (mirt_node_*) costs on ONE GPU, in one process.  Config 3's scene, path traced, 8 spp.

    python tools/node_timing.py [--sizes 1920x1080,3840x2160] [--spp 8] [--frames 10] [--reps 300] [--parent-lib L.so]

Per size it reports
  - assemble_ms: the node's assembly kernel (its own hipEvents, mirt_node_get_stats), loopback N = 2, 4, 8 and forced-RCCL N = 1,
    with gather_ms of the latter;
  - mirt_ctx_deinterleave_device on the SAME 8 parts (stride form) with this library and, given --parent-lib, with a build of the
    parent commit (deinterleave_kernel): mean of --reps launches on one stream between two torch events, rotating over buffer
    sets of > 512 MiB in all (each call then moves its bytes through HBM, not the Infinity Cache), images compared;
  - wall ms per frame (host clock around blocking renders, after warm-up) of loopback N = 1, 2, 4, 8 against one context.
Loopback puts every member on one GPU: it exists to exercise the node path, no speed-up is expected.  The parent build:
    mkdir /tmp/parent && git archive HEAD~ | tar -x -C /tmp/parent
    make -C /tmp/parent/weekend-raytracer-wgpu_amd/csrc OUT=$PWD/tools/_scratch/libs/libmirt_parent.so OBJDIR=/tmp/parent/obj
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import torch  # noqa: E402
import weekend_raytracer_wgpu_amd as m  # noqa: E402
from weekend_raytracer_wgpu_amd import _abi  # noqa: E402
from helpers import scene_data  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--frames", type=int, default=10)
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()


def wall_ms(render, frames):
    render()                                        # warm-up (first launches, buffer growth)
    render()
    t0 = time.perf_counter()
    for _ in range(frames):
        render()
    return (time.perf_counter() - t0) * 1e3 / frames


def deinterleave_ms(lib, ctx, base, sets, stride, reps, stream):
    """Mean time of one mirt_ctx_deinterleave_device call on `stream` (torch events around `reps` calls).  The calls rotate over
    `sets` of (parts, out) buffers larger together than the 256 MiB Infinity Cache, so that each call reads and writes HBM."""
    p = m.multi_gpu.part_params(base, 0, 8, 4)

    def launch(k):
        parts, out = sets[k % len(sets)]
        rc = lib.mirt_ctx_deinterleave_device(ctx, C.byref(p), C.c_void_p(parts.data_ptr()), stride, C.c_void_p(out.data_ptr()),
                                              out.numel(), C.c_void_p(stream.cuda_stream))
        assert rc == 0, lib.mirt_last_error()
    for k in range(len(sets)):
        launch(k)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for k in range(reps):
        launch(k)
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


libs = [("this build (assemble_parts_kernel)", m.lib())]
if a.parent_lib:
    plib = C.CDLL(str(Path(a.parent_lib).resolve()))
    _abi.bind(plib, {k: v for k, v in _abi.SYMBOLS.items() if hasattr(plib, k)})
    libs.append(("parent (deinterleave_kernel)", plib))

print(f"node timing: config 3 scene (three spheres), path traced, {a.spp} spp, 8 bounces; {torch.cuda.get_device_name(0)}")
for size in a.sizes.split(","):
    w, h = map(int, size.split("x"))
    sd = scene_data("three_spheres", w, h)
    base = m.make_params(w, h, a.spp, mode=m.MIRT_MODE_PT, num_bounces=8)
    print(f"\n== {w} x {h}: {w * h * 4 / 1e6:.1f} MB per frame; an assembly reads and writes it once each")
    ctx = m.Context(0)
    ctx.set_scene(sd)
    want = ctx.render(base)

    # the node's assembly kernel (and the forced one-rank RCCL gather)
    for devices, rccl in (([0] * 2, False), ([0] * 4, False), ([0] * 8, False), ([0], True)):
        with m.Node(devices, rccl=rccl) as node:
            node.set_scene(sd)
            asm, gat = [], []
            for _ in range(max(3, a.frames)):
                got = node.render(base)
                st = node.stats()
                asm.append(st["assemble_ms"])
                gat.append(st["gather_ms"])
            assert np.array_equal(got, want), (devices, rccl)
            asm, gat = np.array(asm[2:]), np.array(gat[2:])
            what = f"{'RCCL' if rccl else 'loopback'} N={len(devices)}"
            extra = f"  gather_ms median {np.median(gat) * 1e3:8.1f} us" if rccl else ""
            print(f"  assemble_ms {what:<13} median {np.median(asm) * 1e3:8.1f} us  min {asm.min() * 1e3:8.1f} us "
                  f"(= {2 * w * h * 4 / (np.median(asm) * 1e-3) / 1e12:5.2f} TB/s){extra}")

    # mirt_ctx_deinterleave_device on the same 8 parts, each build, on a stream of this tool's own (not the default stream)
    world = 8
    max_rows = m.multi_gpu.max_part_rows(base, world, 4)
    stream = torch.cuda.Stream()
    parts = torch.zeros((world, max_rows, w, 4), dtype=torch.uint8, device="cuda")
    for r in range(world):
        pr = m.multi_gpu.part_params(base, r, world, 4)
        ctx.render_device(pr, parts[r].data_ptr(), m.params_out_rows(pr) * w * 4, stream.cuda_stream)
    torch.cuda.synchronize()
    n_sets = max(2, -(-(512 << 20) // (parts.numel() + w * h * 4)))
    sets = [(parts if k == 0 else parts.clone(), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")) for k in range(n_sets)]
    stride = max_rows * w * 4
    rounds = {name: [] for name, _ in libs}
    handles = {}
    for name, lib in libs:
        h_ = C.c_void_p()
        assert lib.mirt_ctx_create(0, C.byref(h_)) == 0, lib.mirt_last_error()
        handles[name] = h_
    for _ in range(3):                              # interleaved rounds: A, B, A, B, ...
        for name, lib in libs:
            for _, out in sets:
                out.zero_()
            torch.cuda.synchronize()
            rounds[name].append(deinterleave_ms(lib, handles[name], base, sets, stride, a.reps, stream))
            assert all(np.array_equal(out.cpu().numpy(), want) for _, out in sets), name
    for name, lib in libs:
        t = np.array(rounds[name])
        print(f"  mirt_ctx_deinterleave_device {name:<36} {np.median(t) * 1e3:8.1f} us per call (rounds "
              f"{', '.join('%.1f' % (x * 1e3) for x in t)}; {2 * w * h * 4 / (np.median(t) * 1e-3) / 1e12:5.2f} TB/s; "
              f"{n_sets} buffer sets in rotation)")
        lib.mirt_ctx_destroy(handles[name])
    del sets, parts

    # wall time per frame: one context against loopback nodes
    print(f"  wall ms per frame (blocking, host memory), {a.frames} frames:")
    print(f"    one context        {wall_ms(lambda: ctx.render(base), a.frames):8.3f}")
    for n in (1, 2, 4, 8):
        with m.Node([0] * n) as node:
            node.set_scene(sd)
            print(f"    loopback N={n:<7} {wall_ms(lambda: node.render(base), a.frames):8.3f}")
    ctx.close()
