"""The launch plan of a render call (csrc/mirt_launch_plan.h: plan_render, plan_blocks) against the plans recorded from launch_render as it
was before the plan was split out of it.  No GPU: host/plan_check reads tests/golden/launch_plan_cases_v1.txt -- one case per line: the facts
of a context, the params, the tuning fields that differ from their defaults, the frame bit and the occupancy answer, as they were on an
MI355X -- and prints each plan; the output must be tests/golden/launch_plans_v1.txt byte for byte.  (Keys that are zero are left out of a case.)

The planner's branches and a case that takes each (the first word of a line in both files):

  mode                        parity: layer-parity--spp2; path-traced: three-spp2
  texel tiles                 image texture: earth-tiles-spp32 (cfg 5); none: three-tiles-spp32 (cfg 0); knob set: knob-pool_config=1-three-spp64
  stream_any_spp              >= 16*8*32*CUs pixels: single-1024x1024-spp800 (strip); below: single-1024x1023-spp800 (pool); Hosek sky:
                              single+sky-hosek-1024x1024-spp800; several routines: three-1024x1024-spp800
  pool_min_spp                32: three-spp31 / three-spp32; 800: single-1024x1023-spp799 / single-1024x1023-spp800; (600: single-spp599 /
                              single-spp600, no crossover any more); knob: knob-pool_min_spp=40-three-spp32 / -spp48
  KERNEL_STRIP / _POOL        three-strip-spp128; three-pool-spp4; both: hbm13-poolstrip-spp64
  per-frame stream            three-fspp2-spp64, three-fspp2-pool (never pooled), three-fspp2-count, rtiow-fspp2-count (flat scan)
  255 / 256 bounces           three-pool-nb255 / three-pool-nb256; rtiow-pool-nb255 / -nb256; hbm13-pool-nb255 / -nb256
  scene beyond the flat LDS   gridonly-spp2, gridonly-spp16 (strip, grid); gridonly-pool-spp16 (no pool geometry fits); the refusal:
                              gridonly-nogrid-refused, gridonly-count-refused
  grid_ok                     rtiow-spp8; COUNT_WORK alone: rtiow-count-spp128; with COUNT_GRID: rtiow-countgrid-spp128, gridonly-countgrid-spp16
                              (no counting geometry fits); NO_GRID: rtiow-nogrid-spp128
  pooled grid build           kPoolMinSppGrid: rtiow-spp15 / rtiow-spp16; forced: rtiow-pool-spp4; knobs: knob-pool_grid=0-rtiow-spp32,
                              knob-pool_config=1-rtiow-spp32, knob-pool_config=1-rtiow-pool-spp4; flat-y: rtiow-spp16 / knob-grid_flat_y=0-rtiow-spp32
  HBM scenes                  BVH: hbm13--spp2; flat scan: hbm13-nogrid-spp2, hbm13-count-spp2; counting BVH: hbm13-countgrid-spp2; parity:
                              hbm13-parity-spp2, hbm13-parity-count
  pooled HBM gate             hbm13-pool-spp64; _STRIP: hbm13-poolstrip-spp64; per-frame stream: hbm13-pool-fspp2; bounces: hbm13-pool-nb256; NO_GRID:
                              hbm13-poolnogrid-spp64; geometry by depth: hbm13 (112 slots), hbm20-pool-spp64, hbm-line22-pool-spp64, hbm-line24-pool-spp64,
                              hbm-line26-pool-spp64, hbm-stair28-pool-spp64, hbm32-pool-spp64; sky: hbm13+sky-hosekpool; knob:
                              knob-hbm_pool_slots=80-hbm13-pool; counting: hbm13-poolcountgrid-spp64; frame: hbm13-pool-frame; fast: hbm13-poolfast-spp64
  guided strips               min width 16 / 8 / 4 at spp 63 / 64, 127 / 128 (512 / min_width): three-spp63, three-spp64, three-spp127, three-spp128;
                              three-spp511 / three-spp512; knobs: knob-strip_mode=1-, knob-gss_minw=8-, knob-gss_keep=2.5-; a frame smaller than
                              the keep: three-96x64-spp64
  strip_cand                  rtiow-spp3 / rtiow-spp4; pooled: rtiow-spp16; knob-strip_cand=0-rtiow-spp8
  lane = pixel                below 64 spp: three-strip-spp32 / three-strip-spp128; one routine, 64*4*CUs pixels: single-256x255-spp100 /
                              single-256x256-spp100; counting: three-count-spp4; knobs: knob-by_pixel=0-, knob-by_pixel=1-; parity:
                              layer-parity--spp1000, layer-parity-strip-spp2, layer-parity-count-spp2
  streaming build             three-spp15 / three-spp16; grid: rtiow-spp8 (never); knobs: knob-stream=0-three-spp16, knob-stream=1-three-spp8
  pixel groups                shares of 4: three-spp4 / three-spp8; of 8 when streaming: three-spp16, three-spp24, three-spp31, three-strip-spp32 (four groups);
                              grid: rtiow-spp8, gridonly-spp16; odd: three-spp3, three-spp15; knobs: knob-px_groups=0-, knob-px_groups=3-
  one unit per wave           three-spp2 (64 threads), rtiow-spp3 / rtiow-spp4 (the dispenser from 4 spp on); knobs: knob-static_units=0-,
                              knob-static_units=1-, knob-static_block=128-, knob-static_grid=2-
  fast math                   three-fast-spp4, three-fast-spp128; counting runs the exact build: three-countfast-spp4; HBM: hbm13-fast-spp2
  Hosek sky                   three+sky-hosek-spp2, three+sky-hosek-spp32, rtiow+sky-hosek-spp32, three+sky-hosekcount-spp32
  the frame build             three-frame-spp2, three-frame-spp128, rtiow-frame-spp32, hbm13-frame; sums only: three-add-spp16
  parts and bands             three-parts-w640-part0 .. part3; a part with less than a strip: three-parts-w3-part2; with no row: three-parts-w3-part3;
                              three-band
  block count                 pool, LDS-bound: three-spp32; by units: three-96x64-spp64; knob-pool_blocks_per_cu=3-; pooled HBM, the occupancy answer:
                              hbm13-pool-spp64 (res 4), hbm32-pool-spp64; strip, resident grid: three-strip-spp128 (res 7), three-count-spp4; one unit per
                              wave: three-spp2; fewer than eight waves: three-parts-w3-part0.  (The strip kernels' cap of 8 blocks per CU: answers
                              above 8 were recorded only for launches with one unit per wave -- hbm13--spp2, res 19 --, where it decides nothing.)
  spread_units                pool below 128 spp: three-spp127 / three-spp128; knob-spread_units=0-rtiow-spp8
  pinhole word                single-spp2 (pinhole camera) / three-spp2 (lens); knob-pinhole=0-three-spp8; parity never: layer-parity--spp2
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "weekend-raytracer-wgpu_amd" / "host"
GOLDEN = ROOT / "tests" / "golden"


def test_plans_are_those_recorded_from_launch_render():
    # always through make (a no-op when up to date), as test_cpp_host.py does
    subprocess.run(["make", "-C", str(HOST), "plan_check"], check=True, capture_output=True)
    r = subprocess.run([str(HOST / "plan_check"), str(GOLDEN / "launch_plan_cases_v1.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got, want = r.stdout.splitlines(), (GOLDEN / "launch_plans_v1.txt").read_text().splitlines()
    assert len(want) >= 300 and len(got) == len(want)
    differ = [f"{g}\n   recorded: {w}" for g, w in zip(got, want) if g != w]
    assert not differ, f"{len(differ)} of {len(want)} plans differ from the recorded ones; the first:\n" + "\n".join(differ[:5])
