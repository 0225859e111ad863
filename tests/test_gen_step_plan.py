"""The pooled kernel's default geometry must keep six blocks per CU resident on BASELINE config 3 (three spheres, 1920x1080, 1000 spp):
its LDS decides that -- 24 waves x (112 slots + rings + accumulators) beside the scene in a CU's 160 KB -- and whatever a GEN step
keeps per strip has to fit in it.  No GPU: host/plan_check prints the launch plan (csrc/mirt_launch_plan.h) of the case."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "weekend-raytracer-wgpu_amd" / "host"
LDS_PER_CU = 160 * 1024
CUS = 256


def test_config3_still_plans_six_blocks_per_cu(tmp_path):
    subprocess.run(["make", "-C", str(HOST), "plan_check"], check=True, capture_output=True)
    cases = tmp_path / "cases.txt"
    # no `res`: the occupancy answer is left out, so the LDS of a block alone decides the blocks per CU
    cases.write_text(f"name=config3 cu={CUS} ldscu={LDS_PER_CU} ldsblk={LDS_PER_CU} ns=3 nm=5 nr=3 flat=1 w=1920 h=1080 spp=1000 nb=8 mode=1\n")
    r = subprocess.run([str(HOST / "plan_check"), str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    line = r.stdout.strip()
    assert line.startswith("config3 pt-pool "), line
    pool = re.search(r" pool=(\d+)/(\d+)/(\d+) ", line)
    lds, blocks = int(re.search(r" lds=(\d+) ", line).group(1)), int(re.search(r" blocks=(\d+) ", line).group(1))
    assert (int(pool.group(1)), int(pool.group(2))) == (256, 112), line          # four waves of 112 slots
    assert " cfg=0/3 " in line, line                                             # the default geometry, three scatter queues
    assert int(pool.group(3)) < lds                                              # the pools, and the scene beside them
    assert 6 * lds <= LDS_PER_CU < 7 * lds, line
    assert blocks == 6 * CUS, line
