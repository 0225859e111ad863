"""The test-only device probe (oracle/mirt_math_probe.hip) must be compiled exactly as the product's kernels are: its exact
translation unit with FLAGS of the product's csrc/Makefile, its fast one with FAST_FLAGS.  Otherwise the exhaustive device
tests would check a different compilation from the one that ships."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _vars(path: Path) -> dict:
    text = path.read_text().replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^([A-Z_]+)\s*:=(.*)$", text, re.M):
        out[m.group(1)] = " ".join(m.group(2).split())
    return out


def test_probe_flags_match_the_product():
    product = _vars(ROOT / "weekend-raytracer-wgpu_amd" / "csrc" / "Makefile")
    probe = _vars(ROOT / "oracle" / "Makefile")
    for name in ("FLAGS", "FAST_FLAGS"):
        assert name in product and name in probe, name
        assert probe[name] == product[name], f"{name} of oracle/Makefile drifted from the product's:\n{probe[name]}\n{product[name]}"
    assert "-ffp-contract=off" in product["FLAGS"]


def test_probe_rules_use_the_right_flags():
    text = (ROOT / "oracle" / "Makefile").read_text()
    exact = re.search(r"^\$\(OUT\)/mirt_math_probe\.o:.*\n(?:\t@.*\n)*\t(.*)$", text, re.M)
    fast = re.search(r"^\$\(OUT\)/mirt_math_probe_fast\.o:.*\n(?:\t@.*\n)*\t(.*)$", text, re.M)
    assert exact and fast
    assert exact.group(1).split()[:2] == ["$(HIPCC)", "$(FLAGS)"], exact.group(1)
    assert fast.group(1).split()[:2] == ["$(HIPCC)", "$(FAST_FLAGS)"], fast.group(1)
    assert "libmirt_math_probe.so" in re.search(r"^all:(.*)$", text, re.M).group(1)
    src = (ROOT / "oracle" / "mirt_math_probe_fast.hip").read_text()
    assert "#define MIRT_FAST_MATH 1" in src and "#define MIRT_KNS fast_build" in src


def test_product_never_names_the_oracle():
    pkg = ROOT / "weekend-raytracer-wgpu_amd"
    hits = [str(p) for p in pkg.rglob("*") if p.is_file() and p.suffix in (".py", ".hip", ".h", ".inc", ".cpp", ".rs", "")
            and "oracle" in p.read_text(errors="ignore").lower()]
    assert not hits, hits
