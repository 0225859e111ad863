#!/usr/bin/env python3
"""Are the kernels of one build's gfx950 assembly those of another's?  Compares, function by function, the instruction text of two
`.s` files written by `make -C weekend-raytracer-wgpu_amd/csrc asm` (build/mirt_kernels-hip-amdgcn-amd-amdhsa-gfx950.s), comments
dropped and the function's ordinal taken out of its local labels (.LBB<ordinal>_<n>: a kernel added in the middle of the file renumbers
every later one).  Prints how many functions of the first file are in the second with the same text, the names that differ or are
missing, the names only the second has, and one SHA-256 over the first file's functions as each file has them.
    python tools/isa_bodies.py PARENT.s THIS.s"""
import hashlib
import re
import sys


def bodies(path):
    out, name, buf = {}, None, []
    for line in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):\s", line + " ")
        if m:
            name, buf = m.group(1), []
        elif name is not None:
            if line.strip().startswith(".Lfunc_end"):
                out[name], name = "\n".join(buf), None
            elif not line.strip().startswith(";"):
                buf.append(re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)(\d+)_", r".L\1_", re.sub(r"\s*;.*$", "", line)))
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    differ = sorted(k for k in a if a[k] != b.get(k))
    digest = lambda d: hashlib.sha256("\n".join(k + "\n" + d.get(k, "") for k in sorted(a)).encode()).hexdigest()
    print(f"{len(a)} functions in the first file, {len(a) - len(differ)} of them with the same text in the second, {len(differ)} differ or are missing")
    for k in differ:
        print("  differs:", k)
    for k in sorted(set(b) - set(a)):
        print("  only in the second:", k)
    print("sha256 over the first file's functions:", digest(a), digest(b))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
