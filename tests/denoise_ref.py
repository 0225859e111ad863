"""The filter of mirt_ctx_denoise* restated on the CPU (include/mirt.h): float32 throughout, one IEEE operation per
step in the header's order, the exponential, the fixed-point conversion and the resolve taken from the CPU reference library
(oracle_binding).  Two restatements that share only those three functions: `denoise` works on whole planes, one shifted slice per tap;
`denoise_naive` walks pixel by pixel and tap by tap with scalars.  Both return (float32 [rows, width, 4], uint8 [rows, width, 4])."""
import numpy as np

import oracle_binding as ob

f32 = np.float32
MISS = 0xFFFFFFFF
FEATURE_DTYPE = np.dtype([("albedo", "<f4", (3,)), ("t", "<f4"), ("normal", "<f4", (3,)), ("sphere", "<u4")])
B = (1, 4, 6, 4, 1)
TONE_FLAGS = (1 << 1) | (1 << 2)          # MIRT_FLAG_NO_TONEMAP | MIRT_FLAG_NO_SRGB, checked against _abi in the tests


def level_scales(sigma_colour, levels):
    """inv_i = 1 / (sigma_colour 2^-i)^2 for i < levels, in float32 as the host computes it (None where sigma_colour == 0)."""
    if f32(sigma_colour) == 0:
        return [None] * levels
    out = []
    with np.errstate(all="ignore"):
        for i in range(levels):
            sg = f32(sigma_colour) * f32(2.0 ** -i)
            out.append(f32(1.0) / f32(sg * sg))
    return out


def scales_valid(sigma_colour, levels) -> bool:
    """What the library accepts as sigma_colour: not negative, not NaN, and every level's inv_i finite and positive."""
    s = f32(sigma_colour)
    if not s >= 0:
        return False
    return all(v is None or (np.isfinite(v) and v > 0) for v in level_scales(s, levels))


def means(sums, n):
    """float32 [..., 3]: (float)((double)sum / ((double)n * 2^20)), 0 where n == 0."""
    sums = np.asarray(sums, np.uint64)
    n = np.broadcast_to(np.asarray(n, np.uint32), sums.shape[:-1])
    with np.errstate(all="ignore"):
        m = (sums.astype(np.float64) / (n.astype(np.float64) * 1048576.0)[..., None]).astype(f32)
    m[n == 0] = 0
    return m


def divisors(guides):
    """float32 [..., 3]: the albedo where the centre ray hit and the albedo lies in [2^-6, 64], else 1."""
    alb = guides["albedo"]
    with np.errstate(invalid="ignore"):
        ok = (guides["sphere"] != MISS)[..., None] & (alb >= f32(0.015625)) & (alb <= f32(64.0))
    return np.where(ok, alb, f32(1.0)).astype(f32)


def _finish(c, den, flags):
    r = (c * den).astype(f32)
    out = np.ones(r.shape[:-1] + (4,), f32)
    out[..., :3] = r
    rgba = np.full(r.shape[:-1] + (4,), 255, np.uint8)
    rgba[..., :3] = ob.resolve_channel(ob.to_fixed(r).astype(np.uint64), 1, flags & TONE_FLAGS)
    return out, rgba


def denoise(sums, n, guides, levels, sigma_colour, normal_log2, flags=0):
    """sums uint64 [rows, width, 3], n uint32 [rows, width] or one count, guides FEATURE_DTYPE [rows, width]."""
    guides = np.asarray(guides)
    R, W = guides.shape
    den = divisors(guides)
    with np.errstate(all="ignore"):
        c = (means(sums, n).reshape(R, W, 3) / den).astype(f32)
        nrm, sph = guides["normal"].astype(f32), guides["sphere"]
        for i, inv in enumerate(level_scales(sigma_colour, levels)):
            s = 1 << i
            wsum, acc = np.zeros((R, W), f32), np.zeros((R, W, 3), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        wsum = wsum + f32(36.0)
                        acc = acc + f32(36.0) * c
                        continue
                    ox, oy = s * dx, s * dy
                    y0, y1, x0, x1 = max(0, -oy), min(R, R - oy), max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    kern = f32(B[dx + 2] * B[dy + 2])
                    np_, nq = nrm[P], nrm[Q]
                    x = ((np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]).astype(f32) + np_[..., 2] * nq[..., 2]).astype(f32)
                    x = np.where(x > 0, np.where(x < 1, x, f32(1.0)), f32(0.0)).astype(f32)
                    for _ in range(normal_log2):
                        x = (x * x).astype(f32)
                    wg = np.where(sph[P] != sph[Q], f32(0.0), np.where(sph[P] == MISS, f32(1.0), x)).astype(f32)
                    if inv is None:
                        wc = np.ones_like(wg)
                    else:
                        d = (c[P] - c[Q]).astype(f32)
                        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32)
                        wc = ob.exp((-(d2 * inv)).astype(f32))
                    w = ((kern * wg).astype(f32) * wc).astype(f32)
                    wsum[P] = wsum[P] + w
                    acc[P] = acc[P] + (w[..., None] * c[Q]).astype(f32)
            c = (acc / wsum[..., None]).astype(f32)
    return _finish(c, den, flags)


def denoise_naive(sums, n, guides, levels, sigma_colour, normal_log2, flags=0):
    """The same rule pixel by pixel and tap by tap, scalars only."""
    guides = np.asarray(guides)
    R, W = guides.shape
    sums = np.asarray(sums, np.uint64).reshape(R, W, 3)
    n = np.broadcast_to(np.asarray(n, np.uint32), (R, W))
    den = np.ones((R, W, 3), f32)
    c = np.zeros((R, W, 3), f32)
    with np.errstate(all="ignore"):
        for y in range(R):
            for x in range(W):
                g = guides[y, x]
                for k in range(3):
                    a = f32(g["albedo"][k])
                    if g["sphere"] != MISS and a >= f32(0.015625) and a <= f32(64.0):
                        den[y, x, k] = a
                    m = f32(0.0) if n[y, x] == 0 else f32(np.float64(sums[y, x, k]) / (np.float64(n[y, x]) * 1048576.0))
                    c[y, x, k] = f32(m / den[y, x, k])
        for i in range(levels):
            s = 1 << i
            inv = None
            if f32(sigma_colour) != 0:
                sg = f32(sigma_colour) * f32(2.0 ** -i)
                inv = f32(1.0) / f32(sg * sg)
            nxt = np.zeros_like(c)
            for y in range(R):
                for x in range(W):
                    wsum, acc = f32(0.0), [f32(0.0)] * 3
                    gp, cp = guides[y, x], c[y, x]
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = x + s * dx, y + s * dy
                            if not (0 <= qx < W and 0 <= qy < R):
                                continue
                            gq, cq = guides[qy, qx], c[qy, qx]
                            if dx == 0 and dy == 0:
                                w = f32(36.0)
                            else:
                                kern = f32(B[dx + 2] * B[dy + 2])
                                if gp["sphere"] == MISS and gq["sphere"] == MISS:
                                    wg = f32(1.0)
                                elif gp["sphere"] != gq["sphere"]:
                                    wg = f32(0.0)
                                else:
                                    a, b = gp["normal"], gq["normal"]
                                    t = f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))
                                    t = (t if t < 1 else f32(1.0)) if t > 0 else f32(0.0)
                                    for _ in range(normal_log2):
                                        t = f32(t * t)
                                    wg = t
                                if inv is None:
                                    wc = f32(1.0)
                                else:
                                    d = [f32(cp[k] - cq[k]) for k in range(3)]
                                    d2 = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
                                    wc = ob.exp(np.array([-f32(d2 * inv)], f32))[0]
                                w = f32(f32(kern * wg) * wc)
                            wsum = f32(wsum + w)
                            acc = [f32(acc[k] + f32(w * cq[k])) for k in range(3)]
                    nxt[y, x] = [f32(acc[k] / wsum) for k in range(3)]
            c = nxt
    return _finish(c, den, flags)


def same_f32(got, want) -> bool:
    """Bit for bit (every record is finite, so no NaN needs a rule)."""
    return np.array_equal(np.ascontiguousarray(got, f32).view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32))


def mse(img, ref) -> float:
    return float(np.mean((np.asarray(img, np.float64)[..., :3] - np.asarray(ref, np.float64)[..., :3]) ** 2))
