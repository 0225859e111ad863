"""The rule of mirt_ctx_reproject* and mirt_camera_project restated on the CPU (include/mirt.h): float32 throughout,
one IEEE operation per step in the header's order, fused only where the header writes fmaf (grid_rounding.fma32), the fixed-point
conversion and the resolve taken from the CPU reference library (oracle_binding).  Two restatements that share only those three
functions: `reproject` works on whole planes, one gather per tap; `reproject_naive` walks pixel by pixel and tap by tap with scalars.
Both return (float32 [rows, width, 4], uint8 [rows, width, 4]).  Nothing here runs a kernel of the library."""
import numpy as np

import oracle_binding as ob
from grid_rounding import fma32

f32 = np.float32
MISS = 0xFFFFFFFF
FEATURE_DTYPE = np.dtype([("albedo", "<f4", (3,)), ("t", "<f4"), ("normal", "<f4", (3,)), ("sphere", "<u4")])
TONE_FLAGS = (1 << 1) | (1 << 2)          # MIRT_FLAG_NO_TONEMAP | MIRT_FLAG_NO_SRGB, checked against _abi in the tests
CLAMP = 1                                 # MIRT_REPROJECT_CLAMP
INF = f32(np.inf)


def cam_vectors(cam):
    """(eye, horizontal, vertical, lower_left_corner) of a MirtGpuCamera as float32 [3] each."""
    g = lambda a: np.array(a[:3], f32)
    return g(cam.eye), g(cam.horizontal), g(cam.vertical), g(cam.lower_left_corner)


def _rgba(out, flags):
    rgba = np.full(out.shape[:-1] + (4,), 255, np.uint8)
    rgba[..., :3] = ob.resolve_channel(ob.to_fixed(np.ascontiguousarray(out[..., :3])).astype(np.uint64), 1, flags & TONE_FLAGS)
    return rgba


# ------------------------------------------------------------------------------------------ whole planes

def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f32) + a[..., 2] * b[..., 2]).astype(f32)


def project_rel(cam, w, h, rel):
    """(fx, fy, s) of points given relative to the camera's eye, rel float32 [..., 3]."""
    eye, H, V, llc = cam_vectors(cam)
    rel = np.asarray(rel, f32)
    with np.errstate(all="ignore"):
        a = (llc - eye).astype(f32)
        n = np.array([H[1] * V[2] - H[2] * V[1], H[2] * V[0] - H[0] * V[2], H[0] * V[1] - H[1] * V[0]], f32)
        s = (_dot(rel, n) / _dot(a, n)).astype(f32)
        q = ((rel / s[..., None]).astype(f32) - a).astype(f32)
        pu = (_dot(q, H) / _dot(H, H)).astype(f32)
        pv = (_dot(q, V) / _dot(V, V)).astype(f32)
        fx = ((pu * f32(w)).astype(f32) - f32(0.5)).astype(f32)
        fy = (((f32(1.0) - pv).astype(f32) * f32(h)).astype(f32) - f32(0.5)).astype(f32)
    return fx, fy, s


def project(cam, w, h, points):
    """mirt_camera_project for points float32 [..., 3] -> float32 [..., 3] = {fx, fy, s}."""
    eye = cam_vectors(cam)[0]
    with np.errstate(all="ignore"):
        rel = (np.asarray(points, f32) - eye).astype(f32)
    return np.stack(project_rel(cam, w, h, rel), -1)


def centre_rays(cam, w, h, xs, ys):
    """directions float32 [..., 3] of the centre rays of pixels (xs, ys) (the origin is the eye), as mirt_camera_pixel_ray."""
    eye, H, V, llc = cam_vectors(cam)
    inv_w, inv_h = f32(1.0) / f32(w), f32(1.0) / f32(h)
    u = ((xs.astype(f32) + f32(0.5)).astype(f32) * inv_w).astype(f32)
    v = (f32(1.0) - ((ys.astype(f32) + f32(0.5)).astype(f32) * inv_h).astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        return np.stack([(fma32(v, np.full_like(v, V[k]), fma32(u, np.full_like(u, H[k]), np.full_like(u, llc[k]))) - eye[k]).astype(f32)
                         for k in range(3)], -1)


def reproject(colour, guides, prev_colour, prev_guides, previous, current, width, height, row_begin=0, *, max_history=8.0,
              depth_tolerance=0.05, clamp=True, flags=0):
    """colour, prev_colour float32 [rows, width, 4]; guides, prev_guides FEATURE_DTYPE [rows, width]; the band starts at image row
    row_begin; `flags`: the tone flags of the RGBA8 plane."""
    colour, prev_colour = np.asarray(colour, f32), np.asarray(prev_colour, f32)
    guides, prev_guides = np.asarray(guides), np.asarray(prev_guides)
    R, W = guides.shape
    assert W == width and colour.shape == prev_colour.shape == (R, W, 4) and prev_guides.shape == (R, W)
    mh, dt = f32(max_history), f32(depth_tolerance)
    ys, xs = np.mgrid[row_begin:row_begin + R, 0:W]
    with np.errstate(all="ignore"):
        d = centre_rays(current, width, height, xs, ys)
        eye = cam_vectors(current)[0]
        pe = cam_vectors(previous)[0]
        hit = guides["sphere"] != MISS
        t = guides["t"].astype(f32)
        at = np.stack([(fma32(t, d[..., k], np.full_like(t, eye[k])) - pe[k]).astype(f32) for k in range(3)], -1)
        rel = np.where(hit[..., None], at, d).astype(f32)
        fx, fy, s = project_rel(previous, width, height, rel)
        fw, fh = f32(width), f32(height)
        ok = (s > 0) & (s < INF) & (fx > f32(-1.0)) & (fx < fw) & (fy > f32(-1.0)) & (fy < fh)
        flx, fly = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        ix, iy = np.where(ok, flx, f32(0)).astype(np.int64), np.where(ok, fly, f32(0)).astype(np.int64)
        wx, wy = (fx - flx).astype(f32), (fy - fly).astype(f32)
        wsum, lacc, acc = np.zeros((R, W), f32), np.zeros((R, W), f32), np.zeros((R, W, 3), f32)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = ix + dx, iy + dy - row_begin
                inb = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < R)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, R - 1)
                pg, pc = prev_guides[qyc, qxc], prev_colour[qyc, qxc]
                counts = inb & (pg["sphere"] == guides["sphere"]) & (pc[..., 3] >= f32(1.0))
                depth = np.abs((pg["t"] - s).astype(f32)) <= (dt * s).astype(f32)
                counts &= np.where(hit, depth, True)
                bw = ((wx if dx else (f32(1.0) - wx).astype(f32)) * (wy if dy else (f32(1.0) - wy).astype(f32))).astype(f32)
                wsum = np.where(counts, (wsum + bw).astype(f32), wsum)
                acc = np.where(counts[..., None], (acc + (bw[..., None] * pc[..., :3]).astype(f32)).astype(f32), acc)
                lacc = np.where(counts, (lacc + (bw * pc[..., 3]).astype(f32)).astype(f32), lacc)
        have = wsum >= f32(0.015625)
        hist = (acc / wsum[..., None]).astype(f32)
        hlen = (lacc / wsum).astype(f32)
        c = colour[..., :3]
        if clamp:
            lo, hi = c.copy(), c.copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    y0, y1, x0, x1 = max(0, -dy), min(R, R - dy), max(0, -dx), min(W, W - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    m = c[Q]
                    lo[P] = np.where(m < lo[P], m, lo[P])
                    hi[P] = np.where(m > hi[P], m, hi[P])
            hist = np.where(hist < lo, lo, hist)
            hist = np.where(hist > hi, hi, hist)
        nn = (hlen + f32(1.0)).astype(f32)
        nn = np.where(nn < mh, nn, mh).astype(f32)
        alpha = (f32(1.0) / nn).astype(f32)
        blend = (hist + (alpha[..., None] * (c - hist).astype(f32)).astype(f32)).astype(f32)
    out = np.empty((R, W, 4), f32)
    out[..., :3] = np.where(have[..., None], blend, c)
    out[..., 3] = np.where(have, nn, f32(1.0))
    return out, _rgba(out, flags)


# ------------------------------------------------------------------------------------------ pixel by pixel

def _fma1(a, b, c):
    return fma32(np.array([a], f32), np.array([b], f32), np.array([c], f32))[0]


def _sdot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def project_naive(cam, w, h, rel):
    """(fx, fy, s) of ONE point given relative to the eye, scalars only."""
    eye, H, V, llc = ([f32(x) for x in v[:3]] for v in (cam.eye, cam.horizontal, cam.vertical, cam.lower_left_corner))
    a = [f32(llc[k] - eye[k]) for k in range(3)]
    n = [f32(f32(H[1] * V[2]) - f32(H[2] * V[1])), f32(f32(H[2] * V[0]) - f32(H[0] * V[2])), f32(f32(H[0] * V[1]) - f32(H[1] * V[0]))]
    s = f32(_sdot(rel, n) / _sdot(a, n))
    q = [f32(f32(rel[k] / s) - a[k]) for k in range(3)]
    pu, pv = f32(_sdot(q, H) / _sdot(H, H)), f32(_sdot(q, V) / _sdot(V, V))
    return f32(f32(pu * f32(w)) - f32(0.5)), f32(f32(f32(f32(1.0) - pv) * f32(h)) - f32(0.5)), s


def reproject_naive(colour, guides, prev_colour, prev_guides, previous, current, width, height, row_begin=0, *, max_history=8.0,
                    depth_tolerance=0.05, clamp=True, flags=0):
    """The same rule pixel by pixel and tap by tap, scalars only."""
    colour, prev_colour = np.asarray(colour, f32), np.asarray(prev_colour, f32)
    R, W = np.shape(guides)
    mh, dt = f32(max_history), f32(depth_tolerance)
    eye, H, V, llc = ([f32(x) for x in v[:3]] for v in (current.eye, current.horizontal, current.vertical, current.lower_left_corner))
    pe = [f32(x) for x in previous.eye[:3]]
    inv_w, inv_h = f32(f32(1.0) / f32(width)), f32(f32(1.0) / f32(height))
    out = np.empty((R, W, 4), f32)
    with np.errstate(all="ignore"):
        for cy in range(R):
            for x in range(W):
                y = row_begin + cy
                u = f32(f32(f32(x) + f32(0.5)) * inv_w)
                v = f32(f32(1.0) - f32(f32(f32(y) + f32(0.5)) * inv_h))
                d = [f32(_fma1(v, V[k], _fma1(u, H[k], llc[k])) - eye[k]) for k in range(3)]
                g = guides[cy, x]
                sphere = int(g["sphere"])
                hit = sphere != MISS
                rel = [f32(_fma1(f32(g["t"]), d[k], eye[k]) - pe[k]) for k in range(3)] if hit else d
                fx, fy, s = project_naive(previous, width, height, rel)
                ok = bool(s > 0 and s < INF and fx > -1 and fx < f32(width) and fy > -1 and fy < f32(height))
                wsum, lacc, acc = f32(0.0), f32(0.0), [f32(0.0)] * 3
                if ok:
                    flx, fly = f32(np.floor(fx)), f32(np.floor(fy))
                    ix, iy, wx, wy = int(flx), int(fly), f32(fx - flx), f32(fy - fly)
                    for dy in (0, 1):
                        for dx in (0, 1):
                            qx, qy = ix + dx, iy + dy
                            if not (0 <= qx < width and row_begin <= qy < row_begin + R):
                                continue
                            pg, pc = prev_guides[qy - row_begin, qx], prev_colour[qy - row_begin, qx]
                            if int(pg["sphere"]) != sphere or not pc[3] >= f32(1.0):
                                continue
                            if hit and not abs(f32(f32(pg["t"]) - s)) <= f32(dt * s):
                                continue
                            bw = f32((wx if dx else f32(f32(1.0) - wx)) * (wy if dy else f32(f32(1.0) - wy)))
                            wsum = f32(wsum + bw)
                            acc = [f32(acc[k] + f32(bw * pc[k])) for k in range(3)]
                            lacc = f32(lacc + f32(bw * pc[3]))
                c = [f32(colour[cy, x, k]) for k in range(3)]
                if not wsum >= f32(0.015625):
                    out[cy, x] = c + [f32(1.0)]
                    continue
                hist = [f32(acc[k] / wsum) for k in range(3)]
                hlen = f32(lacc / wsum)
                if clamp:
                    lo, hi = list(c), list(c)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            mx, my = x + dx, cy + dy
                            if not (0 <= mx < W and 0 <= my < R):
                                continue
                            m = colour[my, mx]
                            for k in range(3):
                                lo[k] = f32(m[k]) if m[k] < lo[k] else lo[k]
                                hi[k] = f32(m[k]) if m[k] > hi[k] else hi[k]
                    for k in range(3):
                        hist[k] = lo[k] if hist[k] < lo[k] else hist[k]
                        hist[k] = hi[k] if hist[k] > hi[k] else hist[k]
                nn = f32(hlen + f32(1.0))
                nn = nn if nn < mh else mh
                alpha = f32(f32(1.0) / nn)
                out[cy, x] = [f32(hist[k] + f32(alpha * f32(c[k] - hist[k]))) for k in range(3)] + [nn]
    return out, _rgba(out, flags)


# ------------------------------------------------------------------------------------------ comparison

def same_f32_or_nan(got, want) -> np.ndarray:
    """Per float: the same bit pattern, any NaN counting as equal to any NaN."""
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))


def history_fraction(out) -> float:
    """The share of pixels whose record carries history (length above 1, or NaN: a length of 1 may also be max_history == 1)."""
    return float(np.mean(~(np.asarray(out)[..., 3] == 1)))


def mse(img, ref) -> float:
    return float(np.mean((np.asarray(img, np.float64)[..., :3] - np.asarray(ref, np.float64)[..., :3]) ** 2))
