"""The line contract of "debugGeometry.comp" (DESIGN.md "Debug geometry as a compute pass"; plainrenderer_amd/csrc/kernels/debug_geometry.hip), restated in numpy
float32 / float64 and Python integers, independently of the kernel: tests/test_debug_lines_cpu.py holds it to its own properties, tests/test_debug_lines.py and
tests/test_debug_lines_frame.py hold the GPU to it, word for word.

  1. segments, numbered in submission order: the 12 edges of every draw's world box (s = 12 d + e), then of every SDF box (s = 12 (draws + i) + e), then the
     caller's lines (s = 12 (draws + boxes) + l). A box that submits nothing leaves its numbers unused.
  2. clip = viewProjection * (p, 1); five planes (w - z, 32 w -+ x, 32 w -+ y); an end with !(d >= 0) is outside; both: rejected; one: replaced by
     I + t (O - I), t = d_I / (d_I - d_O), counted as clipped. Then w > 0, |xf|, |yf| < 2^20, finite z, else rejected. X = rint(xf * 256).
  3. coverage in integers: one pixel per major step at the centres c = 256 i + 128 with U0 <= c < U1, minor index by a floor division.
  4. depth in fp64, rounded once to fp32; kept when zf > 0 and zf >= depth[pixel] (the image as found).
  5. a pixel's winner is the maximum of (bits(zf) << 32) | s; it stores its colour word and zf.
Everything fp32 is computed with numpy float32 scalars (IEEE, one rounding per operation); matrices are 16 floats, column-major.
"""
import numpy as np

from plainrenderer_amd import pixfmt

F32 = np.float32
GUARD_NDC = F32(32.0)
GUARD_PIXELS = F32(1048576.0)
DRAW_BOX_RGB = (1.0, 0.0, 0.0)
SDF_BOX_RGB = (0.0, 1.0, 0.0)
STAT_NAMES = ("submitted", "clipped", "rejected", "drawn", "fragments", "pixels_written")


def transform_component(m, i, x, y, z):
    """component i of m * (x, y, z, 1): ((m[0][i] x + m[1][i] y) + m[2][i] z) + m[3][i], fp32"""
    return F32(F32(F32(F32(m[i] * x) + F32(m[4 + i] * y)) + F32(m[8 + i] * z)) + m[12 + i])


def world_box(lo, hi, model):
    """the axis-aligned world box of the local box {lo, hi} under `model` (16 floats): minimum and maximum over corners 0 .. 7 in that order, by `c < lo` / `c > hi`"""
    lo, hi, m = np.asarray(lo, F32), np.asarray(hi, F32), np.asarray(model, F32).reshape(16)
    wlo, whi = [None] * 3, [None] * 3
    with np.errstate(all="ignore"):
        for k in range(8):
            x, y, z = (hi[0] if k & 1 else lo[0]), (hi[1] if k & 2 else lo[1]), (hi[2] if k & 4 else lo[2])
            for r in range(3):
                c = transform_component(m, r, x, y, z)
                if k == 0:
                    wlo[r] = whi[r] = c
                else:
                    wlo[r] = c if c < wlo[r] else wlo[r]
                    whi[r] = c if c > whi[r] else whi[r]
    return np.array(wlo, F32), np.array(whi, F32)


def box_edges(lo, hi):
    """the 12 edges in order: for axis a = 0, 1, 2, for ascending corner k with bit a clear: (corner k, corner k | 1 << a) -> [(a xyz, b xyz)]"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)

    def corner(k):
        return np.array([hi[r] if (k >> r) & 1 else lo[r] for r in range(3)], F32)
    return [(corner(k), corner(k | (1 << a))) for a in range(3) for k in range(8) if not (k >> a) & 1]


def segments(draws=None, bounds=None, transforms=None, sdf_boxes=None, lines=None, draws_culled=False):
    """-> (slots, [(s, a, b, rgb)]): `slots` numbers exist; the list holds the segments that are submitted, in order.
    draws d x 6 uint32, bounds d x 6, transforms n x 48 (model first), sdf_boxes i x 8 (min.xyz, pad, max.xyz, pad), lines l x 9"""
    out, s = [], 0
    if draws is not None and len(draws):
        draws, bounds = np.asarray(draws, np.uint32).reshape(-1, 6), np.asarray(bounds, F32).reshape(-1, 6)
        transforms = np.asarray(transforms, F32).reshape(-1, 48)
        for d in range(draws.shape[0]):
            t = int(draws[d, 3])
            if t < transforms.shape[0] and not (draws_culled and int(draws[d, 1]) == 0):
                wlo, whi = world_box(bounds[d, :3], bounds[d, 3:], transforms[t, :16])
                out += [(s + e, a, b, DRAW_BOX_RGB) for e, (a, b) in enumerate(box_edges(wlo, whi))]
            s += 12
    if sdf_boxes is not None and len(sdf_boxes):
        for bb in np.asarray(sdf_boxes, F32).reshape(-1, 8):
            out += [(s + e, a, b, SDF_BOX_RGB) for e, (a, b) in enumerate(box_edges(bb[0:3], bb[4:7]))]
            s += 12
    if lines is not None and len(lines):
        for l in np.asarray(lines, F32).reshape(-1, 9):
            out.append((s, l[0:3].copy(), l[3:6].copy(), tuple(float(v) for v in l[6:9])))
            s += 1
    return s, out


def plane_distance(plane, c):
    x, y, z, w = c
    if plane == 0:
        return F32(w - z)
    if plane == 1:
        return F32(F32(GUARD_NDC * w) - x)
    if plane == 2:
        return F32(F32(GUARD_NDC * w) + x)
    if plane == 3:
        return F32(F32(GUARD_NDC * w) - y)
    return F32(F32(GUARD_NDC * w) + y)


def clip_and_snap(a, b, view_projection, width, height):
    """-> dict(rejected, clipped, and for a survivor X0, Y0, z0, X1, Y1, z1)"""
    m = np.asarray(view_projection, F32).reshape(16)
    with np.errstate(all="ignore"):
        A = [transform_component(m, i, F32(a[0]), F32(a[1]), F32(a[2])) for i in range(4)]
        B = [transform_component(m, i, F32(b[0]), F32(b[1]), F32(b[2])) for i in range(4)]
        clipped = False
        for plane in range(5):
            da, db = plane_distance(plane, A), plane_distance(plane, B)
            ina, inb = bool(da >= 0), bool(db >= 0)
            if not ina and not inb:
                return dict(rejected=True, clipped=clipped)
            if ina != inb:
                clipped = True
                inside, outside = (A, B) if ina else (B, A)
                di, do = (da, db) if ina else (db, da)
                t = F32(di / F32(di - do))
                new = [F32(inside[i] + F32(t * F32(outside[i] - inside[i]))) for i in range(4)]
                if ina:
                    B = new
                else:
                    A = new
        ends = []
        wf, hf = F32(width), F32(height)
        for x, y, z, w in (A, B):
            nx, ny, nz = F32(x / w), F32(y / w), F32(z / w)
            xf, yf = F32(F32(F32(nx * F32(0.5)) + F32(0.5)) * wf), F32(F32(F32(ny * F32(0.5)) + F32(0.5)) * hf)
            if not (w > 0 and abs(xf) < GUARD_PIXELS and abs(yf) < GUARD_PIXELS and abs(nz) < np.inf):
                return dict(rejected=True, clipped=clipped)
            ends.append((int(np.rint(F32(xf * F32(256.0)))), int(np.rint(F32(yf * F32(256.0)))), nz))
    return dict(rejected=False, clipped=clipped, X0=ends[0][0], Y0=ends[0][1], z0=ends[0][2], X1=ends[1][0], Y1=ends[1][1], z1=ends[1][2])


def cover(X0, Y0, z0, X1, Y1, z1, width, height):
    """the fragments of a snapped segment -> dict(drawn, x_major, xs, ys (int64 arrays), zf (float32 array)), one entry per fragment in ascending major order"""
    X0, Y0, X1, Y1 = int(X0), int(Y0), int(X1), int(Y1)
    dX, dY = X1 - X0, Y1 - Y0
    x_major = abs(dX) >= abs(dY)
    U0, V0, U1, V1 = (X0, Y0, X1, Y1) if x_major else (Y0, X0, Y1, X1)
    EU, EV = (width, height) if x_major else (height, width)
    if U0 > U1:
        U0, V0, U1, V1, z0, z1 = U1, V1, U0, V0, z1, z0
    dU, dV = U1 - U0, V1 - V0
    none = dict(drawn=False, x_major=x_major, xs=np.zeros(0, np.int64), ys=np.zeros(0, np.int64), zf=np.zeros(0, F32), steps=0)
    if dU == 0:
        return none
    i0, i1 = max(0, (U0 + 127) >> 8), min(EU - 1, (U1 - 129) >> 8)
    if i1 < i0:
        return none
    i = np.arange(i0, i1 + 1, dtype=np.int64)
    c = 256 * i + 128
    j = (V0 * dU + (c - U0) * dV) // (256 * dU)  # numpy's // on int64 floors
    with np.errstate(all="ignore"):
        t = (c - U0).astype(np.float64) / np.float64(dU)
        zf = (np.float64(z0) + t * (np.float64(z1) - np.float64(z0))).astype(F32)
    inside = (j >= 0) & (j < EV)
    i, j, zf = i[inside], j[inside], zf[inside]
    return dict(drawn=True, x_major=x_major, xs=i if x_major else j, ys=j if x_major else i, zf=zf, steps=i1 - i0 + 1)


def color_word(rgb):
    return int(pixfmt.pack_r11g11b10(np.asarray(rgb, F32).reshape(1, 3)).reshape(-1)[0])


def draw(color, depth, view_projection, draws=None, bounds=None, transforms=None, sdf_boxes=None, lines=None, draws_culled=False, details=False):
    """the pass: color (h x w uint32 words) and depth (h x w float32) as it finds them -> (color, depth, stats dict[, per-segment details])"""
    color, depth = np.array(color, np.uint32), np.array(depth, F32)
    h, w = depth.shape
    slots, segs = segments(draws, bounds, transforms, sdf_boxes, lines, draws_culled)
    stats = dict.fromkeys(STAT_NAMES, 0)
    keys = np.zeros((h, w), np.uint64)
    words = {}
    info = []
    for s, a, b, rgb in segs:
        stats["submitted"] += 1
        r = clip_and_snap(a, b, view_projection, w, h)
        stats["clipped"] += int(r["clipped"])
        if r["rejected"]:
            stats["rejected"] += 1
            info.append(dict(s=s, rejected=True, clipped=r["clipped"]))
            continue
        f = cover(r["X0"], r["Y0"], r["z0"], r["X1"], r["Y1"], r["z1"], w, h)
        info.append(dict(s=s, rejected=False, clipped=r["clipped"], snapped=r, **f))
        if not f["drawn"]:
            continue
        stats["drawn"] += 1
        words[s] = color_word(rgb)
        with np.errstate(invalid="ignore"):
            kept = (f["zf"] > 0) & (f["zf"] >= depth[f["ys"], f["xs"]])
        stats["fragments"] += int(kept.sum())
        key = (f["zf"][kept].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(s + 1)
        np.maximum.at(keys, (f["ys"][kept], f["xs"][kept]), key)
    won = keys != 0
    stats["pixels_written"] = int(won.sum())
    winner = (keys[won] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    color[won] = np.array([words[int(s)] for s in winner], np.uint32).reshape(-1)
    depth[won] = (keys[won] >> np.uint64(32)).astype(np.uint32).view(F32)
    if details:
        return color, depth, stats, dict(segments=info, winner=np.where(won, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1, -1))
    return color, depth, stats
