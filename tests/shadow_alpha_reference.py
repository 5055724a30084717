"""numpy reference of an execution of "sunShadowRaster.comp" with textureCount > 0: alpha-tested cutout casters, written from the contract text (DESIGN.md
"Alpha-tested cutout casters in the sun shadow raster"; csrc/kernels/sun_shadow_raster.hip implements the same contract independently and must agree bit for bit
on every texel and counter).

The rasterisation contract is untouched: projection, snap, guard band, cull, box, coverage, the fp32 weights l1, l2, zf, clamp and code are written out here as
in tests/shadow_raster_reference.py (whose `project` and `clamp01` this module calls). One clause is added: a fragment of a draw with a cutoff c > 0 counts only
where its alpha code is >= c. The alpha is NOT the prepass sampler's: the level is one per (triangle, texture) from the triangle's constant UV gradient, the bias
is 0, and the UV is interpolated with the depth's fp32 weights. fp64 operations are single np.float64 operations in the contract's order, fp32 ones np.float32,
det_log2f is the oracle's (pyoracle.math_eval(1, .)), taps and weights are int64.

Texture inputs (a dict): uvs n x 2 float32, materials d x 2 uint32 {albedoTexture, cutoff}, textures T x 4 uint32 {texelOffset, width, height, mipCount}, texels
uint32 (RGBA8, R in the low byte, levels back to back and unpadded), texture_count (the push constant: entries at or past it do not exist).
"""
import numpy as np

import shadow_raster_reference as ref

F32 = np.float32
F64 = np.float64
NONE = 0xFFFFFFFF
MAX_SIZE = 16384
UV_LIMIT = F64(1048576.0)  # 2^20
DISCARD_ALL = 256


def cutoff_codes(words):
    """c = min(word, 256): a word above 255 is 256, which no alpha code reaches"""
    return np.minimum(np.asarray(words, np.uint32).astype(np.int64), DISCARD_ALL)


def usable(tex, index):
    """the table entry an albedoTexture word names, or None: none, at or past texture_count, or an unusable entry"""
    table = np.asarray(tex["textures"], np.uint32).reshape(-1, 4)
    if index == NONE or index >= tex["texture_count"] or index >= table.shape[0]:
        return None
    offset, width, height, mips = (int(v) for v in table[index])
    if not (1 <= width <= MAX_SIZE and 1 <= height <= MAX_SIZE and 1 <= mips <= max(width, height).bit_length()):
        return None
    return offset, width, height, mips


def level_dims(width, height, level):
    return max(1, width >> level), max(1, height >> level)


def triangle_level(entry, xs, ys, area, tu, tv):
    """L0, L1, fw of the triangle with snapped vertices (xs, ys), area A and vertex UVs tu, tv (float64, widened from fp32): the level clause"""
    import pyoracle
    _, width, height, mips = entry
    (x0, x1, x2), (y0, y1, y2) = xs, ys
    with np.errstate(all="ignore"):
        A = F64(area)
        sx20, sx01 = F64(-256 * (y0 - y2)), F64(-256 * (y1 - y0))
        sy20, sy01 = F64(256 * (x0 - x2)), F64(256 * (x1 - x0))
        du1, du2, dv1, dv2 = tu[1] - tu[0], tu[2] - tu[0], tv[1] - tv[0], tv[2] - tv[0]
        dudx = (sx20 / A) * du1 + (sx01 / A) * du2
        dvdx = (sx20 / A) * dv1 + (sx01 / A) * dv2
        dudy = (sy20 / A) * du1 + (sy01 / A) * du2
        dvdy = (sy20 / A) * dv1 + (sy01 / A) * dv2
        w0, h0 = F64(width), F64(height)
        axx, axy, ayx, ayy = dudx * w0, dvdx * h0, dudy * w0, dvdy * h0
        rx = axx * axx + axy * axy
        ry = ayx * ayx + ayy * ayy
        rho2 = rx if rx > ry else ry
        r = np.array([rho2], F64).astype(F32)
        lod = F32(F32(0.5) * pyoracle.math_eval(1, r).reshape(1)[0])  # bias 0
        if not lod > 0:  # also a NaN
            lod = F32(0)
        top = F32(mips - 1)
        if lod > top:
            lod = top
        q = int(np.floor(F32(lod * F32(256.0)) + F32(0.5)))
    L0, fw = q >> 8, q & 255
    return L0, min(L0 + 1, mips - 1), fw, dict(lod=float(lod), rx=float(rx), ry=float(ry))


def _alpha_taps(entry, texels, level, u, v):
    """S_l of the alpha channel (int64 per fragment) for the four taps of `level`"""
    offset, width, height, _ = entry
    W, H = level_dims(width, height, level)
    base = offset + sum(level_dims(width, height, l)[0] * level_dims(width, height, l)[1] for l in range(level))
    Tu = np.floor((u * F64(W) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
    Tv = np.floor((v * F64(H) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
    x0, fx, y0, fy = Tu >> 8, Tu & 255, Tv >> 8, Tv & 255
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    x0, y0 = np.mod(x0, W), np.mod(y0, H)

    def alpha(x, y):
        at = base + y * W + x
        inside = at < texels.size
        if not texels.size:
            return np.zeros(at.shape, np.int64)
        return (np.where(inside, texels[np.where(inside, at, 0)], 0).astype(np.int64) >> 24) & 255

    return (256 - fx) * (256 - fy) * alpha(x0, y0) + fx * (256 - fy) * alpha(x1, y0) + (256 - fx) * fy * alpha(x0, y1) + fx * fy * alpha(x1, y1)


def fragment_alpha(entry, texels, levels, tu, tv, l1, l2):
    """alpha codes (int64) of fragments with the depth's fp32 weights l1, l2"""
    L0, L1, fw = levels
    with np.errstate(all="ignore"):
        a, b = l1.astype(F64), l2.astype(F64)
        u = (tu[0] + a * (tu[1] - tu[0])) + b * (tu[2] - tu[0])
        v = (tv[0] + a * (tv[1] - tv[0])) + b * (tv[2] - tv[0])
        valid = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < UV_LIMIT) & (np.abs(v) < UV_LIMIT)
        u, v = np.where(valid, u, F64(0)), np.where(valid, v, F64(0))
    S = (256 - fw) * _alpha_taps(entry, texels, L0, u, v) + fw * _alpha_taps(entry, texels, L1, u, v)
    assert S.max(initial=0) <= 255 << 24
    return (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24, valid


def rasterise(case, tex, details=None):
    """case: the pass' inputs as tests/shadow_raster_cases.py builds them (res, light, transforms, positions, indices, draws); tex: see the module docstring.
    -> dict(map uint16 res x res, coverage int32 (fragments that count, per texel), submitted, drawn, rejects, tested, passed: covered fragments of sampled
    records and how many of them reach their cutoff). details: a list that receives one dict per sampled triangle (draw, L0, L1, fw, lod, rx, ry, invalid)"""
    res = int(case["res"])
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 16)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 4)
    uvs = np.asarray(tex["uvs"], F32).reshape(-1, 2)
    materials = np.asarray(tex["materials"], np.uint32).reshape(-1, 2)
    texels = np.asarray(tex["texels"], np.uint32).reshape(-1)
    depth = np.zeros((res, res), np.uint16)
    coverage = np.zeros((res, res), np.int32)
    submitted = drawn = rejects = tested = passed = 0
    for d, (first, count, vertex_offset, transform_index) in enumerate(draws.tolist()):
        n = count // 3
        submitted += n
        c = int(cutoff_codes(materials[d, 1])) if tex["texture_count"] else 0
        entry = usable(tex, int(materials[d, 0])) if c else None
        slot = first + 3 * np.arange(n, dtype=np.int64)
        in_buffers = (slot + 3 <= indices.size) & (transform_index < transforms.shape[0])
        idx = np.zeros((n, 3), np.int64)
        idx[in_buffers] = indices[slot[in_buffers, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset
        in_buffers &= (idx < positions.shape[0]).all(axis=1)
        rejects += int((~in_buffers).sum())
        if not in_buffers.any():
            continue
        idx = idx[in_buffers]
        X, Y, z, inside = ref.project(case["light"], transforms[transform_index], positions[idx.reshape(-1)], res)
        X, Y, z, inside = X.reshape(-1, 3), Y.reshape(-1, 3), z.reshape(-1, 3), inside.reshape(-1, 3)
        ok = inside.all(axis=1)
        rejects += int((~ok).sum())
        for t in np.flatnonzero(ok):
            xs, ys = [int(v) for v in X[t]], [int(v) for v in Y[t]]
            (x0, x1, x2), (y0, y1, y2) = xs, ys
            area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            if area <= 0:
                continue
            ix0, ix1 = max(0, (min(xs) + 127) >> 8), min(res - 1, (max(xs) - 128) >> 8)
            iy0, iy1 = max(0, (min(ys) + 127) >> 8), min(res - 1, (max(ys) - 128) >> 8)
            if ix0 > ix1 or iy0 > iy1:
                continue
            drawn += 1  # (whatever its alpha: the counters do not depend on it)
            if c == DISCARD_ALL:
                continue  # no alpha code reaches 256, sampled or constant
            px = (np.arange(ix0, ix1 + 1, dtype=np.int64) * 256 + 128)[None, :]
            py = (np.arange(iy0, iy1 + 1, dtype=np.int64) * 256 + 128)[:, None]
            covered = np.ones((iy1 - iy0 + 1, ix1 - ix0 + 1), bool)
            E = []
            for (xa, ya), (xb, yb) in (((x0, y0), (x1, y1)), ((x1, y1), (x2, y2)), ((x2, y2), (x0, y0))):
                dx, dy = xb - xa, yb - ya
                e = dx * (py - ya) - dy * (px - xa)
                covered &= (e > 0) | ((e == 0) & ((dy == 0 and dx > 0) or dy < 0))
                E.append(e)
            if not covered.any():
                continue
            fa = F32(area)
            l1 = E[2].astype(F32) / fa
            l2 = E[0].astype(F32) / fa
            with np.errstate(all="ignore"):
                dz1, dz2 = F32(z[t, 1] - z[t, 0]), F32(z[t, 2] - z[t, 0])
                zf = (z[t, 0] + l1 * dz1) + l2 * dz2
            code = np.rint(ref.clamp01(zf) * F32(65535.0)).astype(np.uint16)
            if c and entry is not None:  # (no usable texture: alpha 255 everywhere, which reaches every c <= 255)
                vi = idx[t]
                tu = [F64(uvs[v, 0]) if v < uvs.shape[0] else F64(0) for v in vi]
                tv = [F64(uvs[v, 1]) if v < uvs.shape[0] else F64(0) for v in vi]
                L0, L1, fw, more = triangle_level(entry, xs, ys, area, tu, tv)
                alpha, valid = fragment_alpha(entry, texels, (L0, L1, fw), tu, tv, l1[covered], l2[covered])
                tested += alpha.size
                passed += int((alpha >= c).sum())
                if details is not None:
                    details.append(dict(draw=d, L0=L0, L1=L1, fw=fw, invalid=int((~valid).sum()), fragments=alpha.size, passed=int((alpha >= c).sum()),
                                        alpha_min=int(alpha.min()), alpha_max=int(alpha.max()), **more))
                keep = covered.copy()
                keep[covered] = alpha >= c
                covered = keep
            sub = depth[iy0:iy1 + 1, ix0:ix1 + 1]
            sub[...] = np.where(covered, np.maximum(sub, code), sub)
            coverage[iy0:iy1 + 1, ix0:ix1 + 1] += covered
    return dict(map=depth, coverage=coverage, submitted=submitted, drawn=drawn, rejects=rejects, tested=tested, passed=passed)


def opaque_inputs(case):
    """texture inputs under which every draw of the case is opaque: all cutoffs 0, a table of one 1 x 1 texture nobody names"""
    d = np.asarray(case["draws"]).reshape(-1, 4).shape[0]
    return dict(uvs=np.zeros((0, 2), F32), materials=np.tile(np.array([[NONE, 0]], np.uint32), (d, 1)), textures=np.array([[0, 1, 1, 1]], np.uint32),
                texels=np.zeros(1, np.uint32), texture_count=1)
