"""numpy reference of the material texture sampling of "depthPrepassRaster.comp", written from the contract text (DESIGN.md "Material textures in the depth
prepass"; csrc/kernels/depth_prepass_raster.hip implements the same contract independently and must agree bit for bit on every texel of albedo and specular).

It takes the winner keys of prepass_raster_reference.rasterise - visibility is not its business - re-derives each winner's draw and vertices from the draws and
the indices itself, and returns the albedo and specular images of a textured execution. fp64 operations are single np.float64 operations in the contract's order,
fp32 ones np.float32, det_log2f is the oracle's (pyoracle.math_eval(1, .)), taps and weights are int64 / Python integers.

Texture inputs (a dict): uvs n x 2 float32, materials d x 2 uint32, textures T x 4 uint32 {texelOffset, width, height, mipCount}, texels uint32, texture_count (the
push constant: entries at or past it do not exist), mip_bias.
"""
import numpy as np

import prepass_raster_reference as ref

F32 = np.float32
F64 = np.float64
NONE = 0xFFFFFFFF
MAX_SIZE = 16384
UV_LIMIT = F64(1048576.0)  # 2^20


def level_size(width, height, level):
    return max(1, width >> level), max(1, height >> level)


def level_offset(width, height, level):
    return sum(level_size(width, height, l)[0] * level_size(width, height, l)[1] for l in range(level))


def chain_texels(width, height, mips):
    return level_offset(width, height, mips)


def full_mip_count(width, height):
    return max(width, height).bit_length()  # floor(log2(max)) + 1


def build_chain(level0, width, height):
    """all levels of the full chain back to back: level l + 1 texel (x, y) per channel = (a + b + c + d + 2) >> 2 of the level-l texels at
    (min(2x, W - 1) | min(2x + 1, W - 1), min(2y, H - 1) | min(2y + 1, H - 1))"""
    levels = [np.asarray(level0, np.uint32).reshape(height, width)]
    w, h = width, height
    while w > 1 or h > 1:
        nw, nh = max(1, w >> 1), max(1, h >> 1)
        src = levels[-1]
        x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
        y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
        out = np.zeros((nh, nw), np.uint32)
        for shift in (0, 8, 16, 24):
            c = (src >> np.uint32(shift)) & np.uint32(255)
            s = c[np.ix_(y0, x0)] + c[np.ix_(y0, x1)] + c[np.ix_(y1, x0)] + c[np.ix_(y1, x1)] + np.uint32(2)
            out |= (s >> np.uint32(2)) << np.uint32(shift)
        levels.append(out)
        w, h = nw, nh
    return np.concatenate([l.reshape(-1) for l in levels])


def usable(tex, index):
    """the table entry a material word names, or None: none, at or past texture_count, or an unusable entry"""
    table = np.asarray(tex["textures"], np.uint32).reshape(-1, 4)
    if index == NONE or index >= tex["texture_count"] or index >= table.shape[0]:
        return None
    offset, width, height, mips = (int(v) for v in table[index])
    if not (1 <= width <= MAX_SIZE and 1 <= height <= MAX_SIZE and 1 <= mips <= full_mip_count(width, height)):
        return None
    return offset, width, height, mips


def _barycentrics(P, V):
    with np.errstate(all="ignore"):
        e = [ref._det(P, V[1], V[2]), ref._det(P, V[2], V[0]), ref._det(P, V[0], V[1])]
        s = (e[0] + e[1]) + e[2]
        good = (s != 0) & np.isfinite(s)
        safe = np.where(good, s, F64(1))
        return [np.where(good, e[0] / safe, F64(1)), np.where(good, e[1] / safe, F64(0)), np.where(good, e[2] / safe, F64(0))]


def levels_of(entry, du_dx, dv_dx, du_dy, dv_dy, mip_bias):
    """-> L0, L1, fw (int64 arrays) and lod (float32) for one texture"""
    import pyoracle
    _, width, height, mips = entry
    with np.errstate(all="ignore"):
        w0, h0 = F64(width), F64(height)
        axx, axy, ayx, ayy = du_dx * w0, dv_dx * h0, du_dy * w0, dv_dy * h0
        rx = axx * axx + axy * axy
        ry = ayx * ayx + ayy * ayy
        rho2 = np.where(rx > ry, rx, ry)
        r = rho2.astype(F32)
        lod = (F32(0.5) * pyoracle.math_eval(1, r).reshape(r.shape)).astype(F32) + F32(mip_bias)
        lod = np.where(lod > 0, lod, F32(0)).astype(F32)  # also a NaN
        top = F32(mips - 1)
        lod = np.where(lod > top, top, lod).astype(F32)
        q = np.floor((lod * F32(256.0)).astype(F32) + F32(0.5)).astype(np.int64)
    L0, fw = q >> 8, q & 255
    return L0, np.minimum(L0 + 1, mips - 1), fw, lod


def _taps(entry, texels, level, u, v):
    """per channel sums S_l (n x 4 int64) of the four taps of `level` (an int64 array: a level per pixel)"""
    offset, width, height, _ = entry
    out = np.zeros((u.size, 4), np.int64)
    for l in np.unique(level):
        sel = np.flatnonzero(level == l)
        W, H = level_size(width, height, int(l))
        base = offset + level_offset(width, height, int(l))
        with np.errstate(all="ignore"):
            Tu = np.floor((u[sel] * F64(W) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
            Tv = np.floor((v[sel] * F64(H) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
        x0, fx, y0, fy = Tu >> 8, Tu & 255, Tv >> 8, Tv & 255
        x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
        x0, y0 = np.mod(x0, W), np.mod(y0, H)

        def fetch(x, y):
            at = base + y * W + x
            inside = at < texels.size
            return np.where(inside, texels[np.where(inside, at, 0)], 0).astype(np.int64) if texels.size else np.zeros(at.shape, np.int64)

        c00, c10, c01, c11 = fetch(x0, y0), fetch(x1, y0), fetch(x0, y1), fetch(x1, y1)
        for k in range(4):
            ch = lambda c: (c >> (8 * k)) & 255
            out[sel, k] = (256 - fx) * (256 - fy) * ch(c00) + fx * (256 - fy) * ch(c10) + (256 - fx) * fy * ch(c01) + fx * fy * ch(c11)
    return out


def sample_texture(entry, texels, u, v, du_dx, dv_dx, du_dy, dv_dy, mip_bias, details=None):
    """one trilinear sample per pixel -> uint32 words. u, v: validated (for the taps); the four differences: raw"""
    L0, L1, fw, lod = levels_of(entry, du_dx, dv_dx, du_dy, dv_dy, mip_bias)
    S0, S1 = _taps(entry, texels, L0, u, v), _taps(entry, texels, L1, u, v)
    S = (256 - fw)[:, None] * S0 + fw[:, None] * S1
    assert S.max(initial=0) <= 255 << 24
    code = (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24
    if details is not None:
        details.update(L0=L0, L1=L1, fw=fw, lod=lod, S=S)
    return (code[:, 0] | (code[:, 1] << 8) | (code[:, 2] << 16) | (code[:, 3] << 24)).astype(np.uint32)


def sample(case, tex, keys, diagnostics=False):
    """-> dict(albedo, specular: uint32 h x w). diagnostics: also per output name the h x w arrays lod (float32, NaN where not sampled), L0, fw (-1 where not
    sampled), rx_gt_ry (int8: 1 where rx > ry, 0 where not, -1 where not sampled), and tu_min: the least level-0 Tu over the samples"""
    width, height = case["width"], case["height"]
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 48)
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    uvs = np.asarray(tex["uvs"], F32).reshape(-1, 2)
    materials = np.asarray(tex["materials"], np.uint32).reshape(-1, 2)
    texels = np.asarray(tex["texels"], np.uint32).reshape(-1)
    keys = np.asarray(keys, np.uint64)
    out = dict(albedo=np.zeros((height, width), np.uint32), specular=np.zeros((height, width), np.uint32))
    diag = {name: dict(lod=np.full((height, width), np.nan, F32), L0=np.full((height, width), -1, np.int64), fw=np.full((height, width), -1, np.int64),
                       rx_gt_ry=np.full((height, width), -1, np.int8)) for name in ("albedo", "specular")}
    jj, ii = np.nonzero(keys)
    t = (keys[jj, ii] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    owner = np.searchsorted(first_triangle, t, side="right") - 1  # the draw that holds triangle t (draws without triangles hold none)
    for d in np.unique(owner):
        sel = owner == d
        pj, pi = jj[sel], ii[sel]
        first, _, vertex_offset, transform_index, albedo, specular = (int(v) for v in draws[d])
        out["albedo"][pj, pi], out["specular"][pj, pi] = albedo, specular
        if d >= materials.shape[0]:
            continue
        entries = [usable(tex, int(materials[d, 0])), usable(tex, int(materials[d, 1]))]
        if entries[0] is None and entries[1] is None:
            continue
        local = t[sel] - first_triangle[d]
        vi = indices[first + 3 * local[:, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset  # n x 3
        mvp = transforms[transform_index, 16:32]
        V, tu, tv = [], [], []
        for k in range(3):
            clip = ref.transform4(mvp, positions[vi[:, k]])
            V.append((clip[:, 0].astype(F64), clip[:, 1].astype(F64), clip[:, 3].astype(F64)))
            inside = vi[:, k] < uvs.shape[0]
            at = np.where(inside, vi[:, k], 0)
            tu.append(np.where(inside, uvs[at, 0] if uvs.size else 0, 0).astype(F64))
            tv.append(np.where(inside, uvs[at, 1] if uvs.size else 0, 0).astype(F64))
        with np.errstate(all="ignore"):
            one = np.ones(pi.size, F64)
            Px = (2 * pi + 1).astype(F64) / F64(width) - F64(1)
            Py = (2 * pj + 1).astype(F64) / F64(height) - F64(1)
            Px1 = (2 * (pi + 1) + 1).astype(F64) / F64(width) - F64(1)
            Py1 = (2 * (pj + 1) + 1).astype(F64) / F64(height) - F64(1)
            b, bx, by = _barycentrics((Px, Py, one), V), _barycentrics((Px1, Py, one), V), _barycentrics((Px, Py1, one), V)
            u, v = ref._weighted(b, *tu), ref._weighted(b, *tv)
            du_dx, dv_dx = ref._weighted(bx, *tu) - u, ref._weighted(bx, *tv) - v
            du_dy, dv_dy = ref._weighted(by, *tu) - u, ref._weighted(by, *tv) - v
            valid = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < UV_LIMIT) & (np.abs(v) < UV_LIMIT)
            u, v = np.where(valid, u, F64(0)), np.where(valid, v, F64(0))
        for name, entry in zip(("albedo", "specular"), entries):
            if entry is None:
                continue
            details = {}
            out[name][pj, pi] = sample_texture(entry, texels, u, v, du_dx, dv_dx, du_dy, dv_dy, tex["mip_bias"], details)
            if diagnostics:
                g = diag[name]
                g["lod"][pj, pi], g["L0"][pj, pi], g["fw"][pj, pi] = details["lod"], details["L0"], details["fw"]
                with np.errstate(all="ignore"):
                    w0, h0 = F64(entry[1]), F64(entry[2])
                    rx = (du_dx * w0) * (du_dx * w0) + (dv_dx * h0) * (dv_dx * h0)
                    ry = (du_dy * w0) * (du_dy * w0) + (dv_dy * h0) * (dv_dy * h0)
                g["rx_gt_ry"][pj, pi] = (rx > ry).astype(np.int8)
                W = level_size(entry[1], entry[2], 0)[0]
                with np.errstate(all="ignore"):
                    g["tu_min"] = min(g.get("tu_min", 1 << 62), int(np.floor((u * F64(W) - F64(0.5)) * F64(256.0) + F64(0.5)).min()))
    if diagnostics:
        out["diagnostics"] = diag
    return out
