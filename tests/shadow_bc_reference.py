"""numpy reference of a format-aware execution of "sunShadowRaster.comp" (textureCount > 0, textureFormats = 1): cutout casters whose textures are RGBA8, BC1, BC3
or BC5, written from the contract text (DESIGN.md "Block-compressed cutout textures in the sun shadow raster"; csrc/kernels/sun_shadow_raster.hip implements the
same contract independently and must agree bit for bit on every texel and counter).

It is tests/shadow_alpha_reference.py's rasterise with the texel fetch replaced: the projection, snap, cull, box, coverage, weights, depth code (the loop below, as
that module writes it), the level of a triangle (its triangle_level, called) and the UV, validity rule, tap positions, weights and rounding of a fragment stay; what
changes is where the alpha of tap (x, y) of a level comes from.
  the store      `texels` are uint32 words, `textures` rows carry word offsets, `formats` one code per row (tests/prepass_bc_reference.py's mixed store)
  usable         the cutout contract's shape rule, and: a code above 3 or a compressed row whose offset is no multiple of its block's words (2 for BC1, 4 for BC3
                 and BC5) makes the row unusable - alpha 255 everywhere, as for a draw without a texture
  BC1, BC5       alpha 255 everywhere: the draw is never sampled (opaque for c <= 255, nothing for c = 256)
  RGBA8          bits 24 - 31 of the word at offset + level offset + y W + x, 0 outside `texels`
  BC3            level l starts at offset + sum of 4 ceil(W_k / 4) ceil(H_k / 4) words over k < l; the block of (x, y) is ((y >> 2) ceil(W / 4) + (x >> 2)) blocks in;
                 a block that does not lie wholly inside `texels` reads 0; else the code of texel 4 (y & 3) + (x & 3) of its alpha block (the first 8 bytes),
                 decoded by prepass_bc_reference.decode_alpha_blocks
"""
import numpy as np

import prepass_bc_reference as bc
import shadow_alpha_reference as aref
import shadow_raster_reference as ref

F32 = np.float32
F64 = np.float64
BLOCK_WORDS = {bc.BC1: 2, bc.BC3: 4, bc.BC5: 4}


def usable(tex, index):
    """(offset, width, height, mips, format) of the row an albedoTexture word names, or None"""
    entry = aref.usable(tex, index)
    if entry is None:
        return None
    formats = np.asarray(tex["formats"], np.uint32).reshape(-1)
    fmt = int(formats[index])
    if fmt > bc.BC5 or (fmt != bc.RGBA8 and entry[0] % BLOCK_WORDS[fmt]):
        return None
    return entry + (fmt,)


def _bc3_alpha_taps(entry, words, level, u, v, modes):
    """S_l of the alpha channel (int64 per fragment) for the four taps of `level` of a BC3 entry; modes: a set that receives "eight" / "six" per sampled block"""
    offset, width, height, _, _ = entry
    W, H = aref.level_dims(width, height, level)
    base = offset + sum(bc.level_words(bc.BC3, *aref.level_dims(width, height, l)) for l in range(level))
    Tu = np.floor((u * F64(W) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
    Tv = np.floor((v * F64(H) - F64(0.5)) * F64(256.0) + F64(0.5)).astype(np.int64)
    x0, fx, y0, fy = Tu >> 8, Tu & 255, Tv >> 8, Tv & 255
    x1, y1 = np.mod(x0 + 1, W), np.mod(y0 + 1, H)
    x0, y0 = np.mod(x0, W), np.mod(y0, H)
    blocks_per_row = (W + 3) // 4

    def alpha(x, y):
        at = base + ((y >> 2) * blocks_per_row + (x >> 2)) * 4
        inside = at + 4 <= words.size
        if not inside.any():
            return np.zeros(at.shape, np.int64)
        safe = np.where(inside, at, 0)
        halves = np.stack([words[safe], words[safe + 1]], axis=-1).astype("<u4")  # the alpha block alone
        blocks = halves.view(np.uint8).reshape(-1, 8)
        codes = bc.decode_alpha_blocks(blocks).astype(np.int64)
        picked = codes[np.arange(codes.shape[0]), (4 * (y & 3) + (x & 3)).reshape(-1)].reshape(at.shape)
        if modes is not None:
            sampled = blocks[inside.reshape(-1)]
            modes.update(np.where(sampled[:, 0] > sampled[:, 1], "eight", "six").tolist())
        return np.where(inside, picked, 0)

    return (256 - fx) * (256 - fy) * alpha(x0, y0) + fx * (256 - fy) * alpha(x1, y0) + (256 - fx) * fy * alpha(x0, y1) + fx * fy * alpha(x1, y1)


def fragment_alpha(entry, words, levels, tu, tv, l1, l2, modes=None):
    """alpha codes (int64) of fragments with the depth's fp32 weights l1, l2: shadow_alpha_reference.fragment_alpha for an RGBA8 entry, the same with the block
    fetch for a BC3 one"""
    if entry[4] == bc.RGBA8:
        return aref.fragment_alpha(entry[:4], words, levels, tu, tv, l1, l2)
    assert entry[4] == bc.BC3
    L0, L1, fw = levels
    with np.errstate(all="ignore"):
        a, b = l1.astype(F64), l2.astype(F64)
        u = (tu[0] + a * (tu[1] - tu[0])) + b * (tu[2] - tu[0])
        v = (tv[0] + a * (tv[1] - tv[0])) + b * (tv[2] - tv[0])
        valid = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < aref.UV_LIMIT) & (np.abs(v) < aref.UV_LIMIT)
        u, v = np.where(valid, u, F64(0)), np.where(valid, v, F64(0))
    S = (256 - fw) * _bc3_alpha_taps(entry, words, L0, u, v, modes) + fw * _bc3_alpha_taps(entry, words, L1, u, v, modes)
    assert S.max(initial=0) <= 255 << 24
    return (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24, valid


def rasterise(case, tex, details=None):
    """case, tex: as shadow_alpha_reference.rasterise takes them, tex with `formats` and the mixed store. -> the same dict. tested / passed count the fragments of
    sampled records only: RGBA8 and BC3. details: one dict per sampled triangle, as there, with `format` and `modes` (the alpha block modes among the blocks it read)"""
    res = int(case["res"])
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 16)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 4)
    uvs = np.asarray(tex["uvs"], F32).reshape(-1, 2)
    materials = np.asarray(tex["materials"], np.uint32).reshape(-1, 2)
    words = np.asarray(tex["texels"], np.uint32).reshape(-1)
    depth = np.zeros((res, res), np.uint16)
    coverage = np.zeros((res, res), np.int32)
    submitted = drawn = rejects = tested = passed = 0
    for d, (first, count, vertex_offset, transform_index) in enumerate(draws.tolist()):
        n = count // 3
        submitted += n
        c = int(aref.cutoff_codes(materials[d, 1])) if tex["texture_count"] else 0
        entry = usable(tex, int(materials[d, 0])) if c else None
        if entry is not None and entry[4] in (bc.BC1, bc.BC5):
            entry = None  # alpha 255 everywhere: like a draw without a usable texture
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
            if c == aref.DISCARD_ALL:
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
            if c and entry is not None:
                vi = idx[t]
                tu = [F64(uvs[v, 0]) if v < uvs.shape[0] else F64(0) for v in vi]
                tv = [F64(uvs[v, 1]) if v < uvs.shape[0] else F64(0) for v in vi]
                L0, L1, fw, more = aref.triangle_level(entry[:4], xs, ys, area, tu, tv)
                modes = set()
                alpha, valid = fragment_alpha(entry, words, (L0, L1, fw), tu, tv, l1[covered], l2[covered], modes)
                tested += alpha.size
                passed += int((alpha >= c).sum())
                if details is not None:
                    details.append(dict(draw=d, L0=L0, L1=L1, fw=fw, invalid=int((~valid).sum()), fragments=alpha.size, passed=int((alpha >= c).sum()),
                                        alpha_min=int(alpha.min()), alpha_max=int(alpha.max()), format=entry[4], modes=modes, **more))
                keep = covered.copy()
                keep[covered] = alpha >= c
                covered = keep
            sub = depth[iy0:iy1 + 1, ix0:ix1 + 1]
            sub[...] = np.where(covered, np.maximum(sub, code), sub)
            coverage[iy0:iy1 + 1, ix0:ix1 + 1] += covered
    return dict(map=depth, coverage=coverage, submitted=submitted, drawn=drawn, rejects=rejects, tested=tested, passed=passed)
