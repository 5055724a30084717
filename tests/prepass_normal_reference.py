"""numpy reference of the normal maps of "depthPrepassRaster.comp", written from the contract text (DESIGN.md "Normal maps in the depth prepass";
csrc/kernels/depth_prepass_raster.hip implements the same contract independently and must agree bit for bit on every texel of shadingNormal).

It takes the winner keys and the `normal` image of prepass_raster_reference.rasterise (or of the alpha reference) - visibility and the vertex normal's word are not
its business - re-derives each winner's draw, vertices and barycentrics itself, samples the draw's normal texture with prepass_texture_reference's sampler (the
contract names that sampler's word), and returns the shadingNormal image. Every fp64 operation is one np.float64 operation in the contract's order.

Normal inputs (a dict): tangents, bitangents n x 3 float32, normal_materials d uint32 (a texture index or NONE), decode (1: the reference's, 2: unit).
"""
import numpy as np

import prepass_raster_reference as ref
import prepass_texture_reference as tref

F32 = np.float32
F64 = np.float64
NONE = tref.NONE
DECODE_REFERENCE, DECODE_UNIT = 1, 2


def decode_texel(cx, cy, decode):
    """n_t (three fp64 arrays) of the codes cx, cy (integers 0 .. 255)"""
    with np.errstate(all="ignore"):
        x, y = cx.astype(F64) / F64(255.0), cy.astype(F64) / F64(255.0)
        if decode == DECODE_REFERENCE:
            z = np.sqrt(((F64(1) - x * x) + y) + y)
            return F64(2) * x - F64(1), F64(2) * y - F64(1), F64(2) * z - F64(1)
        nx, ny = F64(2) * x - F64(1), F64(2) * y - F64(1)
        q = (F64(1) - nx * nx) - ny * ny
        return nx, ny, np.where(q > 0, np.sqrt(np.where(q > 0, q, F64(0))), F64(0))


def _rotate(m64, v):
    """mat3(model) * v: component r = (m[0][r] x + m[1][r] y) + m[2][r] z"""
    return [(m64[0 * 4 + r] * v[0] + m64[1 * 4 + r] * v[1]) + m64[2 * 4 + r] * v[2] for r in range(3)]


def _fetch3(buffer, vi):
    """3 floats per vertex as fp64 columns; a vertex outside the buffer has (0, 0, 0)"""
    buffer = np.asarray(buffer, F32).reshape(-1, 3)
    inside = vi < buffer.shape[0]
    at = np.where(inside, vi, 0)
    if buffer.shape[0] == 0:
        return [np.zeros(vi.size, F64) for _ in range(3)]
    return [np.where(inside, buffer[at, c], F32(0)).astype(F64) for c in range(3)]


def shade(case, tex, nm, keys, normal, variant=None, details=None):
    """-> shadingNormal uint32 h x w. variant "normalised": T, B and Nv are normalised before the multiply (NOT the contract: a test shows the difference).
    details: a dict that receives mapped (bool h x w: pixels whose draw has a usable normal texture), fallback (bool h x w: mapped pixels whose M did not
    normalise), L0 (int64 h x w, -1 where not sampled), nt (h x w x 3 float64, NaN where not sampled)"""
    width, height = case["width"], case["height"]
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 48)
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    normals = np.asarray(case["normals"], F32).reshape(-1, 3)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    uvs = np.asarray(tex["uvs"], F32).reshape(-1, 2)
    texels = np.asarray(tex["texels"], np.uint32).reshape(-1)
    words = np.asarray(nm["normal_materials"], np.uint32).reshape(-1)
    decode = int(nm["decode"])
    assert decode in (DECODE_REFERENCE, DECODE_UNIT)
    keys = np.asarray(keys, np.uint64)
    out = np.where(keys != 0, np.asarray(normal, np.uint32), np.uint32(0)).astype(np.uint32)  # no winner: 0; no normal map: the word of `normal`
    mapped = np.zeros((height, width), bool)
    fallback = np.zeros((height, width), bool)
    level0 = np.full((height, width), -1, np.int64)
    nt_image = np.full((height, width, 3), np.nan, F64)
    jj, ii = np.nonzero(keys)
    t = (keys[jj, ii] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    owner = np.searchsorted(first_triangle, t, side="right") - 1
    for d in np.unique(owner):
        if d >= draws.shape[0] or d >= words.size:
            continue
        entry = tref.usable(tex, int(words[d]))
        if entry is None:
            continue
        sel = owner == d
        pj, pi = jj[sel], ii[sel]
        first, _, vertex_offset, transform_index = (int(v) for v in draws[d, :4])
        local = t[sel] - first_triangle[d]
        vi = indices[first + 3 * local[:, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset
        model, mvp = transforms[transform_index, 0:16].astype(F64), transforms[transform_index, 16:32]
        pos = [positions[vi[:, k]] for k in range(3)]
        V, tu, tv = [], [], []
        for k in range(3):
            clip = ref.transform4(mvp, pos[k])
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
            b, bx, by = tref._barycentrics((Px, Py, one), V), tref._barycentrics((Px1, Py, one), V), tref._barycentrics((Px, Py1, one), V)
            u, v = ref._weighted(b, *tu), ref._weighted(b, *tv)
            du_dx, dv_dx = ref._weighted(bx, *tu) - u, ref._weighted(bx, *tv) - v
            du_dy, dv_dy = ref._weighted(by, *tu) - u, ref._weighted(by, *tv) - v
            valid = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < tref.UV_LIMIT) & (np.abs(v) < tref.UV_LIMIT)
            u, v = np.where(valid, u, F64(0)), np.where(valid, v, F64(0))
            sampled = {}
            texel = tref.sample_texture(entry, texels, u, v, du_dx, dv_dx, du_dy, dv_dy, tex["mip_bias"], sampled)
            nt = decode_texel(texel & np.uint32(255), (texel >> np.uint32(8)) & np.uint32(255), decode)
            # the per-vertex basis
            p64 = [p.astype(F64) for p in pos]
            a, c = p64[0] - p64[2], p64[0] - p64[1]
            face = ref._normalized(a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0])
            N, T, B = [], [], []
            for k in range(3):
                stored = normals[vi[:, k]]
                zero = (stored == 0).all(axis=1)
                n_in = [np.where(zero, face[i], stored[:, i].astype(F64)) for i in range(3)]
                N.append(ref._normalized(*_rotate(model, n_in)))
                T.append(ref._normalized(*_rotate(model, _fetch3(nm["tangents"], vi[:, k]))))
                B.append(ref._normalized(*_rotate(model, _fetch3(nm["bitangents"], vi[:, k]))))
            Ti = [ref._weighted(b, T[0][r], T[1][r], T[2][r]) for r in range(3)]
            Bi = [ref._weighted(b, B[0][r], B[1][r], B[2][r]) for r in range(3)]
            Nv = [ref._weighted(b, N[0][r], N[1][r], N[2][r]) for r in range(3)]
            if variant == "normalised":
                Ti, Bi, Nv = ref._normalized(*Ti), ref._normalized(*Bi), ref._normalized(*Nv)
            else:
                assert variant is None
            M = [(Ti[r] * nt[0] + Bi[r] * nt[1]) + Nv[r] * nt[2] for r in range(3)]
            ns = ref._normalized(*M)
            is_zero = (ns[0] == 0) & (ns[1] == 0) & (ns[2] == 0)
            word = ref._unorm8_half(ns[0]) | (ref._unorm8_half(ns[1]) << np.uint32(8)) | (ref._unorm8_half(ns[2]) << np.uint32(16)) | np.uint32(255 << 24)
        out[pj, pi] = np.where(is_zero, out[pj, pi], word)
        mapped[pj, pi] = True
        fallback[pj, pi] = is_zero
        level0[pj, pi] = sampled["L0"]
        for r in range(3):
            nt_image[pj, pi, r] = nt[r]
    if details is not None:
        details.update(mapped=mapped, fallback=fallback, L0=level0, nt=nt_image)
    return out


def derive_bitangents(tangents, normals):
    """the host's rule for absent bitangents: normalize(cross(tangent, normal)) per vertex in fp64, (0, 0, 0) where the length is not a finite number > 0"""
    t = np.asarray(tangents, F32).reshape(-1, 3).astype(F64)
    n = np.asarray(normals, F32).reshape(-1, 3).astype(F64)
    with np.errstate(all="ignore"):
        c = [t[:, 1] * n[:, 2] - t[:, 2] * n[:, 1], t[:, 2] * n[:, 0] - t[:, 0] * n[:, 2], t[:, 0] * n[:, 1] - t[:, 1] * n[:, 0]]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        good = (length > 0) & np.isfinite(length)
        safe = np.where(good, length, F64(1))
        return np.stack([np.where(good, c[r] / safe, F64(0)).astype(F32) for r in range(3)], axis=1)
