"""numpy reference of the anisotropic filtering of "depthPrepassRaster.comp", written from the contract text (DESIGN.md "Anisotropic filtering in the depth
prepass"; csrc/kernels/depth_prepass_raster.hip implements the same contract independently and must agree bit for bit on all six images and all counters).

An execution with maxAnisotropy A >= 2 samples every texture - the albedo and specular words of the resolve, the alpha of the coverage path, the normal-map
texel - with N probes along the major axis of the pixel's footprint:
  ax, ay, rx, ry    as the sampling contract computes them; the major axis is x where rx > ry, else y; rmax = rho2, rmin the other; (du, dv) the raw forward
                    differences of the major axis
  N                 N = 1; while N < A and (double)(N N) rmin < rmax: N += 1
  level             r = (float)(rho2 / (double)(N N)), then lod, the clamps, q, L0, L1, fw as before
  probes            N = 1: (u, v) as validated; N > 1: t_k = (double)(2 k + 1 - N) / (double)(2 N), u_k = u + t_k du, v_k = v + t_k dv from the RAW u, v, and the
                    validity rule anew per probe: not finite or |.| >= 2^20 -> that probe taps at (0, 0)
  sum               T = sum over k of S_k = (256 - fw) S_L0 + fw S_L1, in integers
  code              T / (N 2^24) rounded half to even: D = N 2^24, qd = T // D, rem = T - qd D, code = qd + (2 rem > D or (2 rem == D and qd odd))
With A <= 1 this module runs the same text with N = 1 everywhere, which must give the isotropic references' bytes (tests/test_prepass_aniso_cpu.py).

The barycentrics, the four taps of a level and the block decode are the existing references' (prepass_raster_reference, prepass_texture_reference._barycentrics
and ._taps, prepass_bc_reference.decode_store); the UV fetch, the raw differences, the probe loop and the drivers - winners, the alpha test, the shading normal -
are written here. Texture inputs: the dict prepass_texture_reference describes; a mixed store (with `formats`) is decoded first.
"""
import numpy as np

import prepass_alpha_reference as aref
import prepass_bc_reference as bref
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_raster_reference as ref
import prepass_texture_reference as tref

F32 = np.float32
F64 = np.float64
MAX_ANISOTROPY = 16


def probe_count(rmin, rmax, A):
    """the contract's loop, per element: N = 1; while N < A and (double)(N N) rmin < rmax: N += 1. A NaN compares false"""
    rmin, rmax = np.asarray(rmin, F64), np.asarray(rmax, F64)
    N = np.ones(rmin.shape, np.int64)
    with np.errstate(all="ignore"):
        for n in range(1, int(A)):
            go = (N == n) & (F64(n * n) * rmin < rmax)
            N = np.where(go, n + 1, N)
    return N


def round_half_even_quotient(T, D):
    """T / D rounded half to even, in integers -> (code, tie: 2 rem == D)"""
    qd = T // D
    rem = T - qd * D
    tie = 2 * rem == D
    return qd + ((2 * rem > D) | (tie & ((qd & 1) == 1))), tie


def sample_texture(entry, texels, u, v, du_dx, dv_dx, du_dy, dv_dy, mip_bias, A, details=None):
    """one anisotropic sample per pixel -> uint32 words. u, v and the four differences: RAW"""
    import pyoracle
    _, width, height, mips = entry
    with np.errstate(all="ignore"):
        w0, h0 = F64(width), F64(height)
        axx, axy, ayx, ayy = du_dx * w0, dv_dx * h0, du_dy * w0, dv_dy * h0
        rx = axx * axx + axy * axy
        ry = ayx * ayx + ayy * ayy
        major_x = rx > ry
        rho2 = np.where(major_x, rx, ry)
        rmin = np.where(major_x, ry, rx)
        N = probe_count(rmin, rho2, A) if A >= 2 else np.ones(rx.shape, np.int64)
        du, dv = np.where(major_x, du_dx, du_dy), np.where(major_x, dv_dx, dv_dy)
        r = (rho2 / (N * N).astype(F64)).astype(F32)
        lod = (F32(0.5) * pyoracle.math_eval(1, r).reshape(r.shape)).astype(F32) + F32(mip_bias)
        lod = np.where(lod > 0, lod, F32(0)).astype(F32)
        top = F32(mips - 1)
        lod = np.where(lod > top, top, lod).astype(F32)
        q = np.floor((lod * F32(256.0)).astype(F32) + F32(0.5)).astype(np.int64)
    L0, fw = q >> 8, q & 255
    L1 = np.minimum(L0 + 1, mips - 1)
    T = np.zeros((u.size, 4), np.int64)
    fell = np.zeros(u.size, bool)
    for k in range(int(N.max(initial=1))):
        sel = np.flatnonzero(k < N)
        n = N[sel]
        with np.errstate(all="ignore"):
            t = (2 * k + 1 - n).astype(F64) / (2 * n).astype(F64)
            uk = np.where(n > 1, u[sel] + t * du[sel], u[sel])
            vk = np.where(n > 1, v[sel] + t * dv[sel], v[sel])
            valid = np.isfinite(uk) & np.isfinite(vk) & (np.abs(uk) < tref.UV_LIMIT) & (np.abs(vk) < tref.UV_LIMIT)
            uk, vk = np.where(valid, uk, F64(0)), np.where(valid, vk, F64(0))
        fell[sel] |= ~valid
        S = (256 - fw[sel])[:, None] * tref._taps(entry, texels, L0[sel], uk, vk) + fw[sel][:, None] * tref._taps(entry, texels, L1[sel], uk, vk)
        assert S.max(initial=0) <= 255 << 24
        T[sel] += S
    assert T.max(initial=0) < 1 << 36
    D = (N << 24)[:, None]
    code, tie = round_half_even_quotient(T, D)
    if details is not None:
        details.update(N=N, major_x=major_x, L0=L0, fw=fw, fell=fell, tie=tie, qd=T // D)
    return (code[:, 0] | (code[:, 1] << 8) | (code[:, 2] << 16) | (code[:, 3] << 24)).astype(np.uint32)


def _decoded(tex):
    return bref.decode_store(tex) if "formats" in tex else tex


def _winners(case, tex, keys):
    """per draw with winner pixels: (draw, pj, pi, vertex indices n x 3, V, b, and the raw u, v, du_dx, dv_dx, du_dy, dv_dy)"""
    width, height = case["width"], case["height"]
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 48)
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    uvs = np.asarray(tex["uvs"], F32).reshape(-1, 2)
    keys = np.asarray(keys, np.uint64)
    jj, ii = np.nonzero(keys)
    t = (keys[jj, ii] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    owner = np.searchsorted(first_triangle, t, side="right") - 1
    for d in np.unique(owner):
        sel = owner == d
        pj, pi = jj[sel], ii[sel]
        first, _, vertex_offset, transform_index = (int(x) for x in draws[d, :4])
        vi = indices[first + 3 * (t[sel] - first_triangle[d])[:, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset
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
            Px, Py = (2 * pi + 1).astype(F64) / F64(width) - F64(1), (2 * pj + 1).astype(F64) / F64(height) - F64(1)
            Px1, Py1 = (2 * (pi + 1) + 1).astype(F64) / F64(width) - F64(1), (2 * (pj + 1) + 1).astype(F64) / F64(height) - F64(1)
            b, bx, by = tref._barycentrics((Px, Py, one), V), tref._barycentrics((Px1, Py, one), V), tref._barycentrics((Px, Py1, one), V)
            u, v = ref._weighted(b, *tu), ref._weighted(b, *tv)
            raw = (u, v, ref._weighted(bx, *tu) - u, ref._weighted(bx, *tv) - v, ref._weighted(by, *tu) - u, ref._weighted(by, *tv) - v)
        yield int(d), pj, pi, vi, b, raw


DIAGNOSTICS = ("N", "major_x", "L0", "fw", "fell")


def sample(case, tex, keys, A, diagnostics=False):
    """-> dict(albedo, specular: uint32 h x w). diagnostics: also per output name h x w int64 arrays N, major_x, L0, fw, fell (-1 where not sampled) and `ties`:
    the qd of every channel that landed exactly on a half (2 rem == D)"""
    tex = _decoded(tex)
    height, width = case["height"], case["width"]
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    materials = np.asarray(tex["materials"], np.uint32).reshape(-1, 2)
    texels = np.asarray(tex["texels"], np.uint32).reshape(-1)
    out = dict(albedo=np.zeros((height, width), np.uint32), specular=np.zeros((height, width), np.uint32))
    diag = {name: dict({key: np.full((height, width), -1, np.int64) for key in DIAGNOSTICS}, ties=[]) for name in ("albedo", "specular")}
    for d, pj, pi, vi, b, raw in _winners(case, tex, keys):
        out["albedo"][pj, pi], out["specular"][pj, pi] = int(draws[d, 4]), int(draws[d, 5])
        if d >= materials.shape[0]:
            continue
        for column, name in enumerate(("albedo", "specular")):
            entry = tref.usable(tex, int(materials[d, column]))
            if entry is None:
                continue
            details = {}
            out[name][pj, pi] = sample_texture(entry, texels, *raw, tex["mip_bias"], A, details)
            for key in DIAGNOSTICS:
                diag[name][key][pj, pi] = details[key]
            diag[name]["ties"].extend(details["qd"][details["tie"]].tolist())
    if diagnostics:
        out["diagnostics"] = diag
    return out


def render(case, tex, cutoffs, A):
    """the alpha-tested execution: the alpha code of a fragment of triangle t at (i, j) is bits 24 - 31 of the anisotropic albedo word for that triangle at that
    pixel. Per tested triangle: rasterised alone, sampled with a key image that carries its t, masked by a >= c; the winner is the maximum of the masked keys"""
    tex = _decoded(tex)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    indices = np.asarray(case["indices"], np.uint32).reshape(-1)
    codes = aref.cutoff_codes(cutoffs)
    assert codes.size == draws.shape[0], "one cutoff per draw"
    whole = pc.rasterise(case)
    first_triangle = np.concatenate([[0], np.cumsum(draws[:, 1].astype(np.int64) // 3)])
    tested = [d for d in range(draws.shape[0]) if codes[d] != 0]
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 48)
    nothing = draws.copy()
    nothing[tested, 3] = transforms.shape[0]  # an added all-zero transform: the tested draws keep their triangles' numbers and draw nothing
    rest = pc.rasterise(dict(case, transforms=np.concatenate([transforms, np.zeros((1, 48), F32)]), draws=nothing))
    keys, motion, normal = rest["keys"].copy(), rest["motion"].copy(), rest["normal"].copy()
    for d in tested:
        for local in range(int(draws[d, 1]) // 3):
            row = draws[d].astype(np.int64)
            row[0], row[1] = row[0] + 3 * local, 3
            if row[0] + 3 > indices.size:
                continue
            single = pc.rasterise(dict(case, draws=row.astype(np.uint32).reshape(1, 6)))
            own = np.where(single["keys"] != 0, (single["keys"] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(int(first_triangle[d]) + local), np.uint64(0))
            if not (own != 0).any():
                continue
            alpha = sample(case, tex, own, A)["albedo"] >> np.uint32(24)
            better = (own != 0) & (alpha.astype(np.int64) >= codes[d]) & (own > keys)
            keys[better], motion[better], normal[better] = own[better], single["motion"][better], single["normal"][better]
    out = dict(keys=keys, depth=(keys >> np.uint64(32)).astype(np.uint32).view(F32), motion=motion, normal=normal)
    s = sample(case, tex, keys, A)
    out.update(albedo=s["albedo"], specular=s["specular"])
    out.update({name: whole[name] for name in ("submitted", "clipped", "drawn", "rejects")})
    return out


def base_images(case, tex, cutoffs, A, diagnostics=False):
    """the five images, keys and counters of an execution without normal maps"""
    if cutoffs is not None:
        out = render(case, tex, cutoffs, A)
        if diagnostics:
            out["diagnostics"] = sample(case, tex, out["keys"], A, diagnostics=True)["diagnostics"]
        return out
    r = pc.rasterise(case)
    s = sample(case, tex, r["keys"], A, diagnostics=diagnostics)
    return dict(r, **s)


def shade(case, tex, nm, keys, normal, A, details=None):
    """-> shadingNormal uint32 h x w: the normal map contract with the anisotropic texel. details: receives the sampler's diagnostics as h x w arrays"""
    tex = _decoded(tex)
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 48)
    positions = np.asarray(case["positions"], F32).reshape(-1, 3)
    normals = np.asarray(case["normals"], F32).reshape(-1, 3)
    draws = np.asarray(case["draws"], np.uint32).reshape(-1, 6)
    texels = np.asarray(tex["texels"], np.uint32).reshape(-1)
    words = np.asarray(nm["normal_materials"], np.uint32).reshape(-1)
    decode = int(nm["decode"])
    keys = np.asarray(keys, np.uint64)
    out = np.where(keys != 0, np.asarray(normal, np.uint32), np.uint32(0)).astype(np.uint32)
    diag = {key: np.full(keys.shape, -1, np.int64) for key in DIAGNOSTICS}
    for d, pj, pi, vi, b, raw in _winners(case, tex, keys):
        if d >= words.size:
            continue
        entry = tref.usable(tex, int(words[d]))
        if entry is None:
            continue
        sampled = {}
        texel = sample_texture(entry, texels, *raw, tex["mip_bias"], A, sampled)
        for key in DIAGNOSTICS:
            diag[key][pj, pi] = sampled[key]
        model = transforms[int(draws[d, 3]), 0:16].astype(F64)
        with np.errstate(all="ignore"):
            nt = nref.decode_texel(texel & np.uint32(255), (texel >> np.uint32(8)) & np.uint32(255), decode)
            p64 = [positions[vi[:, k]].astype(F64) for k in range(3)]
            a, c = p64[0] - p64[2], p64[0] - p64[1]
            face = ref._normalized(a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0])
            N, T, B = [], [], []
            for k in range(3):
                stored = normals[vi[:, k]]
                zero = (stored == 0).all(axis=1)
                N.append(ref._normalized(*nref._rotate(model, [np.where(zero, face[i], stored[:, i].astype(F64)) for i in range(3)])))
                T.append(ref._normalized(*nref._rotate(model, nref._fetch3(nm["tangents"], vi[:, k]))))
                B.append(ref._normalized(*nref._rotate(model, nref._fetch3(nm["bitangents"], vi[:, k]))))
            Ti, Bi, Nv = ([ref._weighted(b, X[0][r], X[1][r], X[2][r]) for r in range(3)] for X in (T, B, N))
            ns = ref._normalized(*[(Ti[r] * nt[0] + Bi[r] * nt[1]) + Nv[r] * nt[2] for r in range(3)])
            is_zero = (ns[0] == 0) & (ns[1] == 0) & (ns[2] == 0)
            word = ref._unorm8_half(ns[0]) | (ref._unorm8_half(ns[1]) << np.uint32(8)) | (ref._unorm8_half(ns[2]) << np.uint32(16)) | np.uint32(255 << 24)
        out[pj, pi] = np.where(is_zero, out[pj, pi], word)
    if details is not None:
        details.update(diag)
    return out
