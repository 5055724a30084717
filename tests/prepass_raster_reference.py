"""numpy reference of the "depthPrepassRaster.comp" pass, written from the contract text (DESIGN.md "Depth prepass as a compute pass";
csrc/kernels/depth_prepass_raster.hip implements the same contract independently and must agree bit for bit on all five images and all counters).

Every fp32 operation is one IEEE operation on np.float32 values, every fp64 operation one on np.float64, sums are written out in the contract's order (no `@`, no
np.sum, no np.linalg), edge functions and areas are Python or int64 integers. Clipping is a scalar loop per triangle that needs it; coverage is vectorised over a
sub-triangle's pixel box; the attributes are vectorised over all pixels that have a winner.

Buffers: transforms n x 48 float32 ({model, mvp, mvpPrevious}, glm column-major), positions and normals v x 3, indices uint32, draws d x 6 uint32
{firstIndex, indexCount, vertexOffset, transformIndex, albedo, specular}.
"""
import numpy as np

F32 = np.float32
F64 = np.float64
GUARD_NDC = F32(32.0)
BAND_PIXELS = F32(1048576.0)  # 2^20
HALF = F32(0.5)


def transform4(m, p):
    """clip = M * (p, 1) for n x 3 positions -> n x 4: m[0][i] x + m[1][i] y + m[2][i] z + m[3][i], summed left to right"""
    m = np.asarray(m, F32).reshape(16)
    p = np.asarray(p, F32).reshape(-1, 3)
    out = np.zeros((p.shape[0], 4), F32)
    with np.errstate(all="ignore"):
        for i in range(4):
            s = m[0 * 4 + i] * p[:, 0]
            s = s + m[1 * 4 + i] * p[:, 1]
            s = s + m[2 * 4 + i] * p[:, 2]
            s = s + m[3 * 4 + i]
            out[:, i] = s
    return out


def plane_distance(plane, v):
    """the five clip planes in their order: near w - z, then 32 w - x, 32 w + x, 32 w - y, 32 w + y; v: (..., 4) float32"""
    x, y, z, w = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
    with np.errstate(all="ignore"):
        if plane == 0:
            return w - z
        g = GUARD_NDC * w
        return (g - x, g + x, g - y, g + y)[plane - 1]


def clip_triangle(v):
    """Sutherland-Hodgman of one triangle (3 x 4 float32 clip vertices) -> (list of float32[4] vertices, clipped)"""
    poly = [v[0], v[1], v[2]]
    clipped = False
    with np.errstate(all="ignore"):
        for plane in range(5):
            cap = 4 + plane
            n = len(poly)
            d = [plane_distance(plane, q) for q in poly]
            out = []
            for i in range(n):
                j = (i + 1) % n
                ina, inb = bool(d[i] >= 0), bool(d[j] >= 0)
                if not ina:
                    clipped = True
                if ina and len(out) < cap:
                    out.append(poly[i])
                if ina != inb and len(out) < cap:  # from the inside vertex towards the outside one
                    I, O, di, do = (poly[i], poly[j], d[i], d[j]) if ina else (poly[j], poly[i], d[j], d[i])
                    t = F32(di / F32(di - do))
                    out.append((I + t * (O - I)).astype(F32))
            poly = out
    return poly, clipped


def project(v, width, height):
    """clip vertices (n x 4) -> X, Y (int64, 8 sub-pixel bits; 0 where not ok), z = clip.z / w, ok"""
    v = np.asarray(v, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        w = v[:, 3]
        nx, ny, nz = v[:, 0] / w, v[:, 1] / w, v[:, 2] / w
        xf = (nx * HALF + HALF) * F32(width)
        yf = (ny * HALF + HALF) * F32(height)
        ok = (w > 0) & (np.abs(xf) < BAND_PIXELS) & (np.abs(yf) < BAND_PIXELS) & np.isfinite(nz)
        X = np.rint(np.where(ok, xf, F32(0)) * F32(256.0)).astype(np.int64)
        Y = np.rint(np.where(ok, yf, F32(0)) * F32(256.0)).astype(np.int64)
    return X, Y, nz, ok


def _normalized(x, y, z):
    """v / sqrt((x x + y y) + z z) in fp64, (0, 0, 0) where the length is not a finite number > 0"""
    with np.errstate(all="ignore"):
        length = np.sqrt((x * x + y * y) + z * z)
        good = (length > 0) & np.isfinite(length)
        safe = np.where(good, length, F64(1.0))
        return np.where(good, x / safe, F64(0)), np.where(good, y / safe, F64(0)), np.where(good, z / safe, F64(0))


def _det(a, b, c):
    """det of three (x, y, w) triples in the contract's order"""
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def _weighted(b, a0, a1, a2):
    return (b[0] * a0 + b[1] * a1) + b[2] * a2


def _unorm8_half(n):
    """n (fp64) rounded once to fp32, n * 0.5 + 0.5, the image contract's UNORM8 rule"""
    with np.errstate(all="ignore"):
        v = n.astype(F32) * HALF + HALF
        code = np.rint(np.fmin(np.fmax(v, F32(0)), F32(1)) * F32(255.0))
    return np.where(np.isnan(v), 0, code).astype(np.uint32)


def _snorm16(m):
    with np.errstate(all="ignore"):
        m = m.astype(F32)
        code = np.rint(np.fmin(np.fmax(m, F32(-1)), F32(1)) * F32(32767.0))
    return np.where(np.isnan(m), 0, code).astype(np.int16)


def rasterise(transforms, positions, normals, indices, draws, width, height, jitter_current=(0.0, 0.0), jitter_previous=(0.0, 0.0), diagnostics=False):
    """-> dict(depth float32 h x w, motion int16 h x w x 2, normal / albedo / specular uint32 h x w, keys uint64 h x w, coverage int32 h x w (kept fragments
    per pixel), weights float64 n x 3 (the barycentrics of the pixels with a winner, row-major order), submitted, clipped, drawn, rejects).
    diagnostics: also polygons [(t, vertices of its clipped polygon)] for every triangle that reaches the clipper, fan_drawn [(t, fan index, (ix0, iy0, ix1,
    iy1), (x span, y span in sub-pixel units))] for every sub-triangle counted as drawn, in submission order, and fan_rejected [(t, fan index)]. An added output:
    nothing else depends on it"""
    width, height = int(width), int(height)
    transforms = np.asarray(transforms, F32).reshape(-1, 48)
    positions = np.asarray(positions, F32).reshape(-1, 3)
    normals = np.asarray(normals, F32).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32).reshape(-1)
    draws = np.asarray(draws, np.uint32).reshape(-1, 6)
    vertex_count = min(positions.shape[0], normals.shape[0])
    keys = np.zeros((height, width), np.uint64)
    coverage = np.zeros((height, width), np.int32)
    submitted = clipped_count = drawn = rejects = 0
    origin_draw, origin_vertices = [], []  # per submitted triangle: its draw and its three vertices (-1 where it is outside its buffers)
    polygons, fan_drawn, fan_rejected = [], [], []
    t_next = 0
    for d, (first, count, vertex_offset, transform_index, _, _) in enumerate(draws.tolist()):
        n = count // 3
        submitted += n
        t_first = t_next
        t_next += n
        slot = first + 3 * np.arange(n, dtype=np.int64)
        in_buffers = (slot + 3 <= indices.size) & (transform_index < transforms.shape[0])
        idx = np.full((n, 3), -1, np.int64)
        idx[in_buffers] = indices[slot[in_buffers, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset
        in_buffers &= (idx < vertex_count).all(axis=1) & (idx >= 0).all(axis=1)
        idx[~in_buffers] = -1
        origin_draw.append(np.full(n, d, np.int64))
        origin_vertices.append(idx)
        rejects += int((~in_buffers).sum())
        if not in_buffers.any():
            continue
        live = np.flatnonzero(in_buffers)
        clip = transform4(transforms[transform_index, 16:32], positions[idx[live].reshape(-1)]).reshape(-1, 3, 4)
        finite = np.isfinite(clip).all(axis=(1, 2))
        rejects += int((~finite).sum())
        with np.errstate(all="ignore"):
            inside_all = np.ones(clip.shape[0], bool)
            for plane in range(5):
                inside_all &= (plane_distance(plane, clip) >= 0).all(axis=1)
        for k in np.flatnonzero(finite):
            t = t_first + int(live[k])
            if inside_all[k]:
                poly, was_clipped = [clip[k, 0], clip[k, 1], clip[k, 2]], False  # a triangle fully inside comes through unchanged
            else:
                poly, was_clipped = clip_triangle(clip[k])
            clipped_count += int(was_clipped)
            if diagnostics:
                polygons.append((t, len(poly)))
            if len(poly) < 3:
                continue
            X, Y, z, ok = project(np.stack(poly), width, height)
            for s in range(len(poly) - 2):
                corners = (0, s + 1, s + 2)
                if not all(ok[c] for c in corners):
                    rejects += 1
                    if diagnostics:
                        fan_rejected.append((t, s))
                    continue
                (x0, x1, x2), (y0, y1, y2) = (int(X[c]) for c in corners), (int(Y[c]) for c in corners)
                area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
                if area >= 0:  # back faces (A > 0) are culled, A == 0 covers nothing
                    continue
                # rasterised as (v0, v2, v1): A' = -A > 0, by the shadow contract
                corners = (0, s + 2, s + 1)
                (x0, x1, x2), (y0, y1, y2) = (int(X[c]) for c in corners), (int(Y[c]) for c in corners)
                z0, z1, z2 = (z[c] for c in corners)
                area = -area
                ix0, ix1 = max(0, (min(x0, x1, x2) + 127) >> 8), min(width - 1, (max(x0, x1, x2) - 128) >> 8)
                iy0, iy1 = max(0, (min(y0, y1, y2) + 127) >> 8), min(height - 1, (max(y0, y1, y2) - 128) >> 8)
                if ix0 > ix1 or iy0 > iy1:
                    continue
                drawn += 1
                if diagnostics:
                    fan_drawn.append((t, s, (ix0, iy0, ix1, iy1), (max(x0, x1, x2) - min(x0, x1, x2), max(y0, y1, y2) - min(y0, y1, y2))))
                px = (np.arange(ix0, ix1 + 1, dtype=np.int64) * 256 + 128)[None, :]
                py = (np.arange(iy0, iy1 + 1, dtype=np.int64) * 256 + 128)[:, None]
                covered = np.ones((iy1 - iy0 + 1, ix1 - ix0 + 1), bool)
                E = []
                for (xa, ya), (xb, yb) in (((x0, y0), (x1, y1)), ((x1, y1), (x2, y2)), ((x2, y2), (x0, y0))):
                    dx, dy = xb - xa, yb - ya
                    e = dx * (py - ya) - dy * (px - xa)
                    top_left = (dy == 0 and dx > 0) or dy < 0
                    covered &= (e > 0) | ((e == 0) & top_left)
                    E.append(e)
                if not covered.any():
                    continue
                fa = F32(area)
                with np.errstate(all="ignore"):
                    l1 = E[2].astype(F32) / fa
                    l2 = E[0].astype(F32) / fa
                    dz1, dz2 = F32(z1 - z0), F32(z2 - z0)
                    zf = ((z0 + l1 * dz1) + l2 * dz2).astype(F32)
                    keep = covered & (zf > 0)  # a NaN, and everything at or beyond the far plane, is dropped
                key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
                sub = keys[iy0:iy1 + 1, ix0:ix1 + 1]
                sub[...] = np.where(keep, np.maximum(sub, key), sub)
                coverage[iy0:iy1 + 1, ix0:ix1 + 1] += keep
    out = dict(keys=keys, coverage=coverage, submitted=submitted, clipped=clipped_count, drawn=drawn, rejects=rejects)
    if diagnostics:
        out.update(polygons=polygons, fan_drawn=fan_drawn, fan_rejected=fan_rejected)
    out["depth"] = (keys >> np.uint64(32)).astype(np.uint32).view(F32)
    motion = np.zeros((height, width, 2), np.int16)
    normal = np.zeros((height, width), np.uint32)
    albedo = np.zeros((height, width), np.uint32)
    specular = np.zeros((height, width), np.uint32)
    out.update(motion=motion, normal=normal, albedo=albedo, specular=specular, weights=np.zeros((0, 3), F64))
    jj, ii = np.nonzero(keys)
    if jj.size == 0:
        return out
    t = (keys[jj, ii] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    tri_draw, tri_vertices = np.concatenate(origin_draw), np.concatenate(origin_vertices)
    dr = draws[tri_draw[t]]
    vi = tri_vertices[t]  # n x 3
    T = transforms[dr[:, 3].astype(np.int64)]
    model, mvp, mvp_previous = T[:, 0:16], T[:, 16:32], T[:, 32:48]

    def clip_of(m, p):  # per-pixel matrices: component i of M * (p, 1)
        with np.errstate(all="ignore"):
            return [((m[:, 0 * 4 + i] * p[:, 0] + m[:, 1 * 4 + i] * p[:, 1]) + m[:, 2 * 4 + i] * p[:, 2]) + m[:, 3 * 4 + i] for i in range(4)]

    pos = [positions[vi[:, k]] for k in range(3)]
    V, prev = [], []
    for k in range(3):
        c = clip_of(mvp, pos[k])
        V.append((c[0].astype(F64), c[1].astype(F64), c[3].astype(F64)))
        c = clip_of(mvp_previous, pos[k])
        prev.append((c[0].astype(F64), c[1].astype(F64), c[3].astype(F64)))
    with np.errstate(all="ignore"):
        P = ((2 * ii + 1).astype(F64) / F64(width) - F64(1), (2 * jj + 1).astype(F64) / F64(height) - F64(1), np.ones(ii.size, F64))
        e = [_det(P, V[1], V[2]), _det(P, V[2], V[0]), _det(P, V[0], V[1])]
        s = (e[0] + e[1]) + e[2]
        good = (s != 0) & np.isfinite(s)
        safe = np.where(good, s, F64(1))
        b = [np.where(good, e[0] / safe, F64(1)), np.where(good, e[1] / safe, F64(0)), np.where(good, e[2] / safe, F64(0))]
        out["weights"] = np.stack(b, axis=1)
        # normal
        p64 = [p.astype(F64) for p in pos]
        a = p64[0] - p64[2]
        c = p64[0] - p64[1]
        face = _normalized(a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0])
        m64 = model.astype(F64)
        N = []
        for k in range(3):
            stored = normals[vi[:, k]]
            zero = (stored == 0).all(axis=1)
            nx, ny, nz = (np.where(zero, face[i], stored[:, i].astype(F64)) for i in range(3))
            N.append(_normalized(*[(m64[:, 0 * 4 + r] * nx + m64[:, 1 * 4 + r] * ny) + m64[:, 2 * 4 + r] * nz for r in range(3)]))
        n = _normalized(*[_weighted(b, N[0][i], N[1][i], N[2][i]) for i in range(3)])
        normal[jj, ii] = _unorm8_half(n[0]) | (_unorm8_half(n[1]) << np.uint32(8)) | (_unorm8_half(n[2]) << np.uint32(16)) | np.uint32(255 << 24)
        # motion
        ws = _weighted(b, prev[0][2], prev[1][2], prev[2][2])
        valid = (ws > 0) & np.isfinite(ws)
        safe = np.where(valid, ws, F64(1))
        jc, jp = [F64(F32(v)) for v in jitter_current], [F64(F32(v)) for v in jitter_previous]
        for axis in range(2):
            previous = _weighted(b, prev[0][axis], prev[1][axis], prev[2][axis]) / safe + jp[axis]
            current = P[axis] + jc[axis]
            motion[jj, ii, axis] = np.where(valid, _snorm16((previous - current) * F64(0.5)), 0)
    albedo[jj, ii] = dr[:, 4]
    specular[jj, ii] = dr[:, 5]
    return out


def mat_mul(a, b):
    """(A * B) for glm column-major 16-float arrays in fp32: element [c][r] = a[0][r] b[c][0] + a[1][r] b[c][1] + a[2][r] b[c][2] + a[3][r] b[c][3], left to right"""
    a = np.asarray(a, F32).reshape(16)
    b = np.asarray(b, F32).reshape(16)
    m = np.zeros(16, F32)
    with np.errstate(all="ignore"):
        for c in range(4):
            for r in range(4):
                s = F32(a[0 * 4 + r] * b[c * 4 + 0])
                for k in range(1, 4):
                    s = F32(s + F32(a[k * 4 + r] * b[c * 4 + k]))
                m[c * 4 + r] = s
    return m


def main_pass_matrices(view_projection, view_projection_previous, models, models_previous=None):
    """n x 48 float32: {model, mvp = viewProjection * model, mvpPrevious = viewProjectionPrevious * previousModel} per draw"""
    models = np.asarray(models, F32).reshape(-1, 16)
    models_previous = models if models_previous is None else np.asarray(models_previous, F32).reshape(-1, 16)
    return np.stack([np.concatenate([m, mat_mul(view_projection, m), mat_mul(view_projection_previous, mp)]) for m, mp in zip(models, models_previous)]).astype(F32)


def face_normals(positions, indices):
    """the contract's face normal per triangle in fp64: normalize(cross(v0 - v2, v0 - v1))"""
    p = np.asarray(positions, F32).reshape(-1, 3).astype(F64)[np.asarray(indices, np.int64).reshape(-1, 3)]
    a, c = p[:, 0] - p[:, 2], p[:, 0] - p[:, 1]
    return np.stack(_normalized(a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]), axis=1)
