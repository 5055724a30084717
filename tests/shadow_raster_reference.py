"""numpy reference of the "sunShadowRaster.comp" pass (DESIGN.md "Sun shadow cascades as a compute pass"; csrc/kernels/sun_shadow_raster.hip implements the
same contract independently and must agree bit for bit).

Every float operation is one fp32 IEEE operation on np.float32 arrays, sums are written out left to right (no `@`, no np.sum), edge functions are int64.
The loop is over triangles, each vectorised over its pixel box.

Outside a buffer: a triangle counts as submitted and as a reject, and draws nothing, when its three index slots are not all inside `indices`, when a vertex
(index + vertexOffset, in 64 bits) is not inside `positions`, or when its draw's transformIndex is not inside `transforms`. A draw submits indexCount // 3
triangles, whatever becomes of them.
The depth clamp is fmin(fmax(zf, 0), 1) with IEEE maxNum / minNum semantics (np.fmax / np.fmin): a NaN zf stores code 0, +inf stores 65535.
"""
import numpy as np

F32 = np.float32
TILE = 64
GUARD_BAND_PIXELS = F32(1048576.0)  # 2^20


def mat_mul(a, b):
    """(A * B) for glm column-major 16-float arrays: element [c][r] = a[0][r] b[c][0] + a[1][r] b[c][1] + a[2][r] b[c][2] + a[3][r] b[c][3], left to right"""
    a = np.asarray(a, F32).reshape(16)
    b = np.asarray(b, F32).reshape(16)
    m = np.zeros(16, F32)
    for c in range(4):
        for r in range(4):
            s = F32(a[0 * 4 + r] * b[c * 4 + 0])
            s = F32(s + F32(a[1 * 4 + r] * b[c * 4 + 1]))
            s = F32(s + F32(a[2 * 4 + r] * b[c * 4 + 2]))
            s = F32(s + F32(a[3 * 4 + r] * b[c * 4 + 3]))
            m[c * 4 + r] = s
    return m


def transform(m, p):
    """clip = M * (p, 1) for n x 3 positions -> n x 3 (x, y, z; w is not needed): m[0][i] x + m[1][i] y + m[2][i] z + m[3][i], left to right"""
    p = np.asarray(p, F32)
    out = np.zeros((p.shape[0], 3), F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            s = m[0 * 4 + i] * p[:, 0]
            s = s + m[1 * 4 + i] * p[:, 1]
            s = s + m[2 * 4 + i] * p[:, 2]
            s = s + m[3 * 4 + i]
            out[:, i] = s
    return out


def is_affine(m):
    m = np.asarray(m, F32).reshape(16)
    return m[3] == 0 and m[7] == 0 and m[11] == 0 and m[15] == 1


def project(light_matrix, model_matrix, positions, res):
    """n x 3 positions -> (X, Y int64 with 8 sub-pixel bits, z float32, inside the guard band and finite); X and Y are 0 where `inside` is false"""
    clip = transform(mat_mul(light_matrix, model_matrix), positions)
    resf = F32(res)
    with np.errstate(all="ignore"):
        xf = (clip[:, 0] * F32(0.5) + F32(0.5)) * resf
        yf = (clip[:, 1] * F32(0.5) + F32(0.5)) * resf
        z = clip[:, 2]
        inside = np.isfinite(z) & (np.abs(xf) < GUARD_BAND_PIXELS) & (np.abs(yf) < GUARD_BAND_PIXELS)  # a NaN or an infinity fails the comparison
        X = np.rint(np.where(inside, xf, F32(0)) * F32(256.0)).astype(np.int64)
        Y = np.rint(np.where(inside, yf, F32(0)) * F32(256.0)).astype(np.int64)
    return X, Y, z, inside


def clamp01(zf):
    """the depth clamp: fmin(fmax(zf, 0), 1) with IEEE maxNum / minNum semantics - of a NaN and a number the number. A NaN zf becomes 0, +inf becomes 1"""
    return np.fmin(np.fmax(zf, F32(0.0)), F32(1.0))


def rasterise(light_matrix, transforms, positions, indices, draws, res):
    """light_matrix: 16 floats; transforms: n x 16; positions: v x 3; indices: uint32; draws: d x 4 {firstIndex, indexCount, vertexOffset, transformIndex}.
    -> dict(map uint16 res x res, coverage int32 res x res (fragments per texel), submitted, drawn, rejects)"""
    res = int(res)
    positions = np.asarray(positions, F32).reshape(-1, 3)
    indices = np.asarray(indices, np.uint32).reshape(-1)
    transforms = np.asarray(transforms, F32).reshape(-1, 16)
    draws = np.asarray(draws, np.uint32).reshape(-1, 4)
    depth = np.zeros((res, res), np.uint16)
    coverage = np.zeros((res, res), np.int32)
    submitted = drawn = rejects = 0
    for first, count, vertex_offset, transform_index in draws.tolist():
        n = count // 3
        submitted += n
        # outside a buffer (module docstring): index slots, vertices (64-bit sums), the draw's transform slot
        slot = first + 3 * np.arange(n, dtype=np.int64)
        in_buffers = (slot + 3 <= indices.size) & (transform_index < transforms.shape[0])
        idx = np.zeros((n, 3), np.int64)
        idx[in_buffers] = indices[slot[in_buffers, None] + np.arange(3)[None, :]].astype(np.int64) + vertex_offset
        in_buffers &= (idx < positions.shape[0]).all(axis=1)
        rejects += int((~in_buffers).sum())
        if not in_buffers.any():
            continue
        idx = idx[in_buffers]
        X, Y, z, inside = project(light_matrix, transforms[transform_index], positions[idx.reshape(-1)], res)
        X, Y, z, inside = X.reshape(-1, 3), Y.reshape(-1, 3), z.reshape(-1, 3), inside.reshape(-1, 3)
        ok = inside.all(axis=1)
        rejects += int((~ok).sum())
        for t in np.flatnonzero(ok):
            x0, x1, x2 = (int(v) for v in X[t])
            y0, y1, y2 = (int(v) for v in Y[t])
            area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            if area <= 0:  # front faces (A < 0) are culled, A == 0 covers nothing
                continue
            # pixel centres 256 i + 128 inside [min, max], clipped to the map
            ix0, ix1 = max(0, (min(x0, x1, x2) + 127) >> 8), min(res - 1, (max(x0, x1, x2) - 128) >> 8)
            iy0, iy1 = max(0, (min(y0, y1, y2) + 127) >> 8), min(res - 1, (max(y0, y1, y2) - 128) >> 8)
            if ix0 > ix1 or iy0 > iy1:
                continue
            drawn += 1
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
            fa = F32(area)  # int64 -> fp32, round to nearest even
            l1 = E[2].astype(F32) / fa
            l2 = E[0].astype(F32) / fa
            z0 = z[t, 0]
            with np.errstate(all="ignore"):  # z1 - z0 may overflow to an infinity, and 0 * inf is a NaN
                dz1, dz2 = F32(z[t, 1] - z0), F32(z[t, 2] - z0)
                zf = (z0 + l1 * dz1) + l2 * dz2
            zf = clamp01(zf)
            code = np.rint(zf * F32(65535.0)).astype(np.uint16)
            sub = depth[iy0:iy1 + 1, ix0:ix1 + 1]
            sub[...] = np.where(covered, np.maximum(sub, code), sub)
            coverage[iy0:iy1 + 1, ix0:ix1 + 1] += covered
    return dict(map=depth, coverage=coverage, submitted=submitted, drawn=drawn, rejects=rejects)


def merge_meshes(meshes, draw_list):
    """meshes: [(positions n x 3, indices)], draw_list: [(mesh, 16 floats)] -> positions, indices, draws (d x 4 uint32), transforms (d x 16): the pass' buffers
    2, 3, 4 and 1, laid out the way plrf_set_shadow_casters lays them out (meshes back to back, one transform per draw)"""
    first, base, pos, idx = [], [], [], []
    nv = ni = 0
    for p, i in meshes:
        p = np.asarray(p, F32).reshape(-1, 3)
        i = np.asarray(i, np.uint32).reshape(-1)
        first.append(ni); base.append(nv)
        pos.append(p); idx.append(i)
        nv += p.shape[0]; ni += i.size
    draws = np.array([[first[m], np.asarray(meshes[m][1]).size, base[m], d] for d, (m, _) in enumerate(draw_list)], np.uint32).reshape(-1, 4)
    transforms = np.array([np.asarray(t, F32).reshape(16) for _, t in draw_list], F32).reshape(-1, 16)
    return np.concatenate(pos), np.concatenate(idx), draws, transforms


def light_matrices(shadow_info_bytes):
    """the four 16-float light matrices of a 304-byte sunShadowInfo block (sunShadowCascades.inc:7-11)"""
    return np.frombuffer(bytes(shadow_info_bytes), F32, 64, 16).reshape(4, 16).copy()
