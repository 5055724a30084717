"""numpy restatement of "sdfInstanceUpdate.comp" and "sceneMeanAlbedo.comp", written from the contract text (DESIGN.md "SDF instances from the scene";
csrc/kernels/scene_sdf.hip and csrc/device/scene_sdf.h implement the same contract independently and must agree byte for byte).

THE INSTANCE CONTRACT. fp32 IEEE operations in the order written, no contraction; fp64 where named. A model matrix is 16 floats, glm column-major: element
[c][r] at 4 c + r.
  min(a, v) = v if v < a else a;  max(a, v) = v if a < v else a
  padded box        pad = max(0.075f (max - min), 0.5f) per component; min - pad, max + pad
  row rule          row i of model (x, y, z, 1) = ((m[0][i] x + m[1][i] y) + m[2][i] z) + m[3][i]
  world box         rows 0 - 2 of the eight corners of the UNPADDED local box, corner k taking max on the axes whose bit of k is set; component min / max over k
                    ascending, starting from corner 0; then the padding rule
  localToWorld      model translate(bbOffset), bbOffset = (paddedMin + paddedMax) 0.5f: columns 0 - 2 are model's, column 3 is the row rule at bbOffset, rows 0 - 3
  worldToLocal      a[i][j] = double(L[4 i + j]); s0 .. s5 the 2 x 2 sub-determinants a[0][p] a[1][q] - a[1][p] a[0][q] for (p, q) = 01 02 03 12 13 23, c0 .. c5 the
                    same of rows 2 and 3; det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0; the sixteen adjugate elements as ADJUGATE lists them, each
                    (p q - r s) + t u or (p q - r s) - t u; element = float(b / det): one division, one rounding
  record            {localExtends = paddedMax - paddedMin, sdfTextureIndex, meanAlbedo, 0, worldToLocal}, 96 bytes; world box {min, 0, max, 0}, 32 bytes
  meanAlbedo        the draw's override where its red is not a NaN; else the mean of the draw's albedo texture; else the mean albedo rule on the draw's constant word

THE MEAN ALBEDO CONTRACT. term_c = uint(trunc(float(c) (float(a) / 255.f))) per texel and channel r, g, b; S_c the exact sum; mean_c = (float(S_c) / 255.f) /
float(texelCount); {r, g, b, 0}. Compressed levels are decoded by tests/prepass_bc_reference.py (BC1 alpha 255, BC5 (R, G, 0, 255)), cropped to the level's size.
"""
import struct

import numpy as np

import prepass_bc_reference as bref

F32, F64, U32 = np.float32, np.float64, np.uint32
NONE = 0xFFFFFFFF
INSTANCE_BYTES, HEADER_BYTES, BB_BYTES = 96, 16, 32


def _min(a, v):
    return np.where(v < a, v, a).astype(F32)


def _max(a, v):
    return np.where(a < v, v, a).astype(F32)


def padded_box(mn, mx):
    mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
    pad = _max(F32(0.075) * (mx - mn), F32(0.5))
    return (mn - pad).astype(F32), (mx + pad).astype(F32)


def row(m, i, x, y, z):
    m = np.asarray(m, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(F32(F32(F32(m[i] * F32(x)) + F32(m[4 + i] * F32(y))) + F32(m[8 + i] * F32(z))) + m[12 + i])


def world_box(model, mn, mx):
    mn, mx = np.asarray(mn, F32), np.asarray(mx, F32)
    lo = hi = None
    for k in range(8):
        corner = [mx[a] if (k >> a) & 1 else mn[a] for a in range(3)]
        v = np.array([row(model, i, *corner) for i in range(3)], F32)
        lo, hi = (v, v) if k == 0 else (_min(lo, v), _max(hi, v))
    return padded_box(lo, hi)


def local_to_world(model, padded_mn, padded_mx):
    out = np.asarray(model, F32).copy()
    offset = ((padded_mn + padded_mx) * F32(0.5)).astype(F32)
    for i in range(4):
        out[12 + i] = row(model, i, *offset)
    return out


def _sub_determinants(m):
    a = np.asarray(m, F32).astype(F64)
    pairs = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    s = [a[p] * a[4 + q] - a[4 + p] * a[q] for p, q in pairs]
    c = [a[8 + p] * a[12 + q] - a[12 + p] * a[8 + q] for p, q in pairs]
    return a, s, c


def determinant(m):
    with np.errstate(over="ignore", invalid="ignore"):
        _, s, c = _sub_determinants(m)
        return ((((s[0] * c[5] - s[1] * c[4]) + s[2] * c[3]) + s[3] * c[2]) - s[4] * c[1]) + s[5] * c[0]


# element e of the adjugate: (a[p] X[i] - a[q] X[j]) sign a[r] X[k], X = c for the elements of columns 0 and 1 of each row group, s for the others
ADJUGATE = (
    (5, "c", 5, 6, "c", 4, +1, 7, "c", 3), (2, "c", 4, 1, "c", 5, -1, 3, "c", 3), (13, "s", 5, 14, "s", 4, +1, 15, "s", 3), (10, "s", 4, 9, "s", 5, -1, 11, "s", 3),
    (6, "c", 2, 4, "c", 5, -1, 7, "c", 1), (0, "c", 5, 2, "c", 2, +1, 3, "c", 1), (14, "s", 2, 12, "s", 5, -1, 15, "s", 1), (8, "s", 5, 10, "s", 2, +1, 11, "s", 1),
    (4, "c", 4, 5, "c", 2, +1, 7, "c", 0), (1, "c", 2, 0, "c", 4, -1, 3, "c", 0), (12, "s", 4, 13, "s", 2, +1, 15, "s", 0), (9, "s", 2, 8, "s", 4, -1, 11, "s", 0),
    (5, "c", 1, 4, "c", 3, -1, 6, "c", 0), (0, "c", 3, 1, "c", 1, +1, 2, "c", 0), (13, "s", 1, 12, "s", 3, -1, 14, "s", 0), (8, "s", 3, 9, "s", 1, +1, 10, "s", 0),
)


def inverse(m):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a, s, c = _sub_determinants(m)
        det = ((((s[0] * c[5] - s[1] * c[4]) + s[2] * c[3]) + s[3] * c[2]) - s[4] * c[1]) + s[5] * c[0]
        x = dict(s=s, c=c)
        out = np.zeros(16, F32)
        for e, (p, xi, i, q, xj, j, sign, r, xk, k) in enumerate(ADJUGATE):
            first = a[p] * x[xi][i] - a[q] * x[xj][j]
            b = first + a[r] * x[xk][k] if sign > 0 else first - a[r] * x[xk][k]
            out[e] = F32(b / det)
        return out


def instance_determinant(model, mn, mx):
    return determinant(local_to_world(model, *padded_box(mn, mx)))


def mean_albedo_sums(words):
    """RGBA8 words, R in the low byte -> the three exact integer sums"""
    w = np.asarray(words, U32).reshape(-1)
    alpha = ((w >> U32(24)) & U32(255)).astype(F32) / F32(255)
    return [int(((((w >> U32(8 * c)) & U32(255)).astype(F32) * alpha).astype(F32)).astype(np.uint64).sum()) for c in range(3)]


def mean_of_sums(sums, texel_count):
    return np.array([F32(F32(F32(np.uint64(s)) / F32(255)) / F32(U32(texel_count))) for s in sums] + [F32(0)], F32)


def mean_albedo(words):
    w = np.asarray(words, U32).reshape(-1)
    return mean_of_sums(mean_albedo_sums(w), w.size)


def level0_words(table_row, fmt, words):
    """level 0 of one row of a texture store as RGBA8 words (row-major, cropped to the level)"""
    offset, width, height = int(table_row[0]), int(table_row[1]), int(table_row[2])
    n = bref.level_words(fmt, width, height)
    level = np.asarray(words, U32)[offset:offset + n]
    return level if fmt == bref.RGBA8 else bref.decode_level(fmt, width, height, level.tobytes()).reshape(-1)


def mean_albedo_pass(table, words, formats, materials, prefill):
    """the mean albedo buffer after the pass: T x 4 float32 from `prefill`, the entries of the textures some draw names as albedo replaced"""
    table = np.asarray(table, U32).reshape(-1, 4)
    out = np.asarray(prefill, F32).reshape(-1, 4).copy()
    named = {int(a) for a, _ in np.asarray(materials, U32).reshape(-1, 2) if int(a) < table.shape[0]}
    for t in sorted(named):
        fmt = int(formats[t]) if formats is not None else bref.RGBA8
        out[t] = mean_albedo(level0_words(table[t], fmt, words))
    return out


def instance_pass(case):
    """-> (instance buffer bytes, world box buffer bytes) after the pass, from the case's prefilled buffers.
    case: models (D x 16), table [(draw, sdf texture index, local min, local max)], albedo_words (D), overrides (D x 3), materials (D x 2) or None, means (T x 4) or
    None, instances_prefill / bbs_prefill (bytes)"""
    inst, bbs = bytearray(case["instances_prefill"]), bytearray(case["bbs_prefill"])
    table = case["table"]
    inst[0:16] = struct.pack("<4I", len(table), 0, 0, 0)
    models = np.asarray(case["models"], F32).reshape(-1, 16)
    textures = 0 if case.get("means") is None else np.asarray(case["means"]).reshape(-1, 4).shape[0]
    for i, (draw, sdf_index, mn, mx) in enumerate(table):
        if draw >= models.shape[0]:
            continue
        model = models[draw]
        pmn, pmx = padded_box(mn, mx)
        wmn, wmx = world_box(model, mn, mx)
        inv = inverse(local_to_world(model, pmn, pmx))
        o = np.asarray(case["overrides"], F32).reshape(-1, 3)[draw]
        texture = int(np.asarray(case["materials"], U32).reshape(-1, 2)[draw][0]) if textures else NONE
        if not np.isnan(o[0]):
            albedo = o
        elif texture < textures:
            albedo = np.asarray(case["means"], F32).reshape(-1, 4)[texture][:3]
        else:
            albedo = mean_albedo([case["albedo_words"][draw]])[:3]
        record = (pmx - pmn).astype(F32).tobytes() + struct.pack("<I", int(sdf_index)) + np.asarray(albedo, F32).tobytes() + struct.pack("<f", 0.0) + inv.tobytes()
        assert len(record) == INSTANCE_BYTES
        inst[HEADER_BYTES + INSTANCE_BYTES * i:HEADER_BYTES + INSTANCE_BYTES * (i + 1)] = record
        bbs[BB_BYTES * i:BB_BYTES * (i + 1)] = wmn.tobytes() + struct.pack("<f", 0.0) + wmx.tobytes() + struct.pack("<f", 0.0)
    return bytes(inst), bytes(bbs)


def pack_scene(models, draw_meshes, mesh_boxes, mesh_textures, albedos, max_instances=None):
    """what a caller of plrf_set_sdf_scene uploads for a scene: the instance buffer and the world boxes of the draws whose mesh has a texture index, in draw order.
    mesh_boxes[m] = (min, max) or None; albedos[d] = the mean albedo (3 floats) of draw d"""
    table = [(d, mesh_textures[m], *mesh_boxes[m]) for d, m in enumerate(draw_meshes) if mesh_textures[m] != NONE]
    n = len(table)
    case = dict(models=models, table=table, albedo_words=[0] * len(draw_meshes), overrides=np.asarray(albedos, F32).reshape(-1, 3), materials=None, means=None,
                instances_prefill=bytes(HEADER_BYTES + INSTANCE_BYTES * n), bbs_prefill=bytes(BB_BYTES * n))
    return instance_pass(case)
