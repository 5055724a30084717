"""Inputs of the material texture tests of "depthPrepassRaster.comp" (tests/test_prepass_texture.py, tests/test_prepass_texture_cpu.py): named cases at the
smallest shapes at which the sampling can still go wrong, each with a check, on the reference alone, that the case is what it is for.

A case is a pair (prepass case, texture inputs): the dict of tests/prepass_raster_cases.py and the dict tests/prepass_texture_reference.py describes. Hand-made
triangles are written in pixel coordinates (prepass_raster_cases.pixel_case, w = 1) and their UVs as a function of the vertex's pixel position.
  magnify_repeat  a 4 x 4 texture on a quad over a 16 x 16 image, UVs from -1 to 2: 0.75 texels per pixel (level 0 only), repeat on both axes, a negative Tu
  level_exact     a 64 x 64 texture whose 7 levels have distinct constant colours on 16 x 16 pixels: 4 texels per pixel, rho2 = 16, lod exactly 2
  level_between   the same at 3 texels per pixel: lod = log2(3), a level fraction that is neither 0 nor 128
  perspective     32 x 32: a floor quad from behind the camera (a vertex with w <= 0) to the distance; the level varies over the image
  unequal_axes    32 x 16, a 32 x 8 texture: a quad stretched along u (rx > ry) beside one stretched along v (ry > rx)
  odd_sizes       32 x 32: textures of 5 x 3, 1 x 1, 8 x 8 with mipCount 1, and 16 x 1
  bias_negative / bias_positive  g_mipBias -0.75 and +1.5 on a magnified and a minified quad: the lower clamp is reached in the first, the upper in the second
  ragged          70 x 66, one triangle over every pixel: P_x and P_y leave the tile (x = 63, y = 63) and the image (x = 69, y = 65)
  degenerate      16 x 16: a triangle whose three clip vertices are exactly collinear in fp64 (s == 0: b = (1, 0, 0)) and whose snapped vertices are not
  material_mix    48 x 16, three draws: albedo only, none, specular only
  hazard_*        raw-record hazards: a texture index >= textureCount; an unusable table entry (width 0, mipCount 16); a texelOffset past texels and one that
                  leaves it half way; a NaN UV; uvs shorter than the positions
"""
import numpy as np

import prepass_raster_cases as pc
import prepass_texture_reference as tref
from shadow_raster_cases import quad

F32 = np.float32
NONE = tref.NONE


def pattern(width, height, salt):
    """distinct RGBA8 texels, every channel varying along both axes"""
    y, x = np.mgrid[0:height, 0:width].astype(np.uint32)
    r, g = (x * 53 + y * 19 + salt * 7) & 255, (x * 11 + y * 97 + salt * 31) & 255
    b, a = (x * 151 + y * 3 + salt) & 255, (x * 29 + y * 61 + salt * 13) & 255
    return (r | (g << 8) | (b << 16) | (a << 24)).astype(np.uint32).reshape(-1)


def chain(level0, width, height, mips=None):
    """the texels of `mips` levels (default: the full chain) built from level 0 by the host's rule"""
    full = tref.build_chain(level0, width, height)
    return full if mips is None else full[:tref.chain_texels(width, height, mips)]


def texture_set(textures):
    """[(texels of all levels, width, height, mips)] -> table (T x 4 uint32), texels"""
    table, texels, offset = [], [], 0
    for t, width, height, mips in textures:
        t = np.asarray(t, np.uint32).reshape(-1)
        assert t.size == tref.chain_texels(width, height, mips)
        table.append((offset, width, height, mips))
        texels.append(t)
        offset += t.size
    return np.asarray(table, np.uint32).reshape(-1, 4), np.concatenate(texels) if texels else np.zeros(0, np.uint32)


def pixel_uvs(case, fn):
    """per vertex of a pixel_case: fn(x, y in pixels) -> (u, v), float32"""
    p = case["positions"].astype(np.float64)
    x, y = (p[:, 0] + 1.0) * 0.5 * case["width"], (p[:, 1] + 1.0) * 0.5 * case["height"]
    u, v = fn(x, y)
    return np.stack([np.broadcast_to(u, x.shape), np.broadcast_to(v, x.shape)], axis=1).astype(F32)


def textured(case, uvs, materials, textures, mip_bias=0.0, texture_count=None):
    table, texels = textures if isinstance(textures, tuple) else texture_set(textures)
    tex = dict(uvs=np.asarray(uvs, F32).reshape(-1, 2), materials=np.asarray(materials, np.uint32).reshape(-1, 2), textures=table, texels=texels,
               texture_count=table.shape[0] if texture_count is None else int(texture_count), mip_bias=float(F32(mip_bias)))
    return case, tex


def _full(width, height, salt):
    return chain(pattern(width, height, salt), width, height), width, height, tref.full_mip_count(width, height)


def _magnify_repeat():
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16)
    uvs = pixel_uvs(case, lambda x, y: (-1.0 + 3.0 * x / 16.0, -1.0 + 3.0 * y / 16.0))
    return [textured(case, uvs, [(0, 1)], [_full(4, 4, 1), _full(4, 4, 2)])]


LEVEL_COLOURS = [0xFF000000 | (40 * l + 10) | ((250 - 30 * l) << 8) | ((17 * l + 3) << 16) for l in range(7)]


def _level_texture():
    return np.concatenate([np.full(tref.level_size(64, 64, l)[0] ** 2, LEVEL_COLOURS[l], np.uint32) for l in range(7)]), 64, 64, 7


def _level(scale):
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16)
    uvs = pixel_uvs(case, lambda x, y: (scale * x / 16.0, scale * y / 16.0))
    return [textured(case, uvs, [(0, 1)], [_level_texture(), _full(64, 64, 5)])]


FLOOR = np.array([[-40.0, 1.5, -5.0], [40.0, 1.5, -5.0], [40.0, 1.5, 200.0], [-40.0, 1.5, 200.0]], F32)


def _perspective():
    cam = pc.camera(aspect=1.0, near=0.1, far=300.0)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    import prepass_raster_reference as ref
    case = pc.make_case(32, 32, ref.main_pass_matrices(vp, vp, [pc.IDENTITY]), FLOOR, [0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3], [[0, 12, 0, 0]])  # both windings: one faces the camera
    uvs = np.stack([FLOOR[:, 0] / F32(4.0), FLOOR[:, 2] / F32(4.0)], axis=1)
    return [textured(case, uvs, [(0, 1)], [_full(64, 64, 3), _full(32, 64, 4)])]


def quad_uvs(case, fns):
    """a pixel_case of quads (six vertices each, in order): quad k's UVs by fns[k](x, y in pixels)"""
    p = case["positions"].astype(np.float64)
    x, y = (p[:, 0] + 1.0) * 0.5 * case["width"], (p[:, 1] + 1.0) * 0.5 * case["height"]
    assert p.shape[0] == 6 * len(fns)
    return np.concatenate([np.stack(fn(x[6 * k:6 * k + 6], y[6 * k:6 * k + 6]), axis=1) for k, fn in enumerate(fns)]).astype(F32)


def _unequal_axes():
    """left: 4 texels per pixel along u, 1 / 8 along v; right: 1 / 2 along u, 2 along v"""
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5) + quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5)], 32, 16)
    uvs = quad_uvs(case, [lambda x, y: (2.0 * x / 16.0, 0.25 * y / 16.0), lambda x, y: (0.25 * (x - 16.0) / 16.0, 4.0 * y / 16.0)])
    return [textured(case, uvs, [(0, 0)], [_full(32, 8, 6)])]


def _odd_sizes():
    quads = [quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5), quad(0.0, 16.0, 16.0, 32.0, 0.5, 0.5), quad(16.0, 16.0, 32.0, 32.0, 0.5, 0.5)]
    case = pc.pixel_case(quads, 32, 32)
    uvs = pixel_uvs(case, lambda x, y: (2.5 * x / 16.0, 2.5 * y / 16.0))
    textures = [_full(5, 3, 7), _full(1, 1, 8), (pattern(8, 8, 9), 8, 8, 1), _full(16, 1, 10)]
    return [textured(case, uvs, [(k, (k + 1) % 4) for k in range(4)], textures)]


def _bias(mip_bias):
    """an 8 x 8 texture with 4 levels: draw 0 at 1 / 2 texel per pixel (lod -1 before the bias), draw 1 at 4 texels per pixel (lod 2)"""
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5)], 32, 16)
    uvs = quad_uvs(case, [lambda x, y: (x / 16.0, y / 16.0), lambda x, y: (8.0 * (x - 16.0) / 16.0, 8.0 * y / 16.0)])
    return [textured(case, uvs, [(0, 0), (0, 0)], [_full(8, 8, 11)], mip_bias=mip_bias)]


def _ragged():
    case = pc.pixel_case([[[(-1.0, -1.0, 0.1), (150.0, -1.0, 0.9), (-1.0, 150.0, 0.5)]]], 70, 66)
    uvs = pixel_uvs(case, lambda x, y: (3.0 * x / 70.0, 3.0 * y / 66.0))
    return [textured(case, uvs, [(0, 1)], [_full(16, 16, 12), _full(8, 16, 13)])]


def _degenerate():
    """the three vertices lie on y = -x - 0.125 exactly (fp32 values, so exactly in fp64 too): s == 0 at every pixel. Vertex 2's x term of the viewport transform,
    x * 0.5 + 0.5, lies in [0.25, 0.5) and is exact, its y term in [0.5, 1) rounds by half a unit in the last place: X snaps to 1101 and Y by one sub-pixel unit
    off the line, and the sliver covers the pixel centres on the line"""
    a = ((1100 + 0.5 + 2.0 ** -13) - 2048.0) / 2048.0
    v = np.array([(-0.5, 0.375, 0.5), (a, -a - 0.125, 0.5), (0.25, -0.375, 0.5)], np.float64)
    assert np.array_equal(v.astype(F32).astype(np.float64), v)
    case = pc.make_case(16, 16, pc.identity_matrices(1), v.astype(F32), [0, 1, 2], [[0, 3, 0, 0]])
    return [textured(case, [(0.1, 0.2), (0.7, 0.3), (0.4, 0.9)], [(0, 0)], [_full(4, 4, 14)])]


def _material_mix():
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5), quad(32.0, 0.0, 48.0, 16.0, 0.5, 0.5)], 48, 16)
    uvs = pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    return [textured(case, uvs, [(0, NONE), (NONE, NONE), (NONE, 1)], [_full(8, 8, 15), _full(8, 4, 16)])]


def _hazard_quads(materials, textures, uvs_fn=None, texture_count=None):
    case = pc.pixel_case([quad(0.0, 0.0, 8.0, 16.0, 0.5, 0.5), quad(8.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16)
    uvs = pixel_uvs(case, lambda x, y: (x / 8.0, y / 8.0))
    if uvs_fn is not None:
        uvs = uvs_fn(uvs)
    return textured(case, uvs, materials, textures, texture_count=texture_count)


def _hazard_index():
    """two table rows, textureCount 1: row 1 does not exist for the pass, and 5 never did; draw 1 samples row 0"""
    return [_hazard_quads([(1, 5), (0, 0)], [_full(4, 4, 17), _full(4, 4, 18)], texture_count=1)]


def _hazard_entry():
    table, texels = texture_set([_full(4, 4, 19), _full(4, 4, 20), _full(4, 4, 21)])
    table[0, 1] = 0    # width 0
    table[1, 3] = 16   # more levels than the size has
    return [_hazard_quads([(0, 1), (2, 1)], (table, texels))]


def _hazard_offset():
    table, texels = texture_set([_full(4, 4, 22), _full(4, 4, 23)])
    table[0, 0] = texels.size + 10  # wholly past the end: every tap reads 0
    table[1, 0] = texels.size - 8   # level 0's second half and the levels above lie past the end
    return [_hazard_quads([(0, 0), (1, 1)], (table, texels))]


def _hazard_nan_uv():
    def nan_one(uvs):
        uvs = uvs.copy()
        uvs[1, 0] = np.nan  # a vertex of draw 0's first triangle
        uvs[4, 1] = np.inf  # and of its second
        return uvs
    return [_hazard_quads([(0, 0), (0, 0)], [_full(4, 4, 24)], uvs_fn=nan_one)]


def _hazard_short_uvs():
    return [_hazard_quads([(0, 0), (0, 0)], [_full(4, 4, 25)], uvs_fn=lambda uvs: uvs[:6].copy())]  # draw 1's vertices 6 .. 11 have none: (0, 0)


CASES = dict(magnify_repeat=_magnify_repeat, level_exact=lambda: _level(1.0), level_between=lambda: _level(0.75), perspective=_perspective, unequal_axes=_unequal_axes,
             odd_sizes=_odd_sizes, bias_negative=lambda: _bias(-0.75), bias_positive=lambda: _bias(1.5), ragged=_ragged, degenerate=_degenerate,
             material_mix=_material_mix, hazard_index=_hazard_index, hazard_entry=_hazard_entry, hazard_offset=_hazard_offset, hazard_nan_uv=_hazard_nan_uv,
             hazard_short_uvs=_hazard_short_uvs)

_reference_cache = {}


def reference(name):
    """[(case, texture inputs, rasterise result, sample result with diagnostics)], computed once; callers must not modify it"""
    if name not in _reference_cache:
        out = []
        for case, tex in CASES[name]():
            r = pc.rasterise(case)
            out.append((case, tex, r, tref.sample(case, tex, r["keys"], diagnostics=True)))
        _reference_cache[name] = out
    return _reference_cache[name]


def _channel(words, k):
    return (np.asarray(words, np.uint32) >> np.uint32(8 * k)) & np.uint32(255)


def _constants(case, draw):
    return int(case["draws"][draw, 4]), int(case["draws"][draw, 5])


def _check_magnify_repeat(runs):
    (case, tex, r, s), = runs
    d = s["diagnostics"]["albedo"]
    assert (r["keys"] != 0).all() and (d["L0"] == 0).all() and (d["fw"] == 0).all(), "0.75 texels per pixel: level 0 alone"
    assert d["tu_min"] < 0, "the left columns have a negative Tu"
    # pixel (5, 5) by hand: u = -1 + 3 * 5.5 / 16 = 0.03125, u * 4 - 0.5 = -0.375, Tu = floor(-96 + 0.5) = -96: x0 = -1 -> 3, fx = 160, x1 = 0; v likewise
    t = tex["texels"][:16].reshape(4, 4)
    for k in range(4):
        c = lambda x, y: int(_channel(t[y, x], k))
        S = 96 * 96 * c(3, 3) + 160 * 96 * c(0, 3) + 96 * 160 * c(3, 0) + 160 * 160 * c(0, 0)
        S *= 256
        assert int(_channel(s["albedo"][5, 5], k)) == (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24
    assert not np.array_equal(s["albedo"], np.full_like(s["albedo"], s["albedo"][0, 0]))


def _check_level_exact(runs):
    (case, tex, r, s), = runs
    d = s["diagnostics"]["albedo"]
    assert (r["keys"] != 0).all() and (d["lod"] == F32(2.0)).all() and (d["L0"] == 2).all() and (d["fw"] == 0).all()
    assert (s["albedo"] == LEVEL_COLOURS[2]).all()
    assert (s["diagnostics"]["specular"]["L0"] == 2).all() and np.unique(s["specular"]).size > 8


def _check_level_between(runs):
    (case, tex, r, s), = runs
    d = s["diagnostics"]["albedo"]
    assert (d["L0"] == 1).all() and np.unique(d["fw"]).tolist() == [150], "lod = log2(3) = 1.585: fw = rint(0.585 * 256) = 150"
    S = [(256 - 150) * 65536 * int(_channel(LEVEL_COLOURS[1], k)) + 150 * 65536 * int(_channel(LEVEL_COLOURS[2], k)) for k in range(4)]
    want = sum(((v + (1 << 23) - 1 + ((v >> 24) & 1)) >> 24) << (8 * k) for k, v in enumerate(S))
    assert (s["albedo"] == want).all()


def _check_perspective(runs):
    (case, tex, r, s), = runs
    import prepass_raster_reference as ref
    clip = ref.transform4(case["transforms"][0, 16:32], case["positions"])
    assert (clip[:, 3] <= 0).any() and (clip[:, 3] > 0).any(), "the floor reaches behind the camera"
    covered = r["keys"] != 0
    assert r["clipped"] >= 1 and covered.sum() > 200
    levels = np.unique(s["diagnostics"]["albedo"]["L0"][covered])
    assert levels.size >= 4, "the level varies over the image: %r" % (levels,)
    fw = np.unique(s["diagnostics"]["albedo"]["fw"][covered])
    assert fw.size > 20


def _check_unequal_axes(runs):
    (case, tex, r, s), = runs
    g = s["diagnostics"]["albedo"]["rx_gt_ry"]
    assert (g[:, :16] == 1).all() and (g[:, 16:] == 0).all()
    assert (s["diagnostics"]["albedo"]["L0"][:, :16] == 2).all() and (s["diagnostics"]["albedo"]["L0"][:, 16:] == 1).all(), "4 and 2 texels per pixel"


def _check_odd_sizes(runs):
    (case, tex, r, s), = runs
    assert (r["keys"] != 0).all()
    assert tex["textures"][:, 1:].tolist() == [[5, 3, 3], [1, 1, 1], [8, 8, 1], [16, 1, 5]]
    assert np.unique(s["albedo"][:16, 16:]).tolist() == [int(tex["texels"][tex["textures"][1, 0]])], "a 1 x 1 texture is its texel"
    assert (s["diagnostics"]["albedo"]["L0"][16:, :16] == 0).all() and np.unique(s["albedo"][16:, :16]).size > 8, "mipCount 1: level 0 whatever the footprint"
    assert s["diagnostics"]["albedo"]["L0"][:16, :16].max() >= 0 and s["diagnostics"]["albedo"]["L0"][16:, 16:].max() >= 1


def _check_bias_negative(runs):
    (case, tex, r, s), = runs
    d = s["diagnostics"]["albedo"]
    assert (d["lod"][:, :16] == 0).all(), "-1 - 0.75 is clamped to 0"
    assert (d["L0"][:, 16:] == 1).all() and (d["fw"][:, 16:] == 64).all(), "2 - 0.75"


def _check_bias_positive(runs):
    (case, tex, r, s), = runs
    d = s["diagnostics"]["albedo"]
    assert (d["L0"][:, :16] == 0).all() and (d["fw"][:, :16] == 128).all(), "-1 + 1.5"
    assert (d["lod"][:, 16:] == 3).all() and (d["L0"][:, 16:] == 3).all() and (d["fw"][:, 16:] == 0).all(), "2 + 1.5 is clamped to mipCount - 1 = 3"


def _check_ragged(runs):
    (case, tex, r, s), = runs
    assert (case["width"], case["height"]) == (70, 66) and (r["keys"] != 0).all(), "winners in column 63, column 69, row 63 and row 65"
    assert np.unique(s["albedo"]).size > 100


def _check_degenerate(runs):
    (case, tex, r, s), = runs
    covered = r["keys"] != 0
    assert covered.sum() >= 1 and np.array_equal(r["weights"], np.tile([1.0, 0.0, 0.0], (int(covered.sum()), 1))), "s == 0: b = (1, 0, 0)"
    assert (s["diagnostics"]["albedo"]["lod"][covered] == 0).all() and np.unique(s["albedo"][covered]).size == 1, "no derivative: level 0, one UV"
    assert int(np.unique(s["albedo"][covered])[0]) != _constants(case, 0)[0]


def _check_material_mix(runs):
    (case, tex, r, s), = runs
    a, sp = s["albedo"], s["specular"]
    assert np.unique(a[:, :16]).size > 8 and (sp[:, :16] == _constants(case, 0)[1]).all()
    assert (a[:, 16:32] == _constants(case, 1)[0]).all() and (sp[:, 16:32] == _constants(case, 1)[1]).all()
    assert (a[:, 32:] == _constants(case, 2)[0]).all() and np.unique(sp[:, 32:]).size > 8


def _check_hazard_index(runs):
    (case, tex, r, s), = runs
    assert tex["texture_count"] == 1 and tex["textures"].shape[0] == 2
    assert (s["albedo"][:, :8] == _constants(case, 0)[0]).all() and (s["specular"][:, :8] == _constants(case, 0)[1]).all()
    assert np.unique(s["albedo"][:, 8:]).size > 8


def _check_hazard_entry(runs):
    (case, tex, r, s), = runs
    assert (s["albedo"][:, :8] == _constants(case, 0)[0]).all() and (s["specular"][:, :8] == _constants(case, 0)[1]).all()
    assert np.unique(s["albedo"][:, 8:]).size > 8 and (s["specular"][:, 8:] == _constants(case, 1)[1]).all()


def _check_hazard_offset(runs):
    (case, tex, r, s), = runs
    assert not s["albedo"][:, :8].any() and not s["specular"][:, :8].any(), "every tap reads 0"
    right = s["albedo"][:, 8:]
    assert (right == 0).any() and (right != 0).any(), "half of level 0 lies inside"


def _check_hazard_nan_uv(runs):
    (case, tex, r, s), = runs
    left = s["albedo"][:, :8]
    assert np.unique(left).size == 1 and (s["diagnostics"]["albedo"]["lod"][:, :8] == 0).all(), "u = v = 0 and level 0 for every pixel of the draw with a NaN or inf UV"
    t = tex["texels"][:16].reshape(4, 4)  # (0, 0): Tu = -128: x0 = -1 -> 3, fx = 128: the mean of the four corner texels
    for k in range(4):
        S = 128 * 128 * 256 * sum(int(_channel(t[y, x], k)) for x in (0, 3) for y in (0, 3))
        assert int(_channel(left[0, 0], k)) == (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24
    assert np.unique(s["albedo"][:, 8:]).size > 8


def _check_hazard_short_uvs(runs):
    (case, tex, r, s), = runs
    assert tex["uvs"].shape[0] == 6 < case["positions"].shape[0]
    assert np.unique(s["albedo"][:, :8]).size > 8
    right = np.unique(s["albedo"][:, 8:])
    assert right.size == 1 and int(right[0]) != _constants(case, 1)[0], "every vertex of draw 1 has (0, 0): one sample, and it is a sample"


CASE_CHECKS = {name: globals()["_check_" + name] for name in CASES}


def check_case_is_what_it_is_for(name):
    CASE_CHECKS[name](reference(name))
