"""Inputs of the cutout tests of "sunShadowRaster.comp" (tests/test_shadow_alpha.py, tests/test_shadow_alpha_cpu.py): named cases at most 160 x 160 texels
large, each with a check, on the reference alone (tests/shadow_alpha_reference.py), that the case exercises what it is named for.

A case is a list of runs (shadow case, texture inputs, cascade index): the dicts of tests/shadow_raster_cases.py and tests/shadow_alpha_reference.py. Hand-made
parts are quads and triangles in pixels of the map (tests/shadow_raster_cases.py), one draw per part, with a UV per vertex given as a function of the vertex's
pixel position. The map keeps the MAXIMUM code: the larger z wins.
  cutout_over_opaque  96: a checker-alpha card with the greater depth code over an opaque quad and partly over nothing
  stacked             96: two tested cards with different textures and cutoffs over an opaque quad
  paths               160 (tiles of 64 + 64 + 32) and 157 (rows stored texel by texel): tested triangles through the lane path (a 4 x 4 box), the wave path (a
                      40 x 40 quad), the int64 path (175 pixels wide) and across a tile corner
  mip_threshold       96: a texture whose levels have the alphas 255, 0, 255, .. minified by ratios on both sides of the half-level points (where fw crosses 128 and
                      the blended alpha crosses the cutoff) and of the level boundaries; two anisotropic quads, one with rx > ry and one with ry > rx, whose smaller
                      axis alone would give the other answer
  cutoff_values       96: cutoff words 0, 1, 128, 255 and 300 on a ramp texture with alpha rows 0 / 127 / 128 / 255 / 1; a draw without a texture, one with an
                      index at or past textureCount and one naming an entry of width 0, each at 128 and 300
  uv_edges            96: UVs that wrap (negative, and above 1), a u that passes 2^20 inside a quad (the validity rule), a non-power-of-two texture, a 1 x 1
                      texture, a chain of one level under minification, and two vertices outside `uvs`
  transformed         160: box, sphere and torus of tests/shadow_raster_cases.py's mesh scene with their UVs and two two-sided cards under the scene's first
                      light matrix: the affine transform and the front-face cull take part
"""
import numpy as np

import prepass_texture_reference as tref
import shadow_alpha_reference as aref
import shadow_raster_cases as sc
import shadow_raster_reference as ref
from shadow_raster_cases import quad

F32 = np.float32
NONE = aref.NONE
REFERENCE_CUTOFF = 128


def code_of(z):
    return int(np.rint(ref.clamp01(F32(z)) * F32(65535.0)))


def checker(width, height, cell, salt, phase=0):
    """RGBA8 texels: alpha 0 / 255 in cells of `cell` texels, colours that are no use to anyone"""
    y, x = np.mgrid[0:height, 0:width]
    alpha = np.where(((x // cell) + (y // cell) + phase) % 2 == 0, 255, 0).astype(np.uint32)
    rgb = ((x * 7 + y * 13 + salt) * 2654435761 & 0x00FFFFFF).astype(np.uint32)
    return (rgb | (alpha << np.uint32(24))).reshape(-1)


def full_chain(level0, width, height):
    return tref.build_chain(level0, width, height), width, height, tref.full_mip_count(width, height)


def store(textures, extra_entries=()):
    """[(texels of all levels, width, height, mipCount)] -> (table T x 4, texels); extra_entries: raw table rows appended behind"""
    table, texels, at = [], [], 0
    for t, w, h, mips in textures:
        t = np.asarray(t, np.uint32).reshape(-1)
        assert t.size == tref.chain_texels(w, h, mips)
        table.append((at, w, h, mips))
        texels.append(t)
        at += t.size
    table += list(extra_entries)
    return np.array(table, np.uint32).reshape(-1, 4), np.concatenate(texels) if texels else np.zeros(0, np.uint32)


def build(res, parts, textures, texture_count=None, extra_entries=(), uv_vertices=None):
    """parts: [(triangles, uv(x, y) -> (u, v), albedoTexture, cutoff word)], one draw each -> (case, tex)"""
    tris = [t for p in parts for t in p[0]]
    case = sc.pixel_case(tris, res)
    xy = np.asarray(tris, np.float64).reshape(-1, 3)[:, :2]
    draws, uvs, first = [], [], 0
    for triangles, uv, texture, cutoff in parts:
        n = 3 * len(triangles)
        draws.append((first, n, 0, 0))
        uvs += [uv(x, y) for x, y in xy[first:first + n]]
        first += n
    case = dict(case, draws=np.array(draws, np.uint32).reshape(-1, 4))
    table, texels = store(textures, extra_entries)
    uvs = np.asarray(uvs, np.float64).astype(F32).reshape(-1, 2)
    if uv_vertices is not None:
        uvs = uvs[:uv_vertices].copy()
    tex = dict(uvs=uvs, materials=np.array([(p[2], p[3]) for p in parts], np.uint32).reshape(-1, 2), textures=table, texels=texels,
               texture_count=table.shape[0] if texture_count is None else texture_count)
    return case, tex


def only(case, tex, d):
    """the run with draw d alone"""
    return dict(case, draws=case["draws"][d:d + 1]), dict(tex, materials=tex["materials"][d:d + 1])


def texel_ratio(x0, y0, ru, rv, width, height):
    """UVs that advance ru texels of a width x height texture per pixel in x and rv per pixel in y"""
    return lambda x, y: ((x - x0) * ru / width, (y - y0) * rv / height)


NO_UV = lambda x, y: (0.0, 0.0)
CHECKER16 = full_chain(checker(16, 16, 2, 11), 16, 16)


def _cutout_over_opaque():
    parts = [(quad(10.0, 10.0, 50.0, 50.0, 0.3, 0.3), NO_UV, NONE, 0),
             (quad(30.0, 20.0, 80.0, 70.0, 0.7, 0.7), texel_ratio(30.0, 20.0, 0.5, 0.5, 16, 16), 0, REFERENCE_CUTOFF)]  # cells of 4 pixels
    return [build(96, parts, [CHECKER16]) + (1,)]


def _stacked():
    parts = [(quad(6.0, 6.0, 90.0, 90.0, 0.3, 0.35), NO_UV, NONE, 0),
             (quad(10.0, 4.0, 70.0, 80.0, 0.5, 0.5), texel_ratio(0.0, 0.0, 0.4, 0.4, 8, 8), 1, 100),
             (quad(20.0, 12.0, 92.0, 60.0, 0.7, 0.65), texel_ratio(3.0, 1.0, 0.25, 0.5, 16, 16), 0, 200)]
    return [build(96, parts, [CHECKER16, full_chain(checker(8, 8, 1, 12, phase=1), 8, 8)]) + (0,)]


# (name, triangles): where each tested part of `paths` is meant to go
PATH_PARTS = [("lane", [[(10.25, 5.5, 0.6), (13.75, 5.5, 0.6), (13.75, 9.0, 0.6)]]),            # a 4 x 4 box
              ("wave", quad(20.0, 20.0, 60.0, 60.0, 0.5, 0.55)),                                  # 8 x 8 stamps inside tile (0, 0)
              ("corner", [[(40.0, 50.0, 0.7), (100.0, 52.0, 0.8), (90.0, 120.0, 0.75)]]),         # across x = 64 and y = 64
              ("int64", [[(-20.0, 130.0, 0.6), (155.0, 132.0, 0.65), (-20.0, 150.0, 0.7)]]),      # 175 pixels wide: a span of 44800 >= 2^15, into the ragged tile column
              ("lane_ragged", [[(140.5, 140.5, 0.9), (144.0, 140.5, 0.9), (144.0, 144.0, 0.9)]])]  # the lane path in the 32-pixel tile column and row


def _paths():
    parts = [(tris, texel_ratio(0.0, 0.0, 1.0, 1.0, 16, 16), 0, REFERENCE_CUTOFF) for _, tris in PATH_PARTS]  # a texel per pixel, cells of 2 pixels
    return [build(160, parts, [CHECKER16]) + (2,), build(157, parts, [CHECKER16]) + (3,)]


MIP_LEVEL_ALPHAS = (255, 0, 255, 0, 255, 0, 255)
# texels per pixel (u, v), and whether the quad passes the cutoff 128: lod = log2(max), fw = rint(256 frac(lod)), alpha = ((256 - fw) a_L0 + fw a_L1) / 256
MIP_QUADS = [((0.9, 0.9), True),     # lod < 0 -> 0: level 0
             ((1.38, 1.38), True),   # lod 0.465, fw 119: 136.5
             ((1.45, 1.45), False),  # lod 0.536, fw 137: 118.5
             ((1.9, 1.9), False),    # lod 0.926, fw 237: 18.9
             ((2.1, 2.1), False),    # lod 1.070, L0 = 1, fw 18: 17.9 (with L0 = 0 it would pass)
             ((2.75, 2.75), False),  # lod 1.459, fw 118: 117.5
             ((2.9, 2.9), True),     # lod 1.536, fw 137: 136.5
             ((4.2, 4.2), True),     # lod 2.070, L0 = 2
             ((2.9, 1.45), True),    # rx > ry: 2.9 decides; 1.45 alone would fail
             ((1.0, 2.75), False)]   # ry > rx: 2.75 decides; 1.0 alone would pass


def _mip_texture():
    levels = []
    for l, a in enumerate(MIP_LEVEL_ALPHAS):
        w, h = tref.level_size(64, 64, l)
        levels.append((checker(w, h, 1, 20 + l) & np.uint32(0x00FFFFFF)) | np.uint32(a << 24))
    return np.concatenate(levels), 64, 64, len(MIP_LEVEL_ALPHAS)


def _mip_quad_box(k):
    x0, y0 = 4.0 + 18.0 * (k % 5), 4.0 + 26.0 * (k // 5)
    return x0, y0, x0 + 16.0, y0 + 16.0


def _mip_threshold():
    parts = []
    for k, ((ru, rv), _) in enumerate(MIP_QUADS):
        x0, y0, x1, y1 = _mip_quad_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.2 + 0.05 * k, 0.2 + 0.05 * k), texel_ratio(x0, y0, ru, rv, 64, 64), 0, REFERENCE_CUTOFF))
    return [build(96, parts, [_mip_texture()]) + (1,)]


RAMP_ROWS = (0, 127, 128, 255, 1)
CUTOFF_DRAWS = [(0, 0), (0, 1), (0, 128), (0, 255), (0, 300),  # (albedoTexture, cutoff word)
                (NONE, 128), (NONE, 300), (7, 128), (7, 300), (1, 128), (1, 300)]  # no texture; at or past textureCount = 2; entry 1 has width 0


def _cutoff_quad_box(k):
    return 2.0 + 8.0 * k, 5.0, 10.0 + 8.0 * k, 30.0


def _cutoff_values():
    ramp = np.repeat(np.array(RAMP_ROWS, np.uint32) << np.uint32(24), 4) | np.uint32(0x00A0B0C0)  # 4 x 5 texels, one level
    parts = []
    for k, (texture, word) in enumerate(CUTOFF_DRAWS):
        x0, y0, x1, y1 = _cutoff_quad_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.2 + 0.05 * k, 0.2 + 0.05 * k), lambda x, y, y0=y0: (x / 8.0, (y - y0) / 25.0), texture, word))  # 5 pixels per texel row
    return [build(96, parts, [(ramp, 4, 5, 1)], extra_entries=[(0, 0, 4, 1)]) + (0,)]


UV_EDGE_PARTS = ["negative", "above_one", "past_2_20", "non_power_of_two", "one_by_one_kept", "one_by_one_dropped", "one_level", "outside_uvs"]


def _uv_edges():
    textures = [CHECKER16, full_chain(checker(5, 3, 1, 31), 5, 3), (np.array([200 << 24 | 0x112233], np.uint32), 1, 1, 1), (checker(16, 16, 2, 32), 16, 16, 1)]
    parts = [(quad(4.0, 4.0, 28.0, 28.0, 0.3, 0.3), lambda x, y: ((x - 50.0) / 16.0, (y - 70.0) / 16.0), 0, REFERENCE_CUTOFF),
             (quad(34.0, 4.0, 58.0, 28.0, 0.35, 0.35), lambda x, y: (x / 16.0 + 1.5, y / 16.0 + 5.25), 0, REFERENCE_CUTOFF),
             # u runs from 0 to 2^21 over 24 pixels: the right half is not valid and samples (0, 0), a blend of the four corner texels that reaches 100
             (quad(64.0, 4.0, 88.0, 28.0, 0.4, 0.4), lambda x, y: ((x - 64.0) / 24.0 * 2097152.0, y / 16.0), 3, 100),
             (quad(4.0, 34.0, 28.0, 58.0, 0.45, 0.45), texel_ratio(4.0, 34.0, 0.5, 0.25, 5, 3), 1, REFERENCE_CUTOFF),
             (quad(34.0, 34.0, 46.0, 58.0, 0.5, 0.5), texel_ratio(0.0, 0.0, 0.3, 0.3, 1, 1), 2, 200),
             (quad(48.0, 34.0, 58.0, 58.0, 0.55, 0.55), texel_ratio(0.0, 0.0, 0.3, 0.3, 1, 1), 2, 201),
             (quad(64.0, 34.0, 88.0, 58.0, 0.6, 0.6), texel_ratio(64.0, 34.0, 3.0, 3.0, 16, 16), 3, REFERENCE_CUTOFF),  # 3 texels per pixel, a chain of one level
             (quad(4.0, 64.0, 28.0, 88.0, 0.65, 0.65), texel_ratio(0.0, 0.0, 0.5, 0.5, 16, 16), 0, REFERENCE_CUTOFF)]
    assert len(parts) == len(UV_EDGE_PARTS)
    return [build(96, parts, textures, uv_vertices=6 * len(parts) - 2) + (3,)]  # the last two vertices have no UV: (0, 0)


CARD = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F32), np.array([0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2], np.uint32),
        np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F32))  # two-sided: each triangle in both windings
TRANSFORMED_MATERIALS = [(0, REFERENCE_CUTOFF), (0, REFERENCE_CUTOFF), (NONE, REFERENCE_CUTOFF), (0, REFERENCE_CUTOFF), (1, 60)]  # box, sphere, torus, two cards


def caster_scene():
    """the casters of `transformed` and of tests/test_shadow_alpha_frame.py: meshes [(positions, indices, uvs)], draws [(mesh, 16 floats)], textures [(texels of
    all levels, width, height, mipCount)] and one (albedoTexture, cutoff) per draw. Built once; callers must not modify it."""
    if "casters" not in _cache:
        from plainrenderer_amd import meshes
        s = sc.mesh_scene()
        with_uvs = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_uvs=True), meshes.uv_sphere(1.25, segments=28, rings=14, with_uvs=True),
                    meshes.torus(1.5, 0.5, segments=24, sides=12, with_uvs=True), CARD]
        with_uvs = [(np.asarray(p, F32), np.asarray(i, np.uint32).reshape(-1), np.asarray(u, F32).reshape(-1, 2)) for p, i, u in with_uvs]
        for (p, i, _), (sp, si) in zip(with_uvs[:3], s["meshes"]):
            assert np.array_equal(p, sp) and np.array_equal(i, si), "the mesh scene's meshes"
        cam = s["cam"]
        fwd, pos = np.asarray(cam.forward, np.float64), np.asarray(cam.position, np.float64)
        right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)
        draws = list(s["draws"]) + [(3, sc.affine((2.0, 2.0, 1.0), 0.3, 1.2, pos + 7.0 * fwd + 0.5 * right + 1.0 * up)),
                                    (3, sc.affine((1.5, 2.5, 1.0), -0.8, -1.0, pos + 10.0 * fwd - 1.0 * right))]
        textures = [full_chain(checker(64, 64, 8, 41), 64, 64), full_chain(checker(32, 16, 4, 42, phase=1), 32, 16)]
        _cache["casters"] = dict(meshes=with_uvs, draws=draws, textures=textures, cutouts=list(TRANSFORMED_MATERIALS))
    return _cache["casters"]


# the frame test's casters: the caster scene and five large two-sided cards that face the sun, along the view direction at distances and sizes that put one near
# the middle of every cascade the frame pipeline fits (the cascades reach hundreds of units; the mesh scene alone covers a handful of texels of the far ones)
FRAME_CARDS = [(30.0, 6.0, 0, REFERENCE_CUTOFF), (60.0, 10.0, 1, 60), (110.0, 16.0, 0, REFERENCE_CUTOFF), (160.0, 24.0, 1, 60), (250.0, 40.0, 0, REFERENCE_CUTOFF)]  # (distance, half size, texture, cutoff)


def frame_scene():
    """caster_scene() with FRAME_CARDS appended; same keys. Built once; callers must not modify it."""
    if "frame" not in _cache:
        base = caster_scene()
        cam, sun = sc.mesh_scene()["cam"], sc.mesh_scene()["sun"]
        fwd, pos = np.asarray(cam.forward, np.float64), np.asarray(cam.position, np.float64)
        right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)
        yaw, pitch = float(np.arctan2(sun[0], sun[2])), float(np.arcsin(-sun[1]))  # rotateY(yaw) rotateX(pitch) turns the card's normal (0, 0, 1) into the sun direction
        draws = list(base["draws"]) + [(3, sc.affine((half, half, 1.0), yaw, pitch, pos + d * fwd + 0.04 * d * right + 0.075 * d * up)) for d, half, _, _ in FRAME_CARDS]
        _cache["frame"] = dict(base, draws=draws, cutouts=list(base["cutouts"]) + [(t, c) for _, _, t, c in FRAME_CARDS])
    return _cache["frame"]


def caster_case(light_matrix, res, draws=None, cutouts=None, scene=None):
    """the caster scene (or `scene`) under a light matrix -> (case, tex)"""
    s = caster_scene() if scene is None else scene
    positions, indices, dr, tr = ref.merge_meshes([(m[0], m[1]) for m in s["meshes"]], s["draws"] if draws is None else draws)
    case = dict(res=res, light=np.asarray(light_matrix, F32).reshape(16).copy(), transforms=tr, positions=positions, indices=indices, draws=dr)
    table, texels = store(s["textures"])
    tex = dict(uvs=np.concatenate([m[2] for m in s["meshes"]]), materials=np.array(s["cutouts"] if cutouts is None else cutouts, np.uint32).reshape(-1, 2),
               textures=table, texels=texels, texture_count=table.shape[0])
    return case, tex


def _transformed():
    return [caster_case(ref.light_matrices(sc.mesh_scene()["info"])[0], 160) + (0,)]


CASES = {"cutout_over_opaque": _cutout_over_opaque, "stacked": _stacked, "paths": _paths, "mip_threshold": _mip_threshold, "cutoff_values": _cutoff_values,
         "uv_edges": _uv_edges, "transformed": _transformed}
_cache = {}


def reference(name):
    """[(case, tex, cascade, tested result, opaque result, details)], computed once per case; callers must not modify it"""
    if name not in _cache:
        runs = []
        for case, tex, cascade in CASES[name]():
            details = []
            runs.append((case, tex, cascade, aref.rasterise(case, tex, details), sc.rasterise(case), details))
        _cache[name] = runs
    return _cache[name]


def _alone(case, tex, d):
    details = []
    c, t = only(case, tex, d)
    return aref.rasterise(c, t, details), sc.rasterise(c), details


def _box_of(triangles, res):
    case = sc.pixel_case(triangles, res)
    X, Y, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], res)
    return ((int(X.max()) - 128) >> 8) - ((int(X.min()) + 127) >> 8) + 1, ((int(Y.max()) - 128) >> 8) - ((int(Y.min()) + 127) >> 8) + 1, int(X.max() - X.min())


def _check_cutout_over_opaque(runs):
    case, tex, _, a, o, _ = runs[0]
    card, behind = code_of(0.7), code_of(0.3)
    both, card_only = (slice(20, 50), slice(30, 50)), (slice(50, 70), slice(30, 80))
    assert (o["map"][both] == card).all() and (o["map"][card_only] == card).all(), "opaque, the card hides the quad"
    assert set(np.unique(a["map"][both]).tolist()) == {behind, card}, "holes show the quad's code"
    assert set(np.unique(a["map"][card_only]).tolist()) == {0, card}, "holes over nothing show 0"
    assert (a["map"][both] == behind).sum() > 100 and (a["map"][card_only] == 0).sum() > 100


def _check_stacked(runs):
    case, tex, _, a, o, _ = runs[0]
    alone = [_alone(case, tex, d)[0]["coverage"] > 0 for d in range(3)]
    solid = [sc.rasterise(only(case, tex, d)[0])["coverage"] > 0 for d in range(3)]
    top_hole, middle_hole = solid[2] & ~alone[2], solid[1] & ~alone[1]
    assert (top_hole & alone[1]).sum() > 50 and (top_hole & middle_hole & alone[0]).sum() > 50 and (alone[2] & alone[1]).sum() > 50
    sel = top_hole & alone[1]
    assert (a["map"][sel] == code_of(0.5)).all(), "a hole of the top card shows the card below where that one passes"
    sel = top_hole & middle_hole & alone[0]
    assert (a["map"][sel] == sc.rasterise(only(case, tex, 0)[0])["map"][sel]).all(), "holes of both show the opaque quad"
    assert (a["map"][alone[2]] >= code_of(0.65)).all()


def _check_paths(runs):
    assert [r[0]["res"] for r in runs] == [160, 157] and 160 % 8 == 0 and 157 % 8 != 0
    boxes = {name: _box_of(tris, 160) for name, tris in PATH_PARTS}
    assert boxes["lane"][:2] == (4, 4) and boxes["lane_ragged"][0] <= 4 and boxes["lane_ragged"][1] <= 4
    assert boxes["wave"][0] == 40 and boxes["wave"][2] < 32768 and boxes["int64"][2] == 44800 >= 32768
    for case, tex, _, a, o, _ in runs:
        for d, (name, _) in enumerate(PATH_PARTS):
            r, _, _ = _alone(case, tex, d)
            assert 0 < r["passed"] < r["tested"], name
            if name == "corner":
                cov = r["coverage"]
                assert cov[:64, :64].any() and cov[:64, 64:128].any() and cov[64:128, 64:128].any(), "across a tile corner"
            if name in ("int64", "lane_ragged"):
                assert r["coverage"][128:, 128:].any(), "the ragged tile column and row"


def _check_mip_threshold(runs):
    case, tex, _, a, o, details = runs[0]
    for k, ((ru, rv), passes) in enumerate(MIP_QUADS):
        x0, y0, x1, y1 = (int(v) for v in _mip_quad_box(k))
        mine = [t for t in details if t["draw"] == k]
        assert len(mine) == 2 and all(t["passed"] == (t["fragments"] if passes else 0) for t in mine), (k, mine)
        assert (a["map"][y0:y1, x0:x1] != 0).all() == passes and (a["map"][y0:y1, x0:x1] != 0).any() == passes
        assert all((t["rx"] > t["ry"]) == (ru > rv) for t in mine)
    assert {t["L0"] for t in details} == {0, 1, 2} and min(t["fw"] for t in details) == 0
    assert any(t["fw"] < 128 for t in details if t["L0"] == 0 and t["fw"]) and any(t["fw"] > 128 for t in details if t["L0"] == 0)
    assert any(t["fw"] < 128 for t in details if t["L0"] == 1) and any(t["fw"] > 128 for t in details if t["L0"] == 1)


def _check_cutoff_values(runs):
    case, tex, _, a, o, _ = runs[0]
    assert tex["texture_count"] == 2 and tex["textures"][1, 1] == 0 and aref.usable(tex, 1) is None and aref.usable(tex, 7) is None
    want = {0: "all", 1: "some", 128: "some", 255: "some", 300: "none"}
    for k, (texture, word) in enumerate(CUTOFF_DRAWS):
        x0, y0, x1, y1 = (int(v) for v in _cutoff_quad_box(k))
        box = a["map"][y0:y1, x0:x1]
        kind = want[word] if texture == 0 else ("all" if word <= 255 else "none")
        covered = int((box != 0).sum())
        assert {"all": covered == box.size, "none": covered == 0, "some": 0 < covered < box.size}[kind], (k, covered)
        if kind != "all":
            assert (o["map"][y0:y1, x0:x1] != 0).all()
    counts = [int((a["map"][5:30, 2 + 8 * k:10 + 8 * k] != 0).sum()) for k in range(5)]
    assert counts[0] > counts[1] > counts[2] > counts[3] > counts[4] == 0, counts
    assert counts[3] == 8, "alpha 255 is reached on the one row of pixel centres that lies on the centres of the texel row"


def _check_uv_edges(runs):
    case, tex, _, a, o, details = runs[0]
    assert tex["uvs"].shape[0] == case["positions"].shape[0] - 2
    by_draw = {k: [t for t in details if t["draw"] == k] for k in range(len(UV_EDGE_PARTS))}
    part = {name: k for k, name in enumerate(UV_EDGE_PARTS)}
    for name in ("negative", "above_one", "non_power_of_two", "one_level", "outside_uvs"):
        assert all(0 < t["passed"] < t["fragments"] for t in by_draw[part[name]]), name
    first = 6 * part["negative"]
    assert (tex["uvs"][first:first + 6] < 0).all() and (tex["uvs"][6 * part["above_one"]:6 * part["above_one"] + 6] > 1).all()
    far = by_draw[part["past_2_20"]]
    assert all(t["invalid"] > 50 and t["fragments"] - t["invalid"] > 50 and 0 < t["passed"] < t["fragments"] for t in far)
    assert (a["map"][4:28, 77:88] != 0).all(), "a fragment that is not valid samples (0, 0), whose blend reaches the cutoff"
    assert all(t["passed"] == t["fragments"] for t in by_draw[part["one_by_one_kept"]]) and all(t["passed"] == 0 for t in by_draw[part["one_by_one_dropped"]])
    assert tuple(tex["textures"][1, 1:].tolist()) == (5, 3, 3) and tuple(tex["textures"][2, 1:].tolist()) == (1, 1, 1)
    assert all(t["L0"] == 0 and t["fw"] == 0 and t["lod"] == 0.0 and t["rx"] > 8.9 for t in by_draw[part["one_level"]]), "the level is clamped to the chain's only one"
    whole = aref.rasterise(case, dict(tex, uvs=np.concatenate([tex["uvs"], np.ones((2, 2), F32)])))
    assert not np.array_equal(whole["map"], a["map"]), "the two vertices outside uvs count as (0, 0)"


def _check_transformed(runs):
    case, tex, _, a, o, details = runs[0]
    assert not ref.is_affine(case["light"]) or not np.array_equal(case["light"], sc.IDENTITY)
    assert a["rejects"] == 0 and 0 < a["drawn"] < a["submitted"], "front faces are culled"
    for d in (3, 4):  # a two-sided card: exactly one winding of each of its two triangles is drawn
        r, solid, _ = _alone(case, tex, d)
        assert r["submitted"] == 4 and r["drawn"] == 2 and 50 < r["passed"] < r["tested"] - 50
    assert {t["draw"] for t in details} == {0, 1, 3, 4}, "the torus has no texture: it is not sampled"
    assert len({t["L0"] for t in details}) >= 2


CHECKS = {"cutout_over_opaque": _check_cutout_over_opaque, "stacked": _check_stacked, "paths": _check_paths, "mip_threshold": _check_mip_threshold,
          "cutoff_values": _check_cutoff_values, "uv_edges": _check_uv_edges, "transformed": _check_transformed}


def check_case_is_what_it_is_for(name):
    runs = reference(name)
    for case, tex, _, a, o, _ in runs:
        assert case["res"] <= 160
        assert (a["submitted"], a["drawn"], a["rejects"]) == (o["submitted"], o["drawn"], o["rejects"]), "the counters do not depend on alpha"
    CHECKS[name](runs)
