"""Inputs of the normal map tests of "depthPrepassRaster.comp" (tests/test_prepass_normal.py, tests/test_prepass_normal_cpu.py): named cases at the smallest
shapes at which the shading normal can still go wrong, each with a check, on the reference alone (tests/prepass_normal_reference.py), that it is what it is for.

A case is a list of runs (prepass case, texture inputs, normal inputs, cutoffs or None): the dicts of tests/prepass_raster_cases.py, tests/prepass_texture_reference.py
and tests/prepass_normal_reference.py, and for an alpha-tested run one uint32 cutoff word per draw.
  flat_codes          16 x 16, 7 texels x 2 decodes: vertex normal (0, 0, 1), tangent (1, 0, 0), bitangent (0, 1, 0), identity model, a constant normal texture;
                      the word is computed by hand. (255, 0) in the reference's decode has the radicand 0, (255, 128) and others in the unit decode q < 0
  fallback_zero       16 x 16: zero tangents and bitangents, unit decode, texel (255, 255): M is exactly zero, shadingNormal == normal
  interpolated_basis  32 x 32: vertex normals and tangents that differ across each triangle: normalising T, B, Nv before the multiply would show
  model_matrix        32 x 32: a rotation with non-uniform scale as the model matrix (T_k is normalised after mat3(model))
  perspective         32 x 32, mip bias 0 and +1.5: the floor quad of the texture cases (a vertex at w <= 0), a normal texture whose levels have distinct texels
  material_mix        48 x 16, three draws: normal-mapped, none, an index >= textureCount
  with_alpha          16 x 16: a cutout card with a normal map in front of a second normal-mapped quad
  ragged              70 x 66: one triangle over every pixel
  hazard_*            raw records: tangents shorter than positions; an unusable table entry; a texelOffset that leaves texels half way; normalMaterials shorter
                      than the draw count (the launcher refuses it; the reference stores `normal`); NaN and infinite tangents
"""
import numpy as np

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_raster_reference as ref
import prepass_texture_cases as tc
import prepass_texture_reference as tref
from shadow_raster_cases import quad

F32 = np.float32
NONE = tref.NONE
REFERENCE, UNIT = nref.DECODE_REFERENCE, nref.DECODE_UNIT
FLAT_TEXELS = ((128, 128), (255, 128), (0, 128), (128, 0), (128, 255), (255, 0), (255, 255))


def normal_inputs(case, tangents, bitangents, normal_materials, decode):
    n = case["positions"].shape[0]
    return dict(tangents=np.broadcast_to(np.asarray(tangents, F32), (n, 3)).copy() if np.asarray(tangents).ndim == 1 else np.asarray(tangents, F32).reshape(-1, 3),
                bitangents=np.broadcast_to(np.asarray(bitangents, F32), (n, 3)).copy() if np.asarray(bitangents).ndim == 1 else np.asarray(bitangents, F32).reshape(-1, 3),
                normal_materials=np.asarray(normal_materials, np.uint32).reshape(-1), decode=int(decode))


def with_normals(case, normals):
    n = case["positions"].shape[0]
    normals = np.asarray(normals, F32)
    return dict(case, normals=np.broadcast_to(normals, (n, 3)).copy() if normals.ndim == 1 else normals.reshape(-1, 3))


def constant_texture(cx, cy):
    return np.array([0xFF000000 | (77 << 16) | (cy << 8) | cx], np.uint32), 1, 1, 1


def steep(width, height, salt):
    """tc.pattern: R and G jump by tens of codes from texel to texel - a steep normal map"""
    return tc.chain(tc.pattern(width, height, salt), width, height), width, height, tref.full_mip_count(width, height)


def _flat(cx, cy, decode):
    case = with_normals(pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16), (0.0, 0.0, 1.0))
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    case, tex = tc.textured(case, uvs, [(NONE, NONE)], [constant_texture(cx, cy)])
    return case, tex, normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), [0], decode), None


def _flat_codes():
    return [_flat(cx, cy, decode) for decode in (REFERENCE, UNIT) for cx, cy in FLAT_TEXELS]


def _fallback_zero():
    case, tex, nm, _ = _flat(255, 255, UNIT)
    return [(case, tex, normal_inputs(case, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), [0], UNIT), None)]


def _unit_rows(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def _interpolated_basis():
    """per vertex of the two triangles: normals tilted by up to ~35 degrees, tangents turned about z by -70 .. +70 degrees - the interpolated T is much shorter
    than 1 inside the triangle while Nv is not, so the proportions of M change when they are normalised first"""
    case = pc.pixel_case([quad(0.0, 0.0, 32.0, 32.0, 0.5, 0.5)], 32, 32)
    normals = _unit_rows([(0.6, 0.0, 1.0), (-0.5, 0.3, 1.0), (0.0, -0.7, 1.0), (0.2, 0.6, 1.0), (-0.6, -0.2, 1.0), (0.4, -0.4, 1.0)])
    angles = np.radians([-70.0, 0.0, 70.0, 60.0, -60.0, 10.0])
    tangents = np.stack([np.cos(angles), np.sin(angles), np.zeros(6)], axis=1).astype(F32)
    bitangents = np.stack([-np.sin(angles), np.cos(angles), np.zeros(6)], axis=1).astype(F32)
    case = with_normals(case, normals)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 32.0, y / 32.0))
    case, tex = tc.textured(case, uvs, [(NONE, NONE)], [steep(8, 8, 61)])
    return [(case, tex, normal_inputs(case, tangents, bitangents, [0], decode), None) for decode in (REFERENCE, UNIT)]


def _model_matrix():
    case = with_normals(pc.pixel_case([quad(0.0, 0.0, 32.0, 32.0, 0.5, 0.5)], 32, 32), (0.0, 0.0, 1.0))
    a, c = np.radians(35.0), np.radians(20.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rx = np.array([[1, 0, 0, 0], [0, np.cos(c), -np.sin(c), 0], [0, np.sin(c), np.cos(c), 0], [0, 0, 0, 1]])
    model = pc.glm(rz @ rx @ np.diag([3.0, 0.25, 1.5, 1.0]))
    transforms = case["transforms"].copy()
    transforms[:, 0:16] = model  # the record's model is independent of its mvp: the quad stays where it is on the screen
    case = dict(case, transforms=transforms)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    case, tex = tc.textured(case, uvs, [(NONE, NONE)], [steep(16, 16, 62)])
    tangents = _unit_rows([(1.0, 0.4, 0.2)])[0]
    return [(case, tex, normal_inputs(case, tangents, (0.0, 1.0, 0.0), [0], decode), None) for decode in (REFERENCE, UNIT)]


LEVEL_TEXELS = [(30 + 32 * l, 240 - 35 * l) for l in range(7)]


def _level_normal_texture():
    return np.concatenate([np.full(tref.level_size(64, 64, l)[0] ** 2, 0xFF000000 | (cy << 8) | cx, np.uint32) for l, (cx, cy) in enumerate(LEVEL_TEXELS)]), 64, 64, 7


def _perspective():
    runs = []
    for bias in (0.0, 1.5):
        (case, tex), = tc._perspective()
        case, tex = tc.textured(case, tex["uvs"], [(NONE, NONE)], [_level_normal_texture()], mip_bias=bias)
        runs.append((case, tex, normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), [0], REFERENCE if bias == 0.0 else UNIT), None))
    return runs


def _three_quads():
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5), quad(32.0, 0.0, 48.0, 16.0, 0.5, 0.5)], 48, 16)
    return with_normals(case, _unit_rows([(0.1, 0.2, 1.0)])[0])


def _material_mix():
    case = _three_quads()
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    case, tex = tc.textured(case, uvs, [(0, NONE), (NONE, NONE), (NONE, 1)], [steep(8, 8, 63), steep(8, 4, 64)])
    return [(case, tex, normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), [1, NONE, 2], UNIT), None)]


def _with_alpha(front_cutoff=ac.REFERENCE_CUTOFF):
    """draw 0 the rear quad, draw 1 the card in front of it: a 0 / 255 checker alpha in cells of 2 texels, 8 x 8 texels over the 16 x 16 pixels"""
    case = with_normals(pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.3, 0.3), quad(0.0, 0.0, 16.0, 16.0, 0.6, 0.6)], 16, 16), (0.0, 0.0, 1.0))
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    card = ac.checker(8, 8, 2, 65)
    textures = [(tc.chain(card, 8, 8), 8, 8, 4), steep(8, 8, 66), steep(4, 4, 67)]
    case, tex = tc.textured(case, uvs, [(NONE, NONE), (0, NONE)], textures)
    return [(case, tex, normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), [1, 2], REFERENCE), np.array([0, front_cutoff], np.uint32))]


def _ragged():
    (case, tex), = tc._ragged()
    case = with_normals(case, _unit_rows([(0.3, -0.2, 1.0), (-0.4, 0.1, 1.0), (0.0, 0.5, 1.0)]))
    tangents = _unit_rows([(1.0, 0.0, -0.3), (1.0, 0.2, 0.4), (1.0, -0.3, 0.0)])
    return [(case, tex, normal_inputs(case, tangents, nref.derive_bitangents(tangents, case["normals"]), [1], decode), None) for decode in (REFERENCE, UNIT)]


def _hazard_quads(normal_materials, textures, tangents=(1.0, 0.0, 0.0), bitangents=(0.0, 1.0, 0.0), texture_count=None):
    case = with_normals(pc.pixel_case([quad(0.0, 0.0, 8.0, 16.0, 0.5, 0.5), quad(8.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16), (0.0, 0.0, 1.0))
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 8.0, y / 8.0))
    case, tex = tc.textured(case, uvs, [(NONE, NONE), (NONE, NONE)], textures, texture_count=texture_count)
    return case, tex, normal_inputs(case, tangents, bitangents, normal_materials, UNIT), None


def _hazard_short_tangents():
    case, tex, nm, _ = _hazard_quads([0, 0], [steep(4, 4, 68)])
    return [(case, tex, dict(nm, tangents=nm["tangents"][:6].copy()), None)]  # draw 1's vertices 6 .. 11 have (0, 0, 0)


def _hazard_entry():
    table, texels = tc.texture_set([steep(4, 4, 69), steep(4, 4, 70)])
    table[0, 1] = 0  # width 0
    return [_hazard_quads([0, 1], (table, texels))]


def _hazard_offset():
    table, texels = tc.texture_set([steep(4, 4, 71), steep(4, 4, 72)])
    table[1, 0] = texels.size - 8  # level 0's second half and the levels above lie past the end
    return [_hazard_quads([0, 1], (table, texels))]


def _hazard_short_materials():
    case, tex, nm, _ = _hazard_quads([0, 0], [steep(4, 4, 73)])
    return [(case, tex, dict(nm, normal_materials=nm["normal_materials"][:1].copy()), None)]


def _hazard_nan_tangents():
    case, tex, nm, _ = _hazard_quads([0, 0], [steep(4, 4, 74)])
    tangents = nm["tangents"].copy()
    tangents[1, 0] = np.nan   # a vertex of draw 0's first triangle
    tangents[7, 1] = np.inf   # and one of draw 1's
    return [(case, tex, dict(nm, tangents=tangents), None)]


CASES = dict(flat_codes=_flat_codes, fallback_zero=_fallback_zero, interpolated_basis=_interpolated_basis, model_matrix=_model_matrix, perspective=_perspective,
             material_mix=_material_mix, with_alpha=_with_alpha, ragged=_ragged, hazard_short_tangents=_hazard_short_tangents, hazard_entry=_hazard_entry,
             hazard_offset=_hazard_offset, hazard_short_materials=_hazard_short_materials, hazard_nan_tangents=_hazard_nan_tangents)
REFUSED_BY_THE_LAUNCHER = ("hazard_short_materials",)

_reference_cache = {}


def base_images(case, tex, cutoffs):
    """the pass without normal maps: the alpha reference's result, or the raster reference's with the sampled albedo and specular"""
    if cutoffs is not None:
        return aref.render(case, tex, cutoffs)
    r = pc.rasterise(case)
    s = tref.sample(case, tex, r["keys"])
    return dict(r, albedo=s["albedo"], specular=s["specular"])


def reference(name):
    """[(case, texture inputs, normal inputs, cutoffs, the pass without normal maps, shadingNormal, details)], computed once; callers must not modify it"""
    if name not in _reference_cache:
        out = []
        for case, tex, nm, cutoffs in CASES[name]():
            base = base_images(case, tex, cutoffs)
            details = {}
            out.append((case, tex, nm, cutoffs, base, nref.shade(case, tex, nm, base["keys"], base["normal"], details=details), details))
        _reference_cache[name] = out
    return _reference_cache[name]


def differing_share(runs):
    """over all runs of a case: the share of winner pixels with shadingNormal != normal"""
    winners = sum(int((base["keys"] != 0).sum()) for _, _, _, _, base, _, _ in runs)
    differing = sum(int(((base["keys"] != 0) & (sn != base["normal"])).sum()) for _, _, _, _, base, sn, _ in runs)
    return differing / max(winners, 1)


def unorm8_half(n):
    """n * 0.5 + 0.5 by the UNORM8 rule, on Python floats rounded to fp32 where the contract rounds"""
    v = F32(F32(F32(n) * F32(0.5)) + F32(0.5))
    return int(np.rint(F32(min(max(v, F32(0)), F32(1))) * F32(255.0)))


def flat_word(cx, cy, decode):
    """the word of a flat_codes run from math.sqrt and Python floats: with T = (1, 0, 0), B = (0, 1, 0), Nv = (0, 0, 1), M is n_t"""
    import math
    x, y = cx / 255.0, cy / 255.0
    if decode == REFERENCE:
        m = (2.0 * x - 1.0, 2.0 * y - 1.0, 2.0 * math.sqrt(((1.0 - x * x) + y) + y) - 1.0)
    else:
        nx, ny = 2.0 * x - 1.0, 2.0 * y - 1.0
        q = (1.0 - nx * nx) - ny * ny
        m = (nx, ny, math.sqrt(q) if q > 0 else 0.0)
    length = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    n = tuple(v / length for v in m)
    return unorm8_half(n[0]) | (unorm8_half(n[1]) << 8) | (unorm8_half(n[2]) << 16) | (255 << 24)


def _check_flat_codes(runs):
    assert len(runs) == 14
    combos = [(decode, texel) for decode in (REFERENCE, UNIT) for texel in FLAT_TEXELS]
    for (decode, (cx, cy)), (case, tex, nm, cutoffs, base, sn, d) in zip(combos, runs):
        assert nm["decode"] == decode and (base["keys"] != 0).all() and d["mapped"].all() and not d["fallback"].any()
        assert (sn == flat_word(cx, cy, decode)).all(), "texel (%d, %d), decode %d: %08x, by hand %08x" % (cx, cy, decode, int(sn[0, 0]), flat_word(cx, cy, decode))
        if decode == REFERENCE and (cx, cy) == (255, 0):
            assert np.array_equal(d["nt"][0, 0], [1.0, -1.0, -1.0]), "the radicand is 0"
        if decode == UNIT and (cx, cy) in ((255, 128), (255, 0), (255, 255)):
            assert d["nt"][0, 0, 2] == 0.0, "q < 0: nz = 0"


def _check_fallback_zero(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert (base["keys"] != 0).all() and d["mapped"].all() and d["fallback"].all(), "M is exactly zero on every winner pixel"
    assert np.array_equal(sn, base["normal"]) and (sn != 0).all()


def _check_interpolated_basis(runs):
    for case, tex, nm, cutoffs, base, sn, d in runs:
        winners = base["keys"] != 0
        other = nref.shade(case, tex, nm, base["keys"], base["normal"], variant="normalised")
        assert ((other != sn) & winners).sum() >= winners.sum() / 10, "normalising T, B and Nv first shows on %d of %d pixels" % (((other != sn) & winners).sum(), winners.sum())


def _check_model_matrix(runs):
    for case, tex, nm, cutoffs, base, sn, d in runs:
        model = case["transforms"][0, 0:16].reshape(4, 4).T[:3, :3].astype(np.float64)
        lengths = np.linalg.norm(model, axis=0)
        assert lengths.max() / lengths.min() > 4 and abs(model[0, 1]) > 0.1, "non-uniform scale and a rotation"
        plain = nref.shade(dict(case, transforms=pc.identity_matrices(1)), tex, nm, base["keys"], base["normal"])
        assert ((plain != sn) & (base["keys"] != 0)).sum() > 500, "the model matrix shows"


def _check_perspective(runs):
    assert [tex["mip_bias"] for _, tex, _, _, _, _, _ in runs] == [0.0, 1.5]
    for case, tex, nm, cutoffs, base, sn, d in runs:
        clip = ref.transform4(case["transforms"][0, 16:32], case["positions"])
        assert (clip[:, 3] <= 0).any() and base["clipped"] >= 1
        covered = base["keys"] != 0
        assert covered.sum() > 200 and np.unique(d["L0"][covered]).size >= 4, "the level varies over the image"
    assert not np.array_equal(runs[0][6]["L0"], runs[1][6]["L0"])


def _check_material_mix(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert nm["normal_materials"].tolist() == [1, NONE, 2] and tex["texture_count"] == 2
    assert d["mapped"][:, :16].all() and not d["mapped"][:, 16:].any()
    assert np.array_equal(sn[:, 16:], base["normal"][:, 16:]) and np.unique(sn[:, :16]).size > 8


def _check_with_alpha(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    own = aref.winner_draw(case, base["keys"])
    assert (own == 0).sum() > 40 and (own == 1).sum() > 40, "the card and, through its holes, the rear quad"
    (_, _, _, _, rear_base, rear, _), = [(c, t, n, k, b, nref.shade(c, t, n, b["keys"], b["normal"]), None) for c, t, n, k in _with_alpha(300)
                                         for b in [base_images(c, t, k)]]
    assert (aref.winner_draw(case, rear_base["keys"]) == 0).all()
    assert np.array_equal(sn[own == 0], rear[own == 0]), "the holes hold the rear quad's shading normal"
    assert (sn[own == 1] != rear[own == 1]).sum() > 30


def _check_ragged(runs):
    for case, tex, nm, cutoffs, base, sn, d in runs:
        assert (case["width"], case["height"]) == (70, 66) and (base["keys"] != 0).all() and np.unique(sn).size > 100


def _check_hazard_short_tangents(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert nm["tangents"].shape[0] == 6 < case["positions"].shape[0] and d["mapped"].all()
    full, = _hazard_quads([0, 0], [steep(4, 4, 68)])[2:3]
    other = nref.shade(case, tex, full, base["keys"], base["normal"])
    assert np.array_equal(other[:, :8], sn[:, :8]) and (other[:, 8:] != sn[:, 8:]).sum() > 30, "draw 1's tangents are (0, 0, 0)"


def _check_hazard_entry(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert tref.usable(tex, 0) is None and not d["mapped"][:, :8].any() and d["mapped"][:, 8:].all()
    assert np.array_equal(sn[:, :8], base["normal"][:, :8]) and (sn[:, 8:] != base["normal"][:, 8:]).sum() > 30


def _check_hazard_offset(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    right = d["nt"][:, 8:, 0]
    assert (right == -1.0).any() and (right != -1.0).any(), "texels past the end read 0: code 0 decodes to -1; half of level 0 lies inside"


def _check_hazard_short_materials(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert nm["normal_materials"].size == 1 < case["draws"].shape[0]
    assert d["mapped"][:, :8].all() and not d["mapped"][:, 8:].any() and np.array_equal(sn[:, 8:], base["normal"][:, 8:])


def _check_hazard_nan_tangents(runs):
    (case, tex, nm, cutoffs, base, sn, d), = runs
    assert np.isnan(nm["tangents"]).sum() == 1 and np.isinf(nm["tangents"]).sum() == 1
    assert (sn >> np.uint32(24) == 255).all() and d["mapped"].all(), "every pixel holds a word: a non-finite T_k normalises to (0, 0, 0)"
    clean, = _hazard_quads([0, 0], [steep(4, 4, 74)])[2:3]
    assert (nref.shade(case, tex, clean, base["keys"], base["normal"]) != sn).sum() > 30


CASE_CHECKS = {name: globals()["_check_" + name] for name in CASES}
MINIMUM_DIFFERING_SHARE = 0.25


def check_case_is_what_it_is_for(name):
    runs = reference(name)
    CASE_CHECKS[name](runs)
    if not name.startswith("hazard_") and name != "fallback_zero":
        share = differing_share(runs)
        assert share >= MINIMUM_DIFFERING_SHARE, "%s: shadingNormal differs from normal on %.0f %% of the winner pixels only" % (name, 100 * share)
