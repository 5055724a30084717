"""Inputs of the alpha test's tests of "depthPrepassRaster.comp" (tests/test_prepass_alpha.py, tests/test_prepass_alpha_cpu.py): named cases a few tiles large,
each with a check, on the reference alone (tests/prepass_alpha_reference.py), that the case exercises what it is named for.

A case is a list of runs (prepass case, texture inputs, cutoffs): the dicts of tests/prepass_raster_cases.py and tests/prepass_texture_reference.py and one
uint32 cutoff word per draw. Depth is reverse Z: the larger z is in front.
  cutout_over_opaque  70 x 50: a tested quad with a checker alpha in front of an opaque quad and partly over nothing
  stacked             70 x 50: three tested layers with different textures and cutoffs
  tie                 70 x 50: two coplanar triangles with bit-equal depth, the later one tested
  paths               200 x 40: tested triangles through the lane path (narrow and int64), the wave path across a tile boundary (narrow) and the wave path with a
                      span >= 2^15 sub-pixel units (int64); opaque draws in the same execution, and a draw without triangles
  clipped             70 x 50: a tested floor from behind the camera (vertices with w <= 0), fanned into sub-triangles
  mip_threshold       70 x 50, three runs (mip_bias -1, 0, +1): a 0 / 255 checker whose chain is 128 from level 1 on, minified by seven ratios, cutoff 128
  cutoff_values       70 x 50: cutoffs 0, 1, 128, 255 and 300 on copies of one draw; constant-word draws below, at and above their cutoff; an unusable texture
"""
import numpy as np

import prepass_alpha_reference as aref
import prepass_raster_cases as pc
import prepass_raster_reference as ref
import prepass_texture_cases as tc
import prepass_texture_reference as tref
from shadow_raster_cases import quad

F32 = np.float32
NONE = tref.NONE
REFERENCE_CUTOFF = 128


def checker(width, height, cell, salt, phase=0):
    """tc.pattern's colours with an alpha of 0 / 255 in cells of `cell` texels"""
    y, x = np.mgrid[0:height, 0:width]
    alpha = np.where(((x // cell) + (y // cell) + phase) % 2 == 0, 255, 0).astype(np.uint32).reshape(-1)
    return (tc.pattern(width, height, salt) & np.uint32(0x00FFFFFF)) | (alpha << np.uint32(24))


def _full(level0, width, height):
    return tc.chain(level0, width, height), width, height, tref.full_mip_count(width, height)


def _with_alpha(case, alphas):
    """the case with the constant albedo words' alpha replaced: {draw: alpha code}"""
    draws = case["draws"].copy()
    for d, a in alphas.items():
        draws[d, 4] = (int(draws[d, 4]) & 0x00FFFFFF) | (int(a) << 24)
    return dict(case, draws=draws)


def _cutout_over_opaque():
    case = pc.pixel_case([quad(20.0, 5.0, 60.0, 45.0, 0.3, 0.3), quad(5.0, 10.0, 45.0, 40.0, 0.6, 0.6)], 70, 50)
    uvs = tc.quad_uvs(case, [lambda x, y: (x * 0.0, y * 0.0), lambda x, y: ((x - 5.0) / 40.0, (y - 10.0) / 30.0)])  # 8 x 8 texels over 40 x 30 pixels
    case, tex = tc.textured(case, uvs, [(NONE, NONE), (0, NONE)], [_full(checker(8, 8, 2, 41), 8, 8)])
    return [(case, tex, np.array([0, REFERENCE_CUTOFF], np.uint32))]


def _stacked():
    case = pc.pixel_case([quad(4.0, 4.0, 66.0, 46.0, 0.3, 0.35), quad(8.0, 2.0, 62.0, 48.0, 0.5, 0.5), quad(2.0, 8.0, 68.0, 42.0, 0.7, 0.65)], 70, 50)
    uvs = tc.quad_uvs(case, [lambda x, y: (x / 35.0, y / 25.0), lambda x, y: (x / 20.0, y / 20.0), lambda x, y: (x / 50.0, y / 30.0)])
    textures = [_full(checker(8, 8, 1, 42), 8, 8), _full(checker(4, 4, 1, 43, phase=1), 4, 4), _full(checker(16, 8, 2, 44), 16, 8)]
    case, tex = tc.textured(case, uvs, [(0, 0), (1, NONE), (2, 1)], textures)
    return [(case, tex, np.array([REFERENCE_CUTOFF, 100, 200], np.uint32))]


TIE_TRIANGLE = [(6.0, 4.0, 0.5), (64.0, 4.0, 0.5), (64.0, 46.0, 0.5)]


def _tie():
    case = pc.pixel_case([[TIE_TRIANGLE], [TIE_TRIANGLE]], 70, 50)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 24.0, y / 24.0))
    case, tex = tc.textured(case, uvs, [(NONE, NONE), (0, NONE)], [_full(checker(8, 8, 2, 45), 8, 8)])
    return [(case, tex, np.array([0, REFERENCE_CUTOFF], np.uint32))]


# (name, triangle): where each tested triangle of `paths` is meant to go
PATH_TRIANGLES = [("lane", [(10.25, 5.5, 0.6), (13.75, 5.5, 0.6), (13.75, 9.0, 0.6)]),                     # a 4 x 4 box
                  ("wave_narrow", [(40.0, 4.0, 0.6), (90.0, 6.0, 0.7), (84.0, 36.0, 0.5)]),                # 50 pixels wide, across x = 64
                  ("wave_int64", [(20.0, 14.0, 0.55), (190.0, 16.0, 0.65), (150.0, 38.0, 0.6)]),           # 170 pixels wide: a span of 43520 >= 2^15
                  ("lane_int64", [(61.0, 1.0, 0.8), (199.0, 1.0, 0.8), (61.0, 5.0, 0.8)])]                 # in tile 0 a 3 x 4 box; 138 pixels wide


def _paths():
    groups = [quad(0.0, 0.0, 200.0, 40.0, 0.2, 0.25), [t for _, t in PATH_TRIANGLES[:2]], [], [[(100.0, 2.0, 0.9), (140.0, 2.0, 0.9), (140.0, 30.0, 0.9)]],
              [t for _, t in PATH_TRIANGLES[2:]]]
    case = pc.pixel_case(groups, 200, 40)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    textures = [_full(checker(8, 8, 1, 46), 8, 8), _full(checker(8, 8, 2, 47), 8, 8)]
    case, tex = tc.textured(case, uvs, [(1, NONE), (0, NONE), (0, 0), (NONE, 1), (1, 0)], textures)
    return [(case, tex, np.array([0, REFERENCE_CUTOFF, REFERENCE_CUTOFF, 0, 90], np.uint32))]


CLIPPED_FLOOR = np.array([[-3.0, 1.5, -5.0], [3.0, 1.5, -5.0], [3.0, 1.5, 60.0], [-3.0, 1.5, 60.0]], F32)  # a strip from behind the camera into the distance


def _clipped():
    cam = pc.camera(aspect=70 / 50, near=0.1, far=300.0)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    case = pc.make_case(70, 50, ref.main_pass_matrices(vp, vp, [pc.IDENTITY]), CLIPPED_FLOOR, [0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3], [[0, 12, 0, 0]])  # both windings
    uvs = np.stack([CLIPPED_FLOOR[:, 0] / F32(3.0), CLIPPED_FLOOR[:, 2] / F32(3.0)], axis=1)
    case, tex = tc.textured(case, uvs, [(0, NONE)], [_full(checker(16, 16, 2, 48), 16, 16)])
    return [(case, tex, np.array([REFERENCE_CUTOFF], np.uint32))]


MIP_RATIOS = (0.8, 1.0, 1.25, 1.5, 2.0, 2.6, 3.4)  # texels per pixel of the seven quads
MIP_BIASES = (-1.0, 0.0, 1.0)


def _mip_threshold():
    case = pc.pixel_case([quad(10.0 * k, 0.0, 10.0 * k + 10.0, 50.0, 0.5, 0.5) for k in range(7)], 70, 50)
    uvs = tc.quad_uvs(case, [(lambda x, y, r=r: (r * x / 16.0, r * y / 16.0)) for r in MIP_RATIOS])
    texture = _full(checker(16, 16, 1, 49), 16, 16)
    return [tc.textured(case, uvs, [(0, NONE)] * 7, [texture], mip_bias=bias) + (np.full(7, REFERENCE_CUTOFF, np.uint32),) for bias in MIP_BIASES]


CUTOFF_WORDS = (0, 1, 128, 255, 300)
CONSTANT_DRAWS = ((100, 128), (128, 128), (200, 128))  # (constant alpha, cutoff): below, at, above
UNUSABLE_DRAW = (0x60, 0x60)                           # its albedo word names a table entry of width 0: the constant word, at its cutoff


RAMP_ROWS = (0, 0, 0, 127, 127, 127, 128, 128, 128, 255, 255, 255, 1, 1, 1, 0)


def ramp(width, height, salt):
    """16 rows of constant alpha, three of each code of interest: a pixel whose two rows of taps fall inside one run has exactly that code"""
    assert height == len(RAMP_ROWS)
    alpha = np.repeat(np.asarray(RAMP_ROWS, np.uint32), width)
    return (tc.pattern(width, height, salt) & np.uint32(0x00FFFFFF)) | (alpha << np.uint32(24))


def _cutoff_values():
    cells = [(14.0 * (k % 5), 25.0 * (k // 5)) for k in range(9)]
    case = pc.pixel_case([quad(x, y, x + 14.0, y + 25.0, 0.5, 0.5) for x, y in cells], 70, 50)
    uvs = tc.quad_uvs(case, [(lambda x, y, c=c: ((x - c[0]) / 14.0, (y - c[1]) / 25.0)) for c in cells])  # 16 x 16 texels over 14 x 25 pixels: level 0
    table, texels = tc.texture_set([(ramp(16, 16, 50), 16, 16, 1), _full(checker(4, 4, 1, 51), 4, 4)])
    table[1, 1] = 0  # unusable
    case = _with_alpha(case, {5: CONSTANT_DRAWS[0][0], 6: CONSTANT_DRAWS[1][0], 7: CONSTANT_DRAWS[2][0], 8: UNUSABLE_DRAW[0]})
    case, tex = tc.textured(case, uvs, [(0, NONE)] * 5 + [(NONE, 0)] * 3 + [(1, NONE)], (table, texels))
    return [(case, tex, np.array(list(CUTOFF_WORDS) + [c for _, c in CONSTANT_DRAWS] + [UNUSABLE_DRAW[1]], np.uint32))]


CASES = dict(cutout_over_opaque=_cutout_over_opaque, stacked=_stacked, tie=_tie, paths=_paths, clipped=_clipped, mip_threshold=_mip_threshold,
             cutoff_values=_cutoff_values)

_reference_cache = {}


def reference(name):
    """[(case, texture inputs, cutoffs, the alpha reference's result, the textured reference without the test)], computed once; callers must not modify it"""
    if name not in _reference_cache:
        out = []
        for case, tex, cutoffs in CASES[name]():
            opaque = pc.rasterise(case, diagnostics=True)
            s = tref.sample(case, tex, opaque["keys"])
            out.append((case, tex, cutoffs, aref.render(case, tex, cutoffs), dict(opaque, albedo=s["albedo"], specular=s["specular"])))
        _reference_cache[name] = out
    return _reference_cache[name]


def _fragment_sets(a, draw=None):
    """over the tested fragments (of `draw`): the masks of those that pass and of those that fail, summed per pixel"""
    shape = a["keys"].shape
    passed, failed = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for f in a["fragments"]:
        if draw is None or f["draw"] == draw:
            ok = f["alpha"].astype(np.int64) >= f["cutoff"]
            passed += f["covered"] & ok
            failed += f["covered"] & ~ok
    return passed, failed


def _check_cutout_over_opaque(runs):
    (case, tex, cutoffs, a, o), = runs
    own = aref.winner_draw(case, a["keys"])
    passed, failed = _fragment_sets(a, 1)
    assert (own == 1).sum() > 100, "pixels won by the front"
    assert ((own == 0) & (failed > 0)).sum() > 100, "pixels won by the back through a hole"
    assert ((own == -1) & (failed > 0)).sum() > 50, "sky through a hole"
    assert (aref.winner_draw(case, o["keys"])[failed > 0] == 1).all(), "without the test the front would have won them"
    assert not np.array_equal(a["depth"], o["depth"]) and not np.array_equal(a["albedo"], o["albedo"])


def _check_stacked(runs):
    (case, tex, cutoffs, a, o), = runs
    own = aref.winner_draw(case, a["keys"])
    assert all((own == d).sum() > 50 for d in range(3)), "each layer wins somewhere: %r" % ([int((own == d).sum()) for d in range(3)],)
    failed = [_fragment_sets(a, d)[1] > 0 for d in range(3)]
    assert (failed[0] & failed[1] & failed[2] & (own == -1)).sum() > 20, "some pixels fail all three"
    assert len(set(int(c) for c in cutoffs)) == 3 and len(set(int(m) for m in tex["materials"][:, 0])) == 3


def _check_tie(runs):
    (case, tex, cutoffs, a, o), = runs
    own = aref.winner_draw(case, a["keys"])
    both = o["coverage"] == 2
    assert both.sum() > 500 and np.unique(a["depth"][both]).size == 1, "bit-equal depth"
    assert (aref.winner_draw(case, o["keys"])[both] == 1).all(), "untested, the later one wins every pixel"
    passed, failed = _fragment_sets(a, 1)
    assert (own[failed > 0] == 0).all() and (failed > 0).sum() > 100, "where the later one fails the earlier one wins"
    assert (own[passed > 0] == 1).all() and (passed > 0).sum() > 100, "where it passes it wins"


def path_of(fan, tile_x):
    """(lane | wave, narrow | int64) of a drawn sub-triangle (a fan_drawn entry) in the tile column tile_x, None where its box does not reach it"""
    _, _, (ix0, iy0, ix1, iy1), (span_x, span_y) = fan
    x0, x1 = max(ix0, 64 * tile_x), min(ix1, 64 * tile_x + 63)
    if x0 > x1:
        return None
    return ("lane" if x1 - x0 < 4 and iy1 - iy0 < 4 else "wave", "narrow" if span_x < 32768 and span_y < 32768 else "int64")


def _check_paths(runs):
    (case, tex, cutoffs, a, o), = runs
    assert case["width"] == 200 and case["height"] == 40 and (case["draws"][:, 1] == 0).sum() == 1, "one tile row (height <= 64), and a draw without triangles"
    own = aref.winner_draw(case, a["keys"])
    first = np.concatenate([[0], np.cumsum(case["draws"][:, 1] // 3)])
    tested_t = {int(first[d]) + k: d for d in (1, 4) for k in range(2)}
    want = {first[1]: ("lane", "narrow"), first[1] + 1: ("wave", "narrow"), first[4]: ("wave", "int64"), first[4] + 1: ("lane", "int64")}
    for fan in o["fan_drawn"]:
        if fan[0] in want:
            paths = {tile_x: path_of(fan, tile_x) for tile_x in range(4)}
            assert want[fan[0]] in paths.values(), (fan, paths)
            if want[fan[0]] == ("wave", "narrow"):
                assert paths[0] is not None and paths[1] is not None, "across the tile boundary at x = 64"
            if want[fan[0]] == ("lane", "int64"):
                assert paths[0] == ("lane", "int64") and paths[1] == ("wave", "int64")
    for t, d in tested_t.items():
        f, = [f for f in a["fragments"] if f["t"] == t]
        ok = f["alpha"].astype(np.int64) >= f["cutoff"]
        assert (f["covered"] & ok).any() and (f["covered"] & ~ok).any(), "triangle %d keeps some fragments and loses some" % t
        if want[t] == ("lane", "int64"):
            assert (f["covered"][:, :64] & ok[:, :64]).any() or (f["covered"][:, :64] & ~ok[:, :64]).any(), "it has fragments in tile 0, where its lane walks it"
    assert (own == 0).sum() > 1000 and (own == 3).sum() > 100, "the opaque draws win where nothing tested is in front"
    assert (cutoffs == 0).sum() == 2 and not np.array_equal(a["depth"], o["depth"])


def _check_clipped(runs):
    (case, tex, cutoffs, a, o), = runs
    clip = ref.transform4(case["transforms"][0, 16:32], case["positions"])
    assert (clip[:, 3] <= 0).any(), "the floor reaches behind the camera"
    t_of_winners = (a["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    checked = 0
    for t in sorted({f[0] for f in o["fan_drawn"]}):
        fans = [f for f in o["fan_drawn"] if f[0] == t]
        vi = case["indices"][3 * t:3 * t + 3]
        if len(fans) < 2 or not (clip[vi, 3] <= 0).any():
            continue
        poly, was_clipped = ref.clip_triangle(clip[vi])
        X, Y, _, ok = ref.project(np.stack(poly), case["width"], case["height"])
        assert was_clipped and ok.all()
        jj, ii = np.nonzero((a["keys"] != 0) & (t_of_winners == t))
        edge = (int(X[2]) - int(X[0])) * (256 * jj + 128 - int(Y[0])) - (int(Y[2]) - int(Y[0])) * (256 * ii + 128 - int(X[0]))  # the fan edge poly[0] -> poly[2]
        assert (edge > 0).sum() > 20 and (edge < 0).sum() > 20, "winner pixels on both sides of a fan edge"
        f, = [f for f in a["fragments"] if f["t"] == t]
        assert (f["covered"] & (f["alpha"] < 128)).sum() > 50, "and discarded fragments"
        checked += 1
    assert checked >= 1, "a tested triangle with a vertex at w <= 0, fanned into >= 2 sub-triangles"


def _check_mip_threshold(runs):
    assert [tex["mip_bias"] for _, tex, _, _, _ in runs] == list(MIP_BIASES)
    texels = runs[0][1]["texels"]
    assert set(np.unique(texels[:256] >> np.uint32(24)).tolist()) == {0, 255} and (texels[256:] >> np.uint32(24) == 128).all(), "the chain averages to the cutoff"
    kept_sets, at, below = [], 0, 0
    for case, tex, cutoffs, a, o in runs:
        assert (cutoffs == 128).all()
        kept_sets.append(a["keys"] != 0)
        for f in a["fragments"]:
            at += int((f["covered"] & (f["alpha"] == 128)).sum())
            below += int((f["covered"] & (f["alpha"] == 127)).sum())
            assert (a["keys"][f["covered"] & (f["alpha"] == 128)] != 0).all() and (a["keys"][f["covered"] & (f["alpha"] == 127)] == 0).all()
    assert at > 100 and below > 0, "fragments with a == c (kept: %d) and a == c - 1 (discarded: %d)" % (at, below)
    assert not np.array_equal(kept_sets[0], kept_sets[1]) and not np.array_equal(kept_sets[1], kept_sets[2])


def _check_cutoff_values(runs):
    (case, tex, cutoffs, a, o), = runs
    own, untested = aref.winner_draw(case, a["keys"]), aref.winner_draw(case, o["keys"])
    alpha = o["albedo"] >> np.uint32(24)  # untested, every draw wins its whole cell: the alpha each fragment has
    assert cutoffs.tolist() == [0, 1, 128, 255, 300, 128, 128, 128, 0x60] and all((untested == d).sum() == 14 * 25 for d in range(9))
    for d, c in enumerate(CUTOFF_WORDS):
        cell = untested == d
        want = alpha[cell] >= min(c, 256)
        assert np.array_equal(own[cell] == d, want) and (own[cell][~want] == -1).all()
        if c in (1, 128, 255):
            assert want.any() and (~want).any(), "cutoff %d keeps some and discards some" % c
        assert (alpha[cell] == 255).any() and (alpha[cell] == 0).any() and (alpha[cell] == 127).any() and (alpha[cell] == 128).any()
    assert (own[untested == 0] == 0).all() and (own[untested == 4] == -1).all(), "cutoff 0 keeps all, a word above 255 none - not what 255 does"
    assert (own[untested == 3] == 3).any()
    assert (own[untested == 5] == -1).all() and (own[untested == 6] == 6).all() and (own[untested == 7] == 7).all(), "constant alpha below, at, above"
    assert tref.usable(tex, 1) is None and (own[untested == 8] == 8).all() and (a["albedo"][untested == 8] >> 24 == 0x60).all(), "an unusable texture: the constant word"


CASE_CHECKS = {name: globals()["_check_" + name] for name in CASES}


def check_case_is_what_it_is_for(name):
    CASE_CHECKS[name](reference(name))
