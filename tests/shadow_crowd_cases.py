"""Input of the crowded-tile tests of the cutout casters of "sunShadowRaster.comp" (tests/test_prepass_crowd.py, tests/test_prepass_crowd_cpu.py): the cases of
tests/shadow_alpha_cases.py put a handful of records into a tile; this one puts 650 into the one tile of a 64 x 64 map, from three set-up blocks that append
their 128-byte records by ballot in whatever order they arrive, so that three waves of the tile kernel work and every window has more than one step of 64 hits.

Triangles as tests/prepass_crowd_cases.py makes them (the shadow pass draws them as they are written): legs of 9 to 12 pixels or of 2 to 3.5, a random depth
per vertex. Twelve draws cycle through opaque casters and casters with the cutoffs 128, 200 and 300 (discard-all), on the 16 x 16 checker of
tests/shadow_alpha_cases.py at a texel per pixel (cutoff 200: a checker of its own, cells of one texel in the other phase); two more draws hold bit-equal copies of 25 tested and 25 opaque triangles with their draws' cutoffs.
`reference()` is (case, tex, cascade, tested result, untested result).
"""
import numpy as np

import prepass_crowd_cases as cc
import shadow_alpha_cases as sac
import shadow_alpha_reference as aref
import shadow_raster_cases as sc

RES = 64
CASCADE = 2
SEED = 0x53484358
ORIGINALS, COPIES = 600, 50
CYCLE = ((sac.NONE, 0), (0, sac.REFERENCE_CUTOFF), (1, 200), (sac.NONE, 0), (0, 300), (0, sac.REFERENCE_CUTOFF))  # (albedoTexture, cutoff word) of draws k, k + 6
SMALL_SHARE = 0.4
UV = sac.texel_ratio(0.0, 0.0, 1.0, 1.0, 16, 16)


def _crowd():
    rng = np.random.default_rng(SEED)
    draws = 2 * len(CYCLE)
    triangles = [[cc.triangle(rng, rng.random() < SMALL_SHARE) for _ in range(ORIGINALS // draws)] for _ in range(draws)]
    parts = [(tris, UV, *CYCLE[d % len(CYCLE)]) for d, tris in enumerate(triangles)]
    large = lambda tris: [tri for tri in tris if tri[1][0] - tri[0][0] >= 9.0]
    parts.append((large(triangles[1])[:COPIES // 2], UV, *CYCLE[1]))
    parts.append((large(triangles[0])[:COPIES // 2], UV, *CYCLE[0]))
    return sac.build(RES, parts, [sac.CHECKER16, sac.full_chain(sac.checker(16, 16, 1, 87, phase=1), 16, 16)]) + (CASCADE,)


_cache = {}


def reference():
    """computed once; callers must not modify it"""
    if "crowd" not in _cache:
        case, tex, cascade = _crowd()
        _cache["crowd"] = (case, tex, cascade, aref.rasterise(case, tex), sc.rasterise(case))
    return _cache["crowd"]


def _subset(case, tex, keep):
    return dict(case, draws=case["draws"][keep]), dict(tex, materials=tex["materials"][keep])


def check_case_is_what_it_is_for():
    case, tex, cascade, a, o = reference()
    triangles = int((case["draws"][:, 1] // 3).sum())
    assert case["res"] == RES and 600 <= triangles <= 700 and triangles > 2 * 256, "one tile, three set-up blocks of 256 triangles"
    assert (a["submitted"], a["drawn"], a["rejects"]) == (o["submitted"], o["drawn"], o["rejects"]) and a["submitted"] == triangles and a["rejects"] == 0, \
        "the counters do not depend on alpha (a small triangle off the map's edge or between texel centres is not drawn)"
    assert a["drawn"] > 512 and a["drawn"] - 512 > 64, "every drawn record touches the one tile: three waves work, and every window of 256 rectangles has more than 64 hits"
    cutoffs = tex["materials"][:, 1]
    assert set(cutoffs.tolist()) == {0, 128, 200, 300} and 0 < a["passed"] < a["tested"] and 0.4 < a["passed"] / a["tested"] < 0.6
    positions = case["positions"].reshape(-1, 3, 3)
    first = np.concatenate([[0], np.cumsum(case["draws"][:, 1] // 3)])
    for copy, original in ((12, 1), (13, 0)):
        assert int(first[copy + 1] - first[copy]) == COPIES // 2 and np.array_equal(tex["materials"][copy], tex["materials"][original])
        theirs = {positions[t].tobytes() + tex["uvs"].reshape(-1, 3, 2)[t].tobytes() for t in range(int(first[original]), int(first[original + 1]))}
        assert all(positions[t].tobytes() + tex["uvs"].reshape(-1, 3, 2)[t].tobytes() in theirs for t in range(int(first[copy]), int(first[copy + 1]))), "bit-equal copies"
    # who owns a texel: the maps of the sampled casters alone and of the opaque casters alone
    sampled = (cutoffs != 0) & (cutoffs <= 255)
    by_sampled = aref.rasterise(*_subset(case, tex, sampled))["map"]
    by_opaque = aref.rasterise(*_subset(case, tex, cutoffs == 0))["map"]
    assert np.array_equal(a["map"], np.maximum(by_sampled, by_opaque))
    assert (by_sampled > by_opaque).sum() >= 300 and (by_opaque > by_sampled).sum() >= 300, "texels owned by tested casters: %d, by opaque ones: %d" % ((by_sampled > by_opaque).sum(), (by_opaque > by_sampled).sum())
    assert (a["map"] != o["map"]).sum() >= 100, "the untested map differs on %d texels" % (a["map"] != o["map"]).sum()
    boxes = [max(tri[:, 0].max() - tri[:, 0].min(), tri[:, 1].max() - tri[:, 1].min()) * RES / 2 for tri in positions]
    assert sum(b < 4 for b in boxes) > 150 and sum(b >= 9 for b in boxes) > 300, "small and large"
