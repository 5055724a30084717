"""Inputs of the crowded-tile tests of the alpha-tested "depthPrepassRaster.comp" (tests/test_prepass_crowd.py, tests/test_prepass_crowd_cpu.py): what the
alpha-tested scan does depends on how many records meet in one tile, and the cases of tests/prepass_alpha_cases.py put at most 16 tested triangles into one.
Every case here is 64 x 64, one tile: every drawn record touches it whatever order the set-up blocks append in. Each has a check, on the reference alone
(tests/prepass_alpha_reference.py), that it reaches what it is named for.

Triangles are made as prepass_raster_cases' crowded_large makes them: a seeded default_rng, corners on the quarter-pixel grid, a random depth per vertex in
0.1 .. 0.9, legs of 9 to 12 pixels (the stamp path) or of 2 to 3.5 pixels (the lane path). A triangle is of one of four kinds by its draw's cutoff word: 0
(opaque), 128 and 200 (tested), 300 (discard-all). The albedo is a 16 x 16 texture with a 0 / 255 checker alpha in cells of two texels under the UVs
(x / 16, y / 16): a texel per pixel, level 0, about half of the tested fragments pass. The draws with cutoff 200 have a second checker, cells of one texel in the
other phase: the UVs are the screen's, so with one texture a candidate sampled with another record's data would still get its own alpha.
  one_wave             250 triangles, one set-up block: the records are in submission order and only wave 0 works, so the kernel's schedule is deterministic and
                       `queue_model` can follow it. A draw per run of equal kinds, so that the kinds interleave in the order of t: four steps of 64 records,
                       each with pushes that carry a remainder down the queue and a flush, one with all six of {opaque, tested, discard-all} x {small, large}
  four_waves           1200 triangles: every wave scans a full window of 256 rectangles with 256 hits (four steps) and wave 0 a second one. A tested triangle
                       with a 64 x 4 box and a span of 35008 (the int64 branch on the stamp path), and as the last 100 triangles bit-equal copies of 100 earlier
                       ones, tested and opaque, in draws of their own with the same cutoff: ties at bit-equal depth across waves and windows, the later t wins
  formats_and_normals  one_wave's geometry with two BC3 albedos (alpha blocks of 0 and 255), a BC5 normal map and an RGBA8 texture in one store, random vertex
                       normals and the tangents of prepass_bc_cases' normal_bc5: four runs with alphaTest 1 - the decoded RGBA8 store and the formatted store, each without and with
                       normal maps, the four alpha-tested instantiations of the tile kernel - that all must give the decoded store's images
`reference(name)` is a dict: case, tex (all RGBA8), cutoffs, a (the alpha reference's result), o (the textured reference without the test, with the raster
reference's diagnostics); formats_and_normals adds store (the formatted one), nm (the normal inputs) and sn (the shading normal).
"""
import numpy as np

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import prepass_bc_cases as bc
import prepass_bc_reference as bref
import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
import test_prepass_raster as tpr

F32 = np.float32
NONE = tref.NONE
SIZE = 64
OPAQUE, TESTED, TESTED_OTHER, DISCARD = range(4)
CUTOFF_OF_KIND = (0, ac.REFERENCE_CUTOFF, 200, 300)
KIND_NAMES = ("opaque", "tested", "tested", "discard")
SIX_KINDS = {(k, s) for k in ("opaque", "tested", "discard") for s in ("small", "large")}
HIGH_WORD = np.uint64(0xFFFFFFFF00000000)


def triangle(rng, small):
    """a right triangle as crowded_large's: legs of 2 to 3.5 pixels (small) or 9 to 12, at a random place, a random depth per vertex"""
    leg = np.rint(rng.uniform((2.0, 2.0), (3.5, 3.5)) * 4) / 4 if small else np.rint(rng.uniform((9.0, 9.0), (12.0, 12.0)) * 4) / 4
    x, y = np.rint(rng.uniform((-2.0, -2.0), (54.0, 54.0)) * 4) / 4
    z = rng.uniform(0.1, 0.9, 3)
    return [(x, y, z[0]), (x + leg[0], y, z[1]), (x + leg[0], y + leg[1], z[2])]


def grouped(triangles, kinds):
    """one draw per run of equal kinds, in the order given -> (groups for pixel_case, the kind of each draw)"""
    groups, draw_kinds = [], []
    for tri, kind in zip(triangles, kinds):
        if not groups or draw_kinds[-1] != kind:
            groups.append([])
            draw_kinds.append(kind)
        groups[-1].append(tri)
    return groups, draw_kinds


def cutoff_words(draw_kinds):
    return np.asarray([CUTOFF_OF_KIND[kind] for kind in draw_kinds], np.uint32)


ALBEDO_OF_KIND = (0, 0, 1, 0)  # the draws with cutoff 200 have the second checker: which record a candidate is sampled with shows in its alpha


def checker_textures():
    """cells of two texels, and cells of one texel in the other phase"""
    full = lambda level0: (tc.chain(level0, 16, 16), 16, 16, tref.full_mip_count(16, 16))
    return [full(ac.checker(16, 16, 2, 81)), full(ac.checker(16, 16, 1, 86, phase=1))]


def checker_materials(draw_kinds):
    return [(ALBEDO_OF_KIND[kind], NONE) for kind in draw_kinds]


def screen_uvs(case):
    return tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))


ONE_WAVE_TRIANGLES = 250
ONE_WAVE_SEED = 0x43524F58
# the share of small triangles per step of 64: the second step holds enough tested small records that the lane path alone fills the queue past 64
ONE_WAVE_SMALL_SHARE = (0.25, 0.9, 0.25, 0.4)
ONE_WAVE_KIND_SHARE = (0.36, 0.3, 0.2, 0.14)


def one_wave_geometry():
    """-> (triangles, kinds): the kinds and sizes drawn per triangle, so that they interleave in submission order"""
    rng = np.random.default_rng(ONE_WAVE_SEED)
    triangles, kinds = [], []
    for k in range(ONE_WAVE_TRIANGLES):
        kinds.append(int(rng.choice(4, p=ONE_WAVE_KIND_SHARE)))
        triangles.append(triangle(rng, rng.random() < ONE_WAVE_SMALL_SHARE[k // 64]))
    return triangles, kinds


def _one_wave():
    groups, draw_kinds = grouped(*one_wave_geometry())
    case = pc.pixel_case(groups, SIZE, SIZE)
    case, tex = tc.textured(case, screen_uvs(case), checker_materials(draw_kinds), checker_textures())
    return dict(case=case, tex=tex, cutoffs=cutoff_words(draw_kinds))


FOUR_WAVES_ORIGINALS, FOUR_WAVES_COPIES = 1100, 100
FOUR_WAVES_SEED = 0x43524F59
FOUR_WAVES_KIND_SHARE = (0.6, 0.2, 0.12, 0.08)
FOUR_WAVES_SMALL_SHARE = 0.5


def _four_waves():
    """draws 0 - 3: the four kinds (the long triangle is the first of draw 2); draw 4: copies of 50 triangles of draw 1, cutoff 128; draw 5: copies of 50 of draw 0"""
    rng = np.random.default_rng(FOUR_WAVES_SEED)
    kinds = rng.choice(4, FOUR_WAVES_ORIGINALS - 1, p=FOUR_WAVES_KIND_SHARE)
    by_kind = [[triangle(rng, rng.random() < FOUR_WAVES_SMALL_SHARE) for _ in range(int((kinds == kind).sum()))] for kind in range(4)]
    by_kind[TESTED_OTHER].insert(0, [tuple(v) for v in tpr.LANE_INT64_ROW])
    # the copies: of large triangles, which own more pixels
    large = lambda tris: [k for k, tri in enumerate(tris) if tri[1][0] - tri[0][0] >= 9.0]
    tested_copies = [by_kind[TESTED][k] for k in rng.permutation(large(by_kind[TESTED]))[:FOUR_WAVES_COPIES // 2]]
    opaque_copies = [by_kind[OPAQUE][k] for k in rng.permutation(large(by_kind[OPAQUE]))[:FOUR_WAVES_COPIES // 2]]
    groups = by_kind + [tested_copies, opaque_copies]
    draw_kinds = [OPAQUE, TESTED, TESTED_OTHER, DISCARD, TESTED, OPAQUE]
    case = pc.pixel_case(groups, SIZE, SIZE)
    case, tex = tc.textured(case, screen_uvs(case), checker_materials(draw_kinds), checker_textures())
    return dict(case=case, tex=tex, cutoffs=cutoff_words(draw_kinds))


ALBEDO_BC3, NORMAL_BC5, SECOND_RGBA8, OTHER_ALBEDO_BC3 = 0, 1, 2, 3
BC_ALBEDO_OF_KIND = (ALBEDO_BC3, ALBEDO_BC3, OTHER_ALBEDO_BC3, ALBEDO_BC3)
NORMAL_MAP_OF_KIND = (SECOND_RGBA8, NORMAL_BC5, NORMAL_BC5, NONE)
NORMALS_SEED = 0x43524F5A


def _formats_and_normals():
    """one_wave's triangles and draws; albedo a BC3 (another one for the draws with cutoff 200), specular the RGBA8 texture in every other draw and the draw's
    constant word in the rest; the tested draws' normal map is the BC5, the opaque draws' the RGBA8 texture. A random vertex normal per vertex, within 45 degrees of
    +z: which triangle wins a pixel shows in `normal` and, with the tangent frame, in `shadingNormal`"""
    groups, draw_kinds = grouped(*one_wave_geometry())
    case = pc.pixel_case(groups, SIZE, SIZE)
    rng = np.random.default_rng(NORMALS_SEED)
    normals = np.concatenate([rng.uniform(-0.7, 0.7, (case["positions"].shape[0], 2)), np.ones((case["positions"].shape[0], 1))], axis=1)
    case = nc.with_normals(case, (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32))
    second = (tc.chain(tc.pattern(8, 8, 83), 8, 8), 8, 8, tref.full_mip_count(8, 8), bc.RGBA8)
    textures = [bc.full(bc.BC3, 16, 16, 82, alpha_binary=True), bc.full(bc.BC5, 8, 8, 84), second, bc.full(bc.BC3, 16, 16, 85, alpha_binary=True)]
    materials = [(BC_ALBEDO_OF_KIND[kind], SECOND_RGBA8 if d % 2 == 0 else NONE) for d, kind in enumerate(draw_kinds)]
    store = bc.store(case, screen_uvs(case), materials, textures)
    nm = nc.normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), [NORMAL_MAP_OF_KIND[kind] for kind in draw_kinds], nref.DECODE_REFERENCE)
    return dict(case=case, tex=bref.decode_store(store), cutoffs=cutoff_words(draw_kinds), store=store, nm=nm)


CASES = dict(one_wave=_one_wave, four_waves=_four_waves, formats_and_normals=_formats_and_normals)

_reference_cache = {}


def reference(name):
    """the dict the module docstring describes, computed once per process; callers must not modify it"""
    if name not in _reference_cache:
        r = CASES[name]()
        opaque = pc.rasterise(r["case"], diagnostics=True)
        s = tref.sample(r["case"], r["tex"], opaque["keys"])
        r["o"] = dict(opaque, albedo=s["albedo"], specular=s["specular"])
        r["a"] = nc.base_images(r["case"], r["tex"], r["cutoffs"])
        if "nm" in r:
            r["sn"] = nref.shade(r["case"], r["tex"], r["nm"], r["a"]["keys"], r["a"]["normal"])
        _reference_cache[name] = r
    return _reference_cache[name]


def first_triangles(case):
    """the number of the first triangle of every draw, and behind them the triangle count"""
    return np.concatenate([[0], np.cumsum(np.asarray(case["draws"], np.uint32).reshape(-1, 6)[:, 1].astype(np.int64) // 3)])


def triangle_alone(case, t):
    """the fragment keys of triangle t rasterised alone by the raster reference, carrying t: 0 where it has no fragment"""
    first = first_triangles(case)
    d = int(np.searchsorted(first, t, side="right")) - 1
    row = np.asarray(case["draws"], np.uint32).reshape(-1, 6)[d].astype(np.int64)
    row[0], row[1] = row[0] + 3 * (t - int(first[d])), 3
    keys = pc.rasterise(dict(case, draws=row.astype(np.uint32).reshape(1, 6)))["keys"]
    return np.where(keys != 0, (keys & HIGH_WORD) | np.uint64(t), np.uint64(0))


def record_kind(case, tex, cutoffs, d):
    """what the scan makes of a record of draw d: opaque, tested (the sample decides) or discard; a tested draw without a usable albedo texture is decided by
    its constant word's alpha"""
    c = int(aref.cutoff_codes(cutoffs)[d])
    if c == 0 or c == aref.DISCARD_ALL:
        return "opaque" if c == 0 else "discard"
    if tref.usable(tex, int(tex["materials"][d, 0])) is None:
        return "opaque" if (int(case["draws"][d, 4]) >> 24) >= c else "discard"
    return "tested"


def queue_model(case, reference):
    """A scalar model of the SCHEDULE of the alpha-tested scan (csrc/kernels/depth_prepass_raster.hip AlphaWalk / AlphaScan under device/raster_tile_walk.h
    rasteriseTile) for an execution whose records are in submission order within one window of 256 rectangles: only wave 0 of each tile works and what it does
    is determined. case: (prepass case, texture inputs, cutoffs); reference: (the alpha reference's result, the raster reference's with diagnostics).

    Per tile the hits are taken in steps of 64 records, and per step: the 16 iterations of the tested small records' lane path, in step over the lanes, each a
    push; the opaque small records; the large records in lane order - an opaque one is written, a discard-all one skipped, a tested one stamped 8 x 8 from its
    box's first pixel inside the tile, a push per stamp -; the flush. A push that takes `pending` to 64 or more samples the first 64 candidates and moves the rest
    down. A candidate is a covered fragment whose key is above its cell when it is queued, and it is looked at again when it is sampled (the early out).

    Coverage, depth and alpha per (t, pixel) are the references': `fragments` of the alpha reference and the raster reference's keys of every triangle alone. The
    model computes no coverage and no alpha. It serves the conditions of the cases - which paths of the scan an input reaches - and never an expected image.
    -> dict(keys, steps (per step the set of (kind, size) present), carries (pushes that sampled and left a remainder), lane_carries (those of the lane path),
    max_pending, flushes (with pending > 0), dropped_queued / dropped_sampled (candidates the early out dropped before the queue / before the sample))"""
    (case, tex, cutoffs), (a, o) = case, reference
    width, height = case["width"], case["height"]
    records = o["fan_drawn"]
    numbers = [r[0] for r in records]
    assert len(records) <= 256 and numbers == sorted(set(numbers)), "one set-up block, one record per triangle: the records are in submission order"
    first = first_triangles(case)
    draw_of = lambda t: int(np.searchsorted(first, t, side="right")) - 1
    kind_of_draw = [record_kind(case, tex, cutoffs, d) for d in range(case["draws"].shape[0])]
    alone = {t: triangle_alone(case, t) for t in numbers}
    fragments = {f["t"]: f for f in a["fragments"]}
    keys = np.zeros((height, width), np.uint64)
    out = dict(steps=[], carries=0, lane_carries=0, max_pending=0, flushes=0, dropped_queued=0, dropped_sampled=0)
    queue = []

    def sample(batch):
        seen = [keys[py, px] for px, py, t in batch]  # the lanes read their cells together, before any of them writes
        for (px, py, t), cell in zip(batch, seen):
            if not alone[t][py, px] > cell:
                out["dropped_sampled"] += 1
            elif int(fragments[t]["alpha"][py, px]) >= fragments[t]["cutoff"]:
                keys[py, px] = max(keys[py, px], alone[t][py, px])

    def push(candidates, lane_path):
        if not candidates:
            return
        queue.extend(candidates)
        out["max_pending"] = max(out["max_pending"], len(queue))
        if len(queue) >= 64:
            sample(queue[:64])
            del queue[:64]
            if queue:
                out["carries"] += 1
                out["lane_carries"] += int(lane_path)

    def candidate(t, px, py, into):
        if alone[t][py, px] != 0:
            if alone[t][py, px] > keys[py, px]:
                into.append((px, py, t))
            else:
                out["dropped_queued"] += 1

    for ty in range((height + 63) // 64):
        for tx in range((width + 63) // 64):
            wx0, wy0, wx1, wy1 = 64 * tx, 64 * ty, min(64 * tx + 63, width - 1), min(64 * ty + 63, height - 1)
            hits = []
            for t, _, (ix0, iy0, ix1, iy1), _ in records:
                bx0, by0, bx1, by1 = max(ix0, wx0), max(iy0, wy0), min(ix1, wx1), min(iy1, wy1)
                if bx0 <= bx1 and by0 <= by1:
                    hits.append((t, kind_of_draw[draw_of(t)], bx1 - bx0 < 4 and by1 - by0 < 4, (bx0, by0, bx1, by1)))
            for k in range(0, len(hits), 64):
                lanes = hits[k:k + 64]
                out["steps"].append({(kind, "small" if small else "large") for _, kind, small, _ in lanes})
                tested_small = [(t, box) for t, kind, small, box in lanes if small and kind == "tested"]
                if tested_small:
                    for i in range(16):
                        candidates = []
                        for t, (bx0, by0, bx1, by1) in tested_small:
                            px, py = bx0 + (i & 3), by0 + (i >> 2)
                            if px <= bx1 and py <= by1:
                                candidate(t, px, py, candidates)
                        push(candidates, True)
                for t, kind, small, (bx0, by0, bx1, by1) in lanes:
                    if small and kind == "opaque":
                        box = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
                        keys[box] = np.maximum(keys[box], alone[t][box])
                for t, kind, small, (bx0, by0, bx1, by1) in lanes:
                    if small or kind == "discard":
                        continue
                    if kind == "opaque":
                        box = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
                        keys[box] = np.maximum(keys[box], alone[t][box])
                        continue
                    for sy in range(by0, by1 + 1, 8):
                        for sx in range(bx0, bx1 + 1, 8):
                            candidates = []
                            for lane in range(64):
                                px, py = sx + (lane & 7), sy + (lane >> 3)
                                if px <= bx1 and py <= by1:
                                    candidate(t, px, py, candidates)
                            push(candidates, False)
                if queue:
                    out["flushes"] += 1
                    sample(list(queue))
                    del queue[:]
    out["keys"] = keys
    return out


def fragment_sets(a, draws=None):
    """over the fragments of sampled triangles (of `draws`; not those of discard-all draws): how many pass and how many fail, per pixel"""
    shape = a["keys"].shape
    passed, failed = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    for f in a["fragments"]:
        if f["cutoff"] != aref.DISCARD_ALL and (draws is None or f["draw"] in draws):
            ok = f["alpha"].astype(np.int64) >= f["cutoff"]
            passed += f["covered"] & ok
            failed += f["covered"] & ~ok
    return passed, failed


def winners_by_kind(case, cutoffs, keys):
    """per pixel the kind name of the winner's draw ("sky" without one)"""
    own = aref.winner_draw(case, keys)
    names = np.array([KIND_NAMES[CUTOFF_OF_KIND.index(int(c))] for c in cutoffs] + ["sky"])
    return names[own]


_model_cache = {}


def model_of(name):
    """queue_model of a one-window case, computed once"""
    if name not in _model_cache:
        r = reference(name)
        _model_cache[name] = queue_model((r["case"], r["tex"], r["cutoffs"]), (r["a"], r["o"]))
    return _model_cache[name]


def _check_crowd_of_250(r, m):
    """what one_wave and formats_and_normals share: the schedule the 250 records take"""
    case, a, o = r["case"], r["a"], r["o"]
    assert case["width"] == case["height"] == SIZE and tpr.counters(o) == (ONE_WAVE_TRIANGLES, 0, ONE_WAVE_TRIANGLES, 0) and tpr.counters(a) == tpr.counters(o)
    assert [f[0] for f in o["fan_drawn"]] == list(range(ONE_WAVE_TRIANGLES)), "one set-up block: the records are in submission order, within wave 0's first window"
    assert np.array_equal(m["keys"], a["keys"]), "the model takes every fragment the reference takes: it is faithful"
    assert len(m["steps"]) >= 3
    assert any(step == SIX_KINDS for step in m["steps"]), "a step with opaque, tested and discard-all records of both sizes: %r" % (m["steps"],)
    assert all(("tested", "small") in step and ("tested", "large") in step and ("opaque", "large") in step for step in m["steps"]), "kinds mix inside every step"
    assert m["carries"] >= 10 and m["lane_carries"] >= 1 and 64 < m["max_pending"] < 128, "carries %d, of the lane path %d, largest pending %d" % (m["carries"], m["lane_carries"], m["max_pending"])
    assert m["flushes"] == len(m["steps"]), "every step flushes something"
    assert m["dropped_queued"] >= 1 and m["dropped_sampled"] >= 1, "the early out drops candidates at both places"
    kinds = winners_by_kind(case, r["cutoffs"], a["keys"])
    won = {kind: int((kinds == kind).sum()) for kind in ("tested", "opaque", "discard", "sky")}
    assert won["tested"] >= 500 and won["opaque"] > 0 and won["discard"] == 0 and won["sky"] > 0, won
    passed, failed = fragment_sets(a)
    assert 0.4 < passed.sum() / (passed.sum() + failed.sum()) < 0.6, "about half of the tested fragments pass: %d of %d" % (passed.sum(), passed.sum() + failed.sum())
    assert not np.array_equal(a["depth"], o["depth"]), "the untested image is another one"
    assert len(set(int(c) for c in r["cutoffs"])) == 4 and r["cutoffs"].size > 100, "all four cutoff words, in many small draws"


def _check_one_wave(r):
    _check_crowd_of_250(r, model_of("one_wave"))


def _check_four_waves(r):
    case, cutoffs, a, o = r["case"], r["cutoffs"], r["a"], r["o"]
    first = first_triangles(case)
    assert case["width"] == case["height"] == SIZE and case["draws"].shape[0] == 6 and cutoffs.tolist() == [0, 128, 200, 300, 128, 0]
    assert o["drawn"] > 1024 and 1100 <= o["drawn"] <= 1300 and tpr.counters(o) == (int(first[-1]), 0, int(first[-1]), 0) and tpr.counters(a) == tpr.counters(o), \
        "more than 1024 rectangles: every wave scans a full window with 256 hits, four steps, and wave 0 a second window; the counters are the untested case's"
    assert len(o["fan_drawn"]) == o["drawn"] and all(0 <= x0 <= x1 < SIZE and 0 <= y0 <= y1 < SIZE for _, _, (x0, y0, x1, y1), _ in o["fan_drawn"]), "every record meets the tile"
    tested = int(first[3] - first[1] + first[5] - first[4])
    assert 0.25 < tested / o["drawn"] < 0.4, "about a third is tested: %d of %d" % (tested, o["drawn"])
    # the long triangle
    long_t = int(first[TESTED_OTHER])
    (_, _, box, spans), = [f for f in o["fan_drawn"] if f[0] == long_t]
    assert box == (0, 10, 63, 13) and max(spans) == 35008 >= tpr.NARROW_SPAN, "a 64 x 4 box: the stamp path; a span of 35008: 64-bit edge functions"
    f, = [f for f in a["fragments"] if f["t"] == long_t]
    ok = f["alpha"].astype(np.int64) >= f["cutoff"]
    assert (f["covered"] & ok).sum() > 10 and (f["covered"] & ~ok).sum() > 10, "it keeps some fragments and loses some"
    # the copies
    positions, uvs = case["positions"].reshape(-1, 3, 3), r["tex"]["uvs"].reshape(-1, 3, 2)
    by_bytes = {}
    for t in range(int(first[4])):
        by_bytes.setdefault(positions[t].tobytes() + uvs[t].tobytes(), t)
    own_t = np.where(a["keys"] != 0, (a["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    fragments = {f["t"]: f for f in a["fragments"]}
    won_by_copy = {4: 0, 5: 0}
    for d, original_draw in ((4, TESTED), (5, OPAQUE)):
        assert int(first[d + 1] - first[d]) == FOUR_WAVES_COPIES // 2
        for t in range(int(first[d]), int(first[d + 1])):
            original = by_bytes[positions[t].tobytes() + uvs[t].tobytes()]
            assert first[original_draw] <= original < first[original_draw + 1] and cutoffs[d] == cutoffs[original_draw], "bit-equal vertices and UVs, the same cutoff"
            if d == 4:
                f, g = fragments[t], fragments[original]
                assert np.array_equal(f["covered"], g["covered"]) and np.array_equal(f["alpha"][f["covered"]], g["alpha"][g["covered"]])
                passes = f["covered"] & (f["alpha"].astype(np.int64) >= f["cutoff"])
            else:
                passes = triangle_alone(case, t) != 0
                assert np.array_equal(passes, triangle_alone(case, original) != 0)
            assert not (own_t[passes] == original).any(), "where the original passes the copy passes at bit-equal depth, and the later t wins"
            won_by_copy[d] += int((own_t[passes] == t).sum())
    assert won_by_copy[4] >= 30 and won_by_copy[5] >= 30, "pixels won by a tested copy and by an opaque copy: %r" % (won_by_copy,)
    passed, failed = fragment_sets(a)
    assert (passed + failed).max() >= 8, "tested fragments %d deep" % (passed + failed).max()
    assert 0.4 < passed.sum() / (passed.sum() + failed.sum()) < 0.6
    assert np.unique(own_t[own_t >= 0]).size >= 300, "winners of %d triangles" % np.unique(own_t[own_t >= 0]).size
    kinds = winners_by_kind(case, cutoffs, a["keys"])
    assert (kinds == "tested").sum() >= 500 and (kinds == "opaque").sum() >= 500 and not (kinds == "discard").any()
    assert not np.array_equal(a["depth"], o["depth"])


def _check_formats_and_normals(r):
    _check_crowd_of_250(r, model_of("formats_and_normals"))
    case, store, nm, a, sn = r["case"], r["store"], r["nm"], r["a"], r["sn"]
    plain = reference("one_wave")["case"]
    assert np.array_equal(case["positions"], plain["positions"]) and np.array_equal(case["draws"], plain["draws"]), "one_wave's geometry"
    assert store["formats"].tolist() == [bc.BC3, bc.BC5, bc.RGBA8, bc.BC3] and "formats" not in r["tex"]
    assert set(store["materials"][:, 0].tolist()) == {ALBEDO_BC3, OTHER_ALBEDO_BC3} and set(store["materials"][:, 1].tolist()) == {SECOND_RGBA8, NONE}
    for row in (ALBEDO_BC3, OTHER_ALBEDO_BC3):
        offset, width, height, _ = (int(v) for v in r["tex"]["textures"][row])
        assert set(np.unique(r["tex"]["texels"][offset:offset + width * height] >> np.uint32(24)).tolist()) == {0, 255}, "the BC3s' alpha blocks hold 0 and 255"
    assert set(nm["normal_materials"].tolist()) == {NORMAL_BC5, SECOND_RGBA8, NONE}
    kinds = winners_by_kind(case, r["cutoffs"], a["keys"])
    differing = int(((sn != a["normal"]) & (kinds == "tested")).sum())
    assert differing >= 200, "the shading normal differs from the vertex normal on %d winner pixels of tested draws" % differing
    assert np.array_equal(sn[kinds == "sky"], a["normal"][kinds == "sky"])


CASE_CHECKS = {name: globals()["_check_" + name] for name in CASES}


def check_case_is_what_it_is_for(name):
    CASE_CHECKS[name](reference(name))
