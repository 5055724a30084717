"""Inputs of the tests of block-compressed cutout textures in "sunShadowRaster.comp" (tests/test_shadow_bc.py, tests/test_shadow_bc_cpu.py): named cases on maps of
64 x 64 to 256 x 256 texels, one to twelve triangles per part, each with a check - on the reference alone (tests/shadow_bc_reference.py) - that the case exercises
what it is named for. Blocks are built in numpy: by hand (alpha_block) or with the encoder of tests/texture_build_reference.py.

A case is a list of runs (shadow case, texture inputs, cascade index) as in tests/shadow_alpha_cases.py, the texture inputs with the mixed store of
tests/prepass_bc_reference.py: `texels` words, `textures` rows with word offsets, `formats`.
  sizes           256: BC3 textures of 1 x 1, 2 x 2, 4 x 4, 5 x 3, 8 x 8, 33 x 17 and 64 x 64 with full chains - partial blocks and levels smaller than a block -, each
                  under a magnified and a minified quad
  alpha_modes     128: a hand-made BC3 level of 12 x 4 texels: an eight-value block (a0 > a1), a six-value block (a0 < a1, with its codes 0 and 255) and a block with
                  a0 == a1, every index 0 .. 7 in each, four pixels per texel, under the cutoffs 0, 1, 128 and 255
  mixed_store     128: one store holding RGBA8 (5 x 3, 18 words: the next block needs padding), BC1, BC3, BC5, a second RGBA8 and a second BC3 entry; every entry
                  named by a draw
  bc1_bc5         96: BC1 and BC5 cutouts at the cutoffs 1, 255 and the raw word 256, over an opaque quad
  unusable        96: a BC3 entry whose offset is no multiple of 4 words, an entry with the format code 4 (both opaque, both also at the raw cutoff 300), next to a
                  BC3 entry that is sampled
  short_buffer    64: `texels` cut short inside the last block of a BC3 level; the block reads 0 and its texels fail every cutoff
  draw_counts     64: 1, 63, 64 and 65 draws of one triangle each, alternating between two BC3 textures
  alpha_<name>    the cases of tests/shadow_alpha_cases.py with every texture re-encoded to BC3: the lane, wave and int64 paths, tile corners, the level transition
                  (mip_threshold: L1 != L0 with fw != 0), cutoff values, UVs that wrap across the texture's edge and across block edges, negative UVs, the |u| >=
                  2^20 rule, vertices outside `uvs`, an affine transform
"""
import numpy as np

import prepass_bc_reference as bc
import prepass_texture_reference as tref
import shadow_alpha_cases as ac
import shadow_alpha_reference as aref
import shadow_bc_reference as bref
import shadow_raster_cases as sc
import texture_build_reference as tbr
from shadow_raster_cases import quad

U32 = np.uint32
NONE = aref.NONE
RGBA8, BC1, BC3, BC5 = bc.RGBA8, bc.BC1, bc.BC3, bc.BC5
REFERENCE_CUTOFF = ac.REFERENCE_CUTOFF


def encoded(fmt, chain, width, height, mips):
    """`mips` RGBA8 levels back to back -> a pack_store entry of their blocks"""
    return b"".join(tbr.encode_level(fmt, level) for level in tbr.split_levels(chain, width, height, mips)), width, height, mips, fmt


def noise_alpha(width, height, salt):
    """RGBA8 texels whose alpha takes every kind of value: cells of two texels (one in a texture of at most 5 x 5), each 0, 255 or a hash"""
    y, x = np.mgrid[0:height, 0:width]
    cell = 1 if max(width, height) <= 5 else 2
    h = (((x // cell) * 73 + (y // cell) * 151 + salt) * 2654435761) & 0xFFFFFFFF
    alpha = np.where(h % 3 == 0, 0, np.where(h % 3 == 1, 255, (h >> 8) & 255)).astype(U32)
    return ((h & 0x00FFFFFF).astype(U32) | (alpha << U32(24))).reshape(-1)


def alpha_block(a0, a1, indices):
    """the 8 bytes of an alpha block with endpoints a0, a1 and 16 three-bit indices"""
    bits = sum(int(k) << (3 * i) for i, k in enumerate(indices))
    return bytes([a0, a1] + [(bits >> (8 * j)) & 255 for j in range(6)])


def build(res, parts, entries, texture_count=None, uv_vertices=None):
    """parts: as shadow_alpha_cases.build takes them; entries: pack_store entries [(data, width, height, mips, format)] -> (case, tex)"""
    case, tex = ac.build(res, parts, [], uv_vertices=uv_vertices)
    table, words, formats = bc.pack_store(entries)
    return case, dict(tex, textures=table, texels=words, formats=formats, texture_count=table.shape[0] if texture_count is None else texture_count)


# ---- sizes
SIZES = [(1, 1), (2, 2), (4, 4), (5, 3), (8, 8), (33, 17), (64, 64)]


def _sizes_box(k, minified):
    x0, y0 = 6.0 + 35.0 * k, 8.0 + 40.0 * minified
    return x0, y0, x0 + 30.0, y0 + 30.0


def _sizes():
    entries, parts = [], []
    for k, (w, h) in enumerate(SIZES):
        chain = tref.build_chain(noise_alpha(w, h, 100 + k), w, h)
        entries.append(encoded(BC3, chain, w, h, tref.full_mip_count(w, h)))
        for minified, ratio in enumerate((0.3, 1.7)):  # texels per pixel: level 0, and a blend of levels 0 and 1 where the chain has them
            x0, y0, x1, y1 = _sizes_box(k, minified)
            parts.append((quad(x0, y0, x1, y1, 0.4 + 0.02 * k, 0.45 + 0.02 * k), ac.texel_ratio(x0 - 3.0, y0 - 2.0, ratio, ratio, w, h), k, 100 if (w, h) == (1, 1) else REFERENCE_CUTOFF))
    parts.append((quad(2.0, 100.0, 254.0, 250.0, 0.2, 0.25), ac.NO_UV, NONE, 0))  # an opaque quad in the lower tiles, under nothing
    return [build(256, parts, entries) + (1,)]


# ---- alpha_modes
MODE_CUTOFFS = (0, 1, 128, 255)
MODE_BLOCKS = [(240, 16), (16, 240), (77, 77)]  # eight values; six values with 0 and 255; a0 == a1 (the six-value rule: indices 6 and 7 are 0 and 255)


def _modes_box(k):
    return 4.0, 4.0 + 30.0 * k, 52.0, 20.0 + 30.0 * k


def _alpha_modes():
    indices = [0, 1, 2, 3, 4, 5, 7, 7, 6, 6, 7, 7, 3, 2, 1, 0]  # every index; a 2 x 2 group of 7s, so that the six-value block's 255 is reached between texel centres
    colour = bytes([0x1F, 0xF8, 0xE0, 0x07, 0x1B, 0xE4, 0x4E, 0xB1])
    data = b"".join(alpha_block(a0, a1, indices) + colour for a0, a1 in MODE_BLOCKS)
    parts = []
    for k, c in enumerate(MODE_CUTOFFS):
        x0, y0, x1, y1 = _modes_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.5, 0.55), ac.texel_ratio(x0, y0, 0.25, 0.25, 12, 4), 0, c))  # four pixels per texel: the quad shows the level once
    return [build(128, parts, [(data, 12, 4, 1, BC3)]) + (0,)]


# ---- mixed_store
def _mixed_box(k):
    return 4.0 + 40.0 * (k % 3), 4.0 + 44.0 * (k // 3), 4.0 + 40.0 * (k % 3) + 34.0, 4.0 + 44.0 * (k // 3) + 36.0


def _mixed_entries():
    def full(w, h, salt):
        return tref.build_chain(noise_alpha(w, h, salt), w, h), w, h, tref.full_mip_count(w, h)
    return [full(5, 3, 1) + (RGBA8,), encoded(BC1, *full(8, 8, 2)), encoded(BC3, *full(16, 16, 3)), encoded(BC5, *full(8, 8, 4)), full(3, 3, 5) + (RGBA8,),
            encoded(BC3, *full(9, 6, 6))]


def _mixed_store():
    entries = _mixed_entries()
    parts = []
    for k, (_, w, h, _, _) in enumerate(entries):
        x0, y0, x1, y1 = _mixed_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.4 + 0.05 * k, 0.42 + 0.05 * k), ac.texel_ratio(x0 + 5.0, y0 + 1.0, 0.45, 0.6, w, h), k, REFERENCE_CUTOFF))
    return [build(128, parts, entries) + (2,)]


# ---- bc1_bc5
CONSTANT_DRAWS = [(0, 1), (0, 255), (0, 256), (1, 1), (1, 255), (1, 256)]  # (entry: 0 = BC1, 1 = BC5; cutoff word); entry 2 is a BC3 one, sampled


def _constant_box(k):
    return 4.0 + 14.0 * k, 10.0, 16.0 + 14.0 * k, 50.0


def _bc1_bc5():
    chain = tref.build_chain(noise_alpha(8, 8, 9), 8, 8), 8, 8, 4
    parts = [(quad(2.0, 30.0, 94.0, 90.0, 0.2, 0.2), ac.NO_UV, NONE, 0)]
    for k, (entry, word) in enumerate(CONSTANT_DRAWS):
        x0, y0, x1, y1 = _constant_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.6, 0.6), ac.texel_ratio(x0, y0, 0.5, 0.5, 8, 8), entry, word))
    parts.append((quad(4.0, 60.0, 60.0, 88.0, 0.7, 0.7), ac.texel_ratio(0.0, 0.0, 0.5, 0.5, 8, 8), 2, REFERENCE_CUTOFF))
    return [build(96, parts, [encoded(BC1, *chain), encoded(BC5, *chain), encoded(BC3, *chain)]) + (0,)]


# ---- unusable
UNUSABLE_DRAWS = [(0, 128), (0, 300), (1, 128), (1, 300), (2, 128)]  # entry 0: misaligned BC3; 1: format code 4; 2: a BC3 entry as it should be


def _unusable_box(k):
    return 4.0 + 18.0 * k, 6.0, 20.0 + 18.0 * k, 60.0


def _unusable():
    chain = tref.build_chain(ac.checker(8, 8, 2, 51), 8, 8), 8, 8, 4
    parts = []
    for k, (entry, word) in enumerate(UNUSABLE_DRAWS):
        x0, y0, x1, y1 = _unusable_box(k)
        parts.append((quad(x0, y0, x1, y1, 0.5, 0.5), ac.texel_ratio(x0, y0, 0.5, 0.5, 8, 8), entry, word))
    # the store by hand: one word, entry 0 behind it (offset 1: no multiple of 4), entry 1 (its format code is 4), three words of padding, entry 2
    case, tex = ac.build(96, parts, [])
    blocks = np.frombuffer(encoded(BC3, *chain)[0], np.uint8).view(U32)
    assert blocks.size == 28
    words = np.concatenate([np.array([0x80112233], U32), blocks, blocks, np.zeros(3, U32), blocks])
    table = np.array([[1, 8, 8, 4], [29, 8, 8, 4], [60, 8, 8, 4]], U32)
    return [(case, dict(tex, textures=table, texels=words, formats=np.array([BC3, 4, BC3], U32), texture_count=3), 1)]


# ---- short_buffer
def _short_buffer():
    level = ac.checker(8, 8, 8, 61) | U32(0xFF000000)  # alpha 255 everywhere: only the block that reads 0 fails
    parts = [(quad(4.0, 4.0, 60.0, 60.0, 0.5, 0.55), ac.texel_ratio(4.0, 4.0, 1.0 / 7.0, 1.0 / 7.0, 8, 8), 0, REFERENCE_CUTOFF)]
    case, tex = build(64, parts, [encoded(BC3, level, 8, 8, 1)])
    assert tex["texels"].size == 16
    return [(case, dict(tex, texels=tex["texels"][:14].copy()), 3)]  # the last block has its alpha block and half its colour block


# ---- draw_counts
DRAW_COUNTS = (1, 63, 64, 65)


def _draw_counts():
    entries = [encoded(BC3, tref.build_chain(ac.checker(8, 8, 1, 71), 8, 8), 8, 8, 4), encoded(BC3, tref.build_chain(ac.checker(4, 4, 1, 72, phase=1), 4, 4), 4, 4, 3)]
    runs = []
    for n in DRAW_COUNTS:
        parts = []
        for d in range(n):
            x0, y0 = 1.0 + 7.0 * (d % 9), 1.0 + 7.0 * (d // 9)
            tri = [[(x0, y0, 0.5), (x0 + 6.0, y0, 0.5), (x0 + 6.0, y0 + 6.0, 0.5)]]
            parts.append((tri, ac.texel_ratio(0.0, 0.0, 0.5, 0.5, *((8, 8) if d % 2 == 0 else (4, 4))), d % 2, REFERENCE_CUTOFF))
        runs.append(build(64, parts, entries) + (n % 4,))
    return runs


# ---- the cases of shadow_alpha_cases with their textures re-encoded to BC3
def bc3_of(tex):
    """shadow_alpha_cases texture inputs -> the same with every usable row's levels as BC3 blocks (an unusable row keeps its place as an RGBA8 row without words)"""
    table = np.asarray(tex["textures"], U32).reshape(-1, 4)
    entries, raw = [], {}
    for row, (offset, width, height, mips) in enumerate(table.tolist()):
        if aref.usable(dict(tex, texture_count=table.shape[0]), row) is None:
            raw[row] = (width, height, mips)
            entries.append((np.zeros(0, U32), 0, 0, 0, RGBA8))
            continue
        chain = tex["texels"][offset:offset + tref.chain_texels(width, height, mips)]
        entries.append(encoded(BC3, chain, width, height, mips))
    out_table, words, formats = bc.pack_store(entries)
    for row, (width, height, mips) in raw.items():
        out_table[row, 1:] = (width, height, mips)
    return dict(tex, textures=out_table, texels=words, formats=formats)


def _alpha_case(name):
    return lambda: [(case, bc3_of(tex), cascade) for case, tex, cascade in ac.CASES[name]()]


CASES = {"sizes": _sizes, "alpha_modes": _alpha_modes, "mixed_store": _mixed_store, "bc1_bc5": _bc1_bc5, "unusable": _unusable, "short_buffer": _short_buffer,
         "draw_counts": _draw_counts}
CASES.update({"alpha_" + name: _alpha_case(name) for name in ac.CASES})
_cache = {}


def reference(name):
    """[(case, tex, cascade, format-aware result, opaque result, details)], computed once per case; callers must not modify it"""
    if name not in _cache:
        runs = []
        for case, tex, cascade in CASES[name]():
            details = []
            runs.append((case, tex, cascade, bref.rasterise(case, tex, details), sc.rasterise(case), details))
        _cache[name] = runs
    return _cache[name]


def decoded_reference(name):
    """[(decoded texture inputs, shadow_alpha_reference's result on them)] per run: the store through prepass_bc_reference.decode_store. Computed once"""
    key = ("decoded", name)
    if key not in _cache:
        out = []
        for case, tex, _, _, _, _ in reference(name):
            flat = bc.decode_store(tex)
            out.append((flat, aref.rasterise(case, flat)))
        _cache[key] = out
    return _cache[key]


def _box_codes(r, box):
    x0, y0, x1, y1 = (int(v) for v in box)
    return r["map"][y0:y1, x0:x1]


def _check_sizes(runs):
    case, tex, _, a, o, details = runs[0]
    assert case["res"] == 256 and [tuple(r) for r in tex["textures"][:, 1:3].tolist()] == SIZES and (tex["formats"] == BC3).all()
    assert all(int(m) == tref.full_mip_count(w, h) for (w, h), m in zip(SIZES, tex["textures"][:, 3]))
    for k, (w, h) in enumerate(SIZES):
        mine = [t for t in details if t["draw"] in (2 * k, 2 * k + 1)]
        assert len(mine) == 4 and all(t["format"] == BC3 for t in mine)
        if (w, h) != (1, 1):
            assert any(0 < t["passed"] < t["fragments"] for t in mine), (w, h)
            assert any(t["fw"] != 0 and t["L1"] != t["L0"] for t in mine if t["draw"] == 2 * k + 1), (w, h)
    assert any(w % 4 and w > 4 for w, _ in SIZES) and any(max(w, h) < 4 for w, h in SIZES), "partial blocks, and levels smaller than a block"


def _check_alpha_modes(runs):
    case, tex, _, a, o, details = runs[0]
    blocks = np.frombuffer(tex["texels"].tobytes(), np.uint8).reshape(3, 16)[:, :8]
    codes = bc.decode_alpha_blocks(blocks)
    assert blocks[0, 0] > blocks[0, 1] and blocks[1, 0] < blocks[1, 1] and blocks[2, 0] == blocks[2, 1]
    assert len(set(codes[0].tolist())) == 8 and codes[1, 8] == 0 and codes[1, 6] == 255 and len(set(codes[1].tolist())) == 8, "all eight indices in both modes"
    assert set(codes[2].tolist()) == {77, 0, 255}
    assert {m for t in details for m in t["modes"]} == {"eight", "six"}
    covered = [int((_box_codes(a, _modes_box(k)) != 0).sum()) for k in range(len(MODE_CUTOFFS))]
    assert covered[0] == 48 * 16 >= covered[1] > covered[2] > covered[3] > 0, covered  # (between texel centres a code of 0 blends with its neighbours: cutoff 1 may keep all)
    assert {t["draw"] for t in details} == {1, 2, 3}, "cutoff 0 is never sampled"


def _check_mixed_store(runs):
    case, tex, _, a, o, details = runs[0]
    assert tex["formats"].tolist() == [RGBA8, BC1, BC3, BC5, RGBA8, BC3]
    offsets = tex["textures"][:, 0].tolist()
    assert offsets[0] == 0 and offsets[1] == 20 and tref.chain_texels(5, 3, 3) == 18, "padding in front of the first compressed entry"
    assert all(offsets[k] % 4 == 0 for k in (1, 2, 3, 5)) and offsets[5] > offsets[4] + tref.chain_texels(3, 3, 2) - 1
    assert {t["draw"] for t in details} == {0, 2, 4, 5}, "RGBA8 and BC3 rows are sampled, BC1 and BC5 rows never"
    for k in (0, 2, 4, 5):
        assert any(0 < t["passed"] < t["fragments"] for t in details if t["draw"] == k), k
    for k in (1, 3):
        assert (_box_codes(a, _mixed_box(k)) != 0).all()


def _check_bc1_bc5(runs):
    case, tex, _, a, o, details = runs[0]
    assert tex["formats"].tolist() == [BC1, BC5, BC3] and {t["draw"] for t in details} == {len(CONSTANT_DRAWS) + 1}
    front, behind = ac.code_of(0.6), ac.code_of(0.2)
    for k, (_, word) in enumerate(CONSTANT_DRAWS):
        x0, y0, x1, y1 = (int(v) for v in _constant_box(k))
        assert (a["map"][y0:30, x0:x1] == (0 if word == 256 else front)).all() and (a["map"][30:y1, x0:x1] == (behind if word == 256 else front)).all(), k


def _check_unusable(runs):
    case, tex, _, a, o, details = runs[0]
    assert tex["textures"][0, 0] % 4 == 1 and tex["formats"].tolist() == [BC3, 4, BC3] and tex["textures"][2, 0] % 4 == 0
    assert bref.usable(tex, 0) is None and bref.usable(tex, 1) is None and bref.usable(tex, 2) is not None
    assert {t["draw"] for t in details} == {4} and all(0 < t["passed"] < t["fragments"] for t in details)
    for k, (_, word) in enumerate(UNUSABLE_DRAWS[:4]):
        assert (_box_codes(a, _unusable_box(k)) != 0).all() == (word <= 255) and (_box_codes(a, _unusable_box(k)) != 0).any() == (word <= 255), k


def _check_short_buffer(runs):
    case, tex, _, a, o, details = runs[0]
    assert tex["texels"].size == 14 and tex["textures"].tolist() == [[0, 8, 8, 1]]
    whole = bref.rasterise(case, dict(tex, texels=np.concatenate([tex["texels"], np.zeros(2, U32)])))
    assert (whole["map"][4:60, 4:60] != 0).all(), "with the whole block every fragment passes"
    hole = a["map"][4:60, 4:60] == 0
    assert hole[36:48, 36:48].all() and not hole[:24, :].any() and not hole[:, :24].any(), "the texels of the last block read 0"


def _check_draw_counts(runs):
    assert [r[0]["draws"].shape[0] for r in runs] == list(DRAW_COUNTS) and all(r[0]["res"] == 64 for r in runs)
    for case, tex, _, a, o, details in runs:
        assert {t["draw"] for t in details} == set(range(case["draws"].shape[0])) and a["drawn"] == case["draws"].shape[0]


def _check_alpha(name):
    def check(runs):
        for (case, tex, _, a, o, details), (_, old_tex, _) in zip(runs, ac.CASES[name]()):
            rows = [r for r in range(old_tex["textures"].shape[0]) if aref.usable(dict(old_tex, texture_count=old_tex["textures"].shape[0]), r) is not None]
            assert rows and all(tex["formats"][r] == BC3 for r in rows) and np.array_equal(tex["textures"][rows, 1:], old_tex["textures"][rows, 1:])
        if name == "mip_threshold":
            assert any(t["L1"] != t["L0"] and t["fw"] != 0 for t in runs[0][5]), "a record whose two levels differ"
        if name == "uv_edges":
            case, tex, _, a, o, details = runs[0]
            assert (tex["uvs"] < 0).any() and (tex["uvs"] > 1).any() and any(t["invalid"] > 50 for t in details) and tex["uvs"].shape[0] < case["positions"].shape[0]
    return check


CHECKS = {"sizes": _check_sizes, "alpha_modes": _check_alpha_modes, "mixed_store": _check_mixed_store, "bc1_bc5": _check_bc1_bc5, "unusable": _check_unusable,
          "short_buffer": _check_short_buffer, "draw_counts": _check_draw_counts}
CHECKS.update({"alpha_" + name: _check_alpha(name) for name in ac.CASES})


def check_case_is_what_it_is_for(name):
    runs = reference(name)
    for case, tex, _, a, o, _ in runs:
        assert 64 <= case["res"] <= 256
        assert (a["submitted"], a["drawn"], a["rejects"]) == (o["submitted"], o["drawn"], o["rejects"]), "the counters do not depend on alpha"
        # every case holds a BC3 entry: it shows (a texel differs from the opaque map) and it does not hide everything
        assert (tex["formats"] == BC3).any() and (a["map"] != o["map"]).any() and (a["map"] != 0).any(), name
    CHECKS[name](runs)
