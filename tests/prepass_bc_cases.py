"""Inputs of the block-compressed texture tests of "depthPrepassRaster.comp" (tests/test_prepass_bc.py, tests/test_prepass_bc_cpu.py): named cases at the smallest
shapes at which the block decode can still go wrong, each with a check, on the reference alone, that the case is what it is for.

A run is (prepass case, texture store, normal inputs or None, cutoffs or None): the dict of tests/prepass_raster_cases.py, the mixed store tests/prepass_bc_reference.py
describes, and what tests/prepass_normal_cases.py and tests/prepass_alpha_cases.py hand their references. Frames are at most 70 x 66, textures at most 16 x 16.
  magnify_repeat     a 4 x 4 BC1 (four-colour) and a 4 x 4 BC1 (three-colour) on a quad with UVs from -1 to 2: level 0 only, every tap wraps inside one block
  magnify_bc3        an 8 x 8 BC3 at 0.75 texels per pixel, UVs from 0 to 1.5: taps cross block edges and the texture edge
  level_between      16 x 16 BC1 and BC3 with the full chain down to 1 x 1 at 3 and at 6 texels per pixel: levels 1 | 2 (2 x 2 blocks | 1 block) and 2 | 3 (a 2 x 2 level)
  partial_blocks     5 x 7 with the chain 2 x 3 and 1 x 1 in all three formats, magnified and minified: blocks that reach past their level
  bias_negative / bias_positive   g_mipBias -0.75 and +1.5 on an 8 x 8 BC3 with 4 levels: the lower clamp in the first, the upper (the 1 x 1 level) in the second
  ragged             70 x 66, one triangle over every pixel, a 16 x 16 BC1 and an 8 x 16 BC5
  mixed              one store with RGBA8 (18 words: the BC1 behind it is moved to word 20), BC1, BC3 and BC5 across albedo and specular of two draws
  alpha_holes        a BC3 albedo whose alpha blocks hold 0 and 255 on a card in front of a quad, cutoff 128: depth and motion change behind the holes
  normal_bc5         a BC5 normal map under both decodes
  hazard_format      a format code 7: the draw's constant word
  hazard_misaligned  a BC1 at an odd word and a BC3 at a word that is no multiple of 4: constant words; an aligned BC1 beside them samples
  hazard_end         a BC3 whose last block crosses the end of `texels` (zeros from that block alone) and a BC1 wholly behind it (zeros)
"""
import numpy as np

import prepass_alpha_cases as ac
import prepass_bc_reference as bref
import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
from shadow_raster_cases import quad

F32 = np.float32
NONE = tref.NONE
RGBA8, BC1, BC3, BC5 = bref.RGBA8, bref.BC1, bref.BC3, bref.BC5
HAZARDS = ("hazard_format", "hazard_misaligned", "hazard_end")


def blocks(fmt, width, height, mips, seed, colour_order=None, alpha_binary=False):
    """random blocks of all levels, as bytes. colour_order: '>' forces c0 > c1 in every colour block, '<=' c0 <= c1; alpha_binary: every alpha block is
    {a0 = 255, a1 = 0, indices 0 | 1}: alpha 255 or 0"""
    n = sum(np.prod(bref.level_blocks(*tref.level_size(width, height, l))) for l in range(mips))
    b = bref.random_blocks(fmt, int(n), seed)
    at = {BC1: 0, BC3: 8}.get(fmt)
    if colour_order and at is not None:
        c0 = b[:, at].astype(np.uint16) | (b[:, at + 1].astype(np.uint16) << 8)
        c1 = b[:, at + 2].astype(np.uint16) | (b[:, at + 3].astype(np.uint16) << 8)
        hi, lo = np.maximum(c0, c1), np.minimum(c0, c1)
        if colour_order == ">":
            hi = np.where(hi == lo, hi ^ np.uint16(0x0821), hi)  # (equal endpoints would be three-colour mode)
            hi, lo = np.maximum(hi, lo), np.minimum(hi, lo)
            c0, c1 = hi, lo
        else:
            c0, c1 = lo, hi
        b[:, at], b[:, at + 1], b[:, at + 2], b[:, at + 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    if alpha_binary:
        rng = np.random.default_rng(seed + 1000)
        b[:, 0], b[:, 1] = 255, 0
        bits = np.zeros(b.shape[0], np.uint64)
        for i in range(16):
            bits |= rng.integers(0, 2, b.shape[0]).astype(np.uint64) << np.uint64(3 * i)
        for k in range(6):
            b[:, 2 + k] = (bits >> np.uint64(8 * k)) & np.uint64(255)
    return b.tobytes()


def full(fmt, width, height, seed, **how):
    mips = tref.full_mip_count(width, height)
    return blocks(fmt, width, height, mips, seed, **how), width, height, mips, fmt


def store(case, uvs, materials, textures, mip_bias=0.0, texture_count=None):
    table, words, formats = textures if isinstance(textures, tuple) else bref.pack_store(textures)
    return dict(uvs=np.asarray(uvs, F32).reshape(-1, 2), materials=np.asarray(materials, np.uint32).reshape(-1, 2), textures=table, texels=words, formats=formats,
                texture_count=table.shape[0] if texture_count is None else int(texture_count), mip_bias=float(F32(mip_bias)))


def _one_quad(size=16):
    return pc.pixel_case([quad(0.0, 0.0, float(size), float(size), 0.5, 0.5)], size, size)


def _magnify_repeat():
    case = _one_quad()
    uvs = tc.pixel_uvs(case, lambda x, y: (-1.0 + 3.0 * x / 16.0, -1.0 + 3.0 * y / 16.0))
    return [(case, store(case, uvs, [(0, 1)], [full(BC1, 4, 4, 1, colour_order=">"), full(BC1, 4, 4, 2, colour_order="<=")]), None, None)]


def _magnify_bc3():
    case = _one_quad()
    uvs = tc.pixel_uvs(case, lambda x, y: (1.5 * x / 16.0, 1.5 * y / 16.0))
    return [(case, store(case, uvs, [(0, 1)], [full(BC3, 8, 8, 3, colour_order="<="), full(BC3, 8, 8, 4)]), None, None)]


def _level_between():
    runs = []
    for scale in (3.0, 6.0):
        case = _one_quad()
        uvs = tc.pixel_uvs(case, lambda x, y: (scale * x / 16.0, scale * y / 16.0))
        runs.append((case, store(case, uvs, [(0, 1)], [full(BC1, 16, 16, 5), full(BC3, 16, 16, 6)]), None, None))
    return runs


def _partial_blocks():
    runs = []
    for scale in (2.5, 8.0):
        quads = [quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5), quad(0.0, 16.0, 16.0, 32.0, 0.5, 0.5)]
        case = pc.pixel_case(quads, 32, 32)
        uvs = tc.pixel_uvs(case, lambda x, y: (scale * x / 16.0, scale * y / 16.0))
        textures = [full(BC1, 5, 7, 7), full(BC3, 5, 7, 8), full(BC5, 5, 7, 9)]
        runs.append((case, store(case, uvs, [(k, (k + 1) % 3) for k in range(3)], textures), None, None))
    return runs


def _bias(mip_bias):
    """as prepass_texture_cases._bias: draw 0 at 1 / 2 texel per pixel (lod -1 before the bias), draw 1 at 4 texels per pixel (lod 2)"""
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5)], 32, 16)
    uvs = tc.quad_uvs(case, [lambda x, y: (x / 16.0, y / 16.0), lambda x, y: (8.0 * (x - 16.0) / 16.0, 8.0 * y / 16.0)])
    return [(case, store(case, uvs, [(0, 0), (0, 0)], [full(BC3, 8, 8, 11)], mip_bias=mip_bias), None, None)]


def _ragged():
    case = pc.pixel_case([[[(-1.0, -1.0, 0.1), (150.0, -1.0, 0.9), (-1.0, 150.0, 0.5)]]], 70, 66)
    uvs = tc.pixel_uvs(case, lambda x, y: (3.0 * x / 70.0, 3.0 * y / 66.0))
    return [(case, store(case, uvs, [(0, 1)], [full(BC1, 16, 16, 12), full(BC5, 8, 16, 13)]), None, None)]


def _mixed():
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.5, 0.5), quad(16.0, 0.0, 32.0, 16.0, 0.5, 0.5)], 32, 16)
    uvs = tc.pixel_uvs(case, lambda x, y: (1.25 * x / 16.0, 1.25 * y / 16.0))
    rgba = (tc.chain(tc.pattern(5, 3, 14), 5, 3), 5, 3, 3, RGBA8)  # 15 + 2 + 1 = 18 words
    return [(case, store(case, uvs, [(0, 1), (2, 3)], [rgba, full(BC1, 8, 8, 15), full(BC3, 8, 4, 16), full(BC5, 4, 8, 17)]), None, None)]


def _alpha_holes():
    """draw 0 the rear quad, draw 1 the card in front of it (as prepass_normal_cases._with_alpha): 8 x 8 texels over 16 x 16 pixels, level 0"""
    case = pc.pixel_case([quad(0.0, 0.0, 16.0, 16.0, 0.3, 0.3), quad(0.0, 0.0, 16.0, 16.0, 0.6, 0.6)], 16, 16)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 16.0, y / 16.0))
    return [(case, store(case, uvs, [(NONE, NONE), (0, NONE)], [full(BC3, 8, 8, 18, alpha_binary=True)]), None, np.array([0, ac.REFERENCE_CUTOFF], np.uint32))]


def _normal_bc5():
    runs = []
    for decode in (nref.DECODE_REFERENCE, nref.DECODE_UNIT):
        case = nc.with_normals(pc.pixel_case([quad(0.0, 0.0, 8.0, 16.0, 0.5, 0.5), quad(8.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16), (0.0, 0.0, 1.0))
        uvs = tc.pixel_uvs(case, lambda x, y: (x / 8.0, y / 8.0))
        tex = store(case, uvs, [(NONE, NONE), (1, NONE)], [full(BC5, 8, 8, 19), full(BC1, 4, 4, 20)])
        runs.append((case, tex, nc.normal_inputs(case, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), [0, 0], decode), None))
    return runs


def _hazard_quads(materials, textures, texture_count=None):
    case = pc.pixel_case([quad(0.0, 0.0, 8.0, 16.0, 0.5, 0.5), quad(8.0, 0.0, 16.0, 16.0, 0.5, 0.5)], 16, 16)
    uvs = tc.pixel_uvs(case, lambda x, y: (x / 8.0, y / 8.0))
    return case, store(case, uvs, materials, textures, texture_count=texture_count), None, None


def _hazard_format():
    table, words, formats = bref.pack_store([full(BC1, 4, 4, 21), full(BC1, 4, 4, 22)])
    formats[0] = 7
    return [_hazard_quads([(0, 0), (1, 1)], (table, words, formats))]


def _hazard_misaligned():
    one = lambda fmt, seed: np.frombuffer(blocks(fmt, 4, 4, 1, seed), np.uint8).view(np.uint32)
    words = np.concatenate([[0xA5A5A5A5], one(BC1, 23), [1, 2, 3], one(BC3, 24), one(BC1, 25)]).astype(np.uint32)  # BC1 at word 1, BC3 at word 6, BC1 at word 10
    table = np.array([(1, 4, 4, 1), (6, 4, 4, 1), (10, 4, 4, 1)], np.uint32)
    return [_hazard_quads([(0, 0), (1, 2)], (table, words, np.array([BC1, BC3, BC1], np.uint32)))]


def _hazard_end():
    table, words, formats = bref.pack_store([(blocks(BC3, 8, 8, 1, 26), 8, 8, 1, BC3), (blocks(BC1, 4, 4, 1, 27), 4, 4, 1, BC1)])
    assert table[:, 0].tolist() == [0, 16] and words.size == 18
    return [_hazard_quads([(0, 0), (1, 1)], (table, words[:14].copy(), formats))]  # the BC3's fourth block has 2 of its 4 words; the BC1 lies behind the end


CASES = dict(magnify_repeat=_magnify_repeat, magnify_bc3=_magnify_bc3, level_between=_level_between, partial_blocks=_partial_blocks, bias_negative=lambda: _bias(-0.75),
             bias_positive=lambda: _bias(1.5), ragged=_ragged, mixed=_mixed, alpha_holes=_alpha_holes, normal_bc5=_normal_bc5, hazard_format=_hazard_format,
             hazard_misaligned=_hazard_misaligned, hazard_end=_hazard_end)

_reference_cache = {}


def reference(name):
    """[(case, store, normal inputs, cutoffs, the decoded all-RGBA8 store, the five images and counters, shadingNormal or None)], computed once; callers must not
    modify it"""
    if name not in _reference_cache:
        out = []
        for case, tex, nm, cutoffs in CASES[name]():
            decoded = bref.decode_store(tex)
            base = nc.base_images(case, decoded, cutoffs)
            out.append((case, tex, nm, cutoffs, decoded, base, None if nm is None else nref.shade(case, decoded, nm, base["keys"], base["normal"])))
        _reference_cache[name] = out
    return _reference_cache[name]


def _channel(words, k):
    return (np.asarray(words, np.uint32) >> np.uint32(8 * k)) & np.uint32(255)


def _level0(tex, row):
    """the decoded level 0 of store row `row`, h x w words"""
    offset, width, height, mips = (int(v) for v in tex["textures"][row])
    fmt = int(tex["formats"][row])
    n = bref.level_words(fmt, width, height)
    return bref.decode_level(fmt, width, height, tex["texels"][offset:offset + n].tobytes())


def _diagnostics(case, decoded, base):
    return tref.sample(case, decoded, base["keys"], diagnostics=True)["diagnostics"]


def _check_magnify_repeat(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    d = _diagnostics(case, decoded, base)["albedo"]
    assert (base["keys"] != 0).all() and (d["L0"] == 0).all() and (d["fw"] == 0).all() and d["tu_min"] < 0
    w = np.frombuffer(tex["texels"].tobytes(), np.uint16)
    assert w[0] > w[1], "texture 0 is in four-colour mode"
    o = int(tex["textures"][1, 0]) * 2
    assert w[o] <= w[o + 1], "texture 1 is in three-colour mode"
    assert (_channel(base["albedo"], 3) == 255).all() and (_channel(base["specular"], 3) == 255).all(), "BC1 alpha is 255, index 3 of three-colour mode included"
    # pixel (5, 5) by hand, as in prepass_texture_cases: x0 = 3, fx = 160, x1 = 0 (the wrap inside the one block); v likewise
    t = _level0(tex, 0)
    for k in range(4):
        c = lambda x, y: int(_channel(t[y, x], k))
        S = 256 * (96 * 96 * c(3, 3) + 160 * 96 * c(0, 3) + 96 * 160 * c(3, 0) + 160 * 160 * c(0, 0))
        assert int(_channel(base["albedo"][5, 5], k)) == (S + (1 << 23) - 1 + ((S >> 24) & 1)) >> 24


def _check_magnify_bc3(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    d = _diagnostics(case, decoded, base)["albedo"]
    assert (d["L0"] == 0).all() and (d["fw"] == 0).all(), "0.75 texels per pixel"
    w = np.frombuffer(tex["texels"].tobytes(), np.uint16)
    assert all(w[8 * b + 4] <= w[8 * b + 5] for b in range(4)), "texture 0's colour blocks have c0 <= c1 and are four-colour all the same"
    t = _level0(tex, 0)
    assert np.unique(_channel(t, 3)).size > 4, "the alpha varies"
    # pixel (5, 0): u = 1.5 * 5.5 / 16: u * 8 - 0.5 = 3.625: x0 = 3, x1 = 4 - the tap pair crosses the block edge; pixel (11, 0): u * 8 - 0.5 = 8.125 - 0.5 ... x0 = 7, x1 = 0
    u = 1.5 * (np.arange(16) + 0.5) / 16.0 * 8.0 - 0.5
    x0 = np.floor(u).astype(int)
    assert 3 in x0 and 7 in x0 and 8 in x0, "tap pairs (3, 4), (7, 0) and the repeat beyond the edge"
    assert np.unique(base["albedo"]).size > 100


def _check_level_between(runs):
    for (case, tex, nm, cutoffs, decoded, base, sn), (l0, fw) in zip(runs, ((1, 150), (2, 150))):
        d = _diagnostics(case, decoded, base)["albedo"]
        assert (d["L0"] == l0).all() and np.unique(d["fw"]).tolist() == [fw], "lod = log2(3) and log2(6)"
        assert tex["textures"][0].tolist() == [0, 16, 16, 5] and int(tex["textures"][1, 0]) == 2 * (16 + 4 + 1 + 1 + 1) + 2, "block grids of 4 x 4, 2 x 2 and three single blocks: 46 words, the BC3 at 48"
        assert np.unique(base["albedo"]).size > 8 and np.unique(base["specular"]).size > 8


def _check_partial_blocks(runs):
    for (case, tex, nm, cutoffs, decoded, base, sn), levels in zip(runs, ((0,), (1, 2))):
        assert tex["textures"][:, 1:].tolist() == [[5, 7, 3]] * 3
        assert tex["textures"][:, 0].tolist() == [0, 2 * (4 + 1 + 1), 12 + 4 * 6], "2 x 2 blocks, then one block for 2 x 3 and one for 1 x 1"
        assert decoded["textures"][:, 0].tolist() == [0, 42, 84], "35 + 6 + 1 texels each"
        d = _diagnostics(case, decoded, base)["albedo"]
        won = base["keys"] != 0
        assert sorted(np.unique(d["L0"][won]).tolist()) == list(levels)[:len(np.unique(d["L0"][won]))] and set(np.unique(d["L0"][won]).tolist()) <= set(levels)
        assert (_channel(base["albedo"][16:, :16], 2) == 0).all() and (_channel(base["albedo"][16:, :16], 3) == 255).all(), "BC5 is (R, G, 0, 255)"


def _check_bias_negative(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    d = _diagnostics(case, decoded, base)["albedo"]
    assert (d["lod"][:, :16] == 0).all() and (d["L0"][:, 16:] == 1).all() and (d["fw"][:, 16:] == 64).all()


def _check_bias_positive(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    d = _diagnostics(case, decoded, base)["albedo"]
    assert (d["L0"][:, :16] == 0).all() and (d["fw"][:, :16] == 128).all()
    assert (d["L0"][:, 16:] == 3).all() and (d["fw"][:, 16:] == 0).all(), "the 1 x 1 level: one texel of one block"
    assert np.unique(base["albedo"][:, 16:]).size == 1


def _check_ragged(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    assert (case["width"], case["height"]) == (70, 66) and (base["keys"] != 0).all()
    assert np.unique(base["albedo"]).size > 100 and np.unique(base["specular"]).size > 100


def _check_mixed(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    assert tex["formats"].tolist() == [RGBA8, BC1, BC3, BC5]
    assert tex["textures"][:, 0].tolist() == [0, 20, 36, 36 + 4 * (2 + 1 + 1 + 1)] and not tex["texels"][18:20].any() and not tex["texels"][34:36].any(), "two words of padding behind the RGBA8 texture, and two behind the BC1's 14"
    assert tex["materials"].tolist() == [[0, 1], [2, 3]]
    for image in ("albedo", "specular"):
        assert np.unique(base[image][:, :16]).size > 8 and np.unique(base[image][:, 16:]).size > 8
    assert (_channel(base["specular"][:, 16:], 2) == 0).all(), "draw 1's specular is the BC5"


def _check_alpha_holes(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    opaque = nc.base_images(case, decoded, None)
    holes = base["depth"] != opaque["depth"]
    assert 20 < holes.sum() < 236, "the card has holes and is not all holes: %d" % holes.sum()
    assert not np.array_equal(base["motion"], opaque["motion"]) or not np.array_equal(base["albedo"], opaque["albedo"])
    assert set(np.unique(_channel(_level0(tex, 0), 3)).tolist()) == {0, 255}
    own = (base["keys"] & np.uint64(0xFFFFFFFF)) >= 2
    assert (_channel(base["albedo"][own], 3) >= 128).all() and own.sum() > 20


def _check_normal_bc5(runs):
    assert [nm["decode"] for _, _, nm, _, _, _, _ in runs] == [nref.DECODE_REFERENCE, nref.DECODE_UNIT]
    for case, tex, nm, cutoffs, decoded, base, sn in runs:
        assert int(tex["formats"][0]) == BC5 and nm["normal_materials"].tolist() == [0, 0]
        assert np.unique(sn).size > 30 and not np.array_equal(sn, base["normal"])
    assert not np.array_equal(runs[0][6], runs[1][6]), "the decodes differ"


def _constants(case, draw):
    return int(case["draws"][draw, 4]), int(case["draws"][draw, 5])


def _check_hazard_format(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    assert tex["formats"].tolist() == [7, BC1]
    assert (base["albedo"][:, :8] == _constants(case, 0)[0]).all() and (base["specular"][:, :8] == _constants(case, 0)[1]).all()
    assert np.unique(base["albedo"][:, 8:]).size > 3, "a sample (one block has four colours)"


def _check_hazard_misaligned(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    assert tex["textures"][:, 0].tolist() == [1, 6, 10]
    assert (base["albedo"][:, :8] == _constants(case, 0)[0]).all() and (base["specular"][:, :8] == _constants(case, 0)[1]).all()
    assert (base["albedo"][:, 8:] == _constants(case, 1)[0]).all() and np.unique(base["specular"][:, 8:]).size > 3


def _check_hazard_end(runs):
    (case, tex, nm, cutoffs, decoded, base, sn), = runs
    assert tex["texels"].size == 14
    left = base["albedo"][:, :8]
    assert (left == 0).any() and (left != 0).any(), "the taps of the fourth block read 0 in all four channels, the others do not"
    assert (decoded["texels"][:64].reshape(8, 8)[4:, 4:] == 0).all() and (decoded["texels"][:64].reshape(8, 8)[:4, :] != 0).any()
    assert not base["albedo"][:, 8:].any() and not base["specular"][:, 8:].any(), "every tap of the BC1 reads 0"


CASE_CHECKS = {name: globals()["_check_" + name] for name in CASES}


def check_case_is_what_it_is_for(name):
    CASE_CHECKS[name](reference(name))
