"""The texture store built on the GPU (plrf_build_scene_textures: "textureMipChain.comp", "textureBlockEncode.comp") against tests/texture_build_reference.py, word
for word: one pipeline at 96 x 64 (the prepass frame tests' size), per case one build, one frame and one plrf_read_scene_texture_store.

Every row of the table of accepted format pairs - RGBA8 kept or compressed, levels given or built; a compressed source kept, with its levels or with level 0 alone -
at 1 x 1, 2 x 2, 3 x 5, 4 x 4, 5 x 7, 64 x 32 and 130 x 67 (odd sizes, partial blocks, levels of one block, several workgroups per job); a mixed store of 37 small
textures in all four store formats (the job tables' prefix sums, the 4-word alignment padding), whose build takes at most 14 chain executions and one encode
execution; the caller's level-0 blocks verbatim; refusals that name their cause and leave the store in place.
"""
import numpy as np
import pytest

import prepass_bc_reference as bref
import test_prepass_texture_frame as ttf
import test_texture_build_cpu as cpu
import texture_build_reference as xref

SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (5, 7), (64, 32), (130, 67)]  # (width, height)
RGBA8, BC1, BC3, BC5 = bref.RGBA8, bref.BC1, bref.BC3, bref.BC5
CODE_OF = {RGBA8: 2, BC1: 13, BC3: 14, BC5: 15}  # PLR_FORMAT_*
INVALID_ARGUMENT = ttf.INVALID_ARGUMENT
KINDS = ("noise", "gradient", "two_colour", "anti_correlated", "constant")
U32 = np.uint32


def _level0(width, height, k):
    return cpu.inputs(width, height, seed=3 + k)[KINDS[k % len(KINDS)]]


def _rgba_source(width, height, k, given, stored):
    """an RGBA8 source: `given` = its whole chain, else level 0 with mip_count 0"""
    level0 = _level0(width, height, k)
    if not given:
        return level0.reshape(-1), width, height, 0, RGBA8, stored
    levels = xref.chain(level0)
    return np.concatenate([l.reshape(-1) for l in levels]), width, height, len(levels), RGBA8, stored


def _block_source(width, height, k, given, fmt):
    """a compressed source of random blocks (three-colour BC1 blocks and six-value alpha blocks among them): its chain, else level 0 with mip_count 0"""
    mips = max(width, height).bit_length() if given else 1
    n = sum(int(np.prod(bref.level_blocks(max(1, width >> l), max(1, height >> l)))) for l in range(mips))
    return bref.random_blocks(fmt, n, 40 + k).tobytes(), width, height, mips if given else 0, fmt, fmt


ROWS = {
    "rgba8_levels_given": lambda: [_rgba_source(w, h, k, True, RGBA8) for k, (w, h) in enumerate(SIZES)],
    "rgba8_chain_built": lambda: [_rgba_source(w, h, k, False, RGBA8) for k, (w, h) in enumerate(SIZES)],
    "rgba8_to_bc_levels_given": lambda: [_rgba_source(w, h, 3 * k + f, True, fmt) for k, (w, h) in enumerate(SIZES) for f, fmt in enumerate((BC1, BC3, BC5))],
    "rgba8_to_bc_chain_built": lambda: [_rgba_source(w, h, 3 * k + f, False, fmt) for k, (w, h) in enumerate(SIZES) for f, fmt in enumerate((BC1, BC3, BC5))],
    "bc_levels_given": lambda: [_block_source(w, h, 3 * k + f, True, fmt) for k, (w, h) in enumerate(SIZES) for f, fmt in enumerate((BC1, BC3, BC5))],
    "bc_chain_built": lambda: [_block_source(w, h, 3 * k + f, False, fmt) for k, (w, h) in enumerate(SIZES) for f, fmt in enumerate((BC1, BC3, BC5))],
}


def _mixed_sources():
    """37 textures of 1 .. 21 texels a side: the four store formats in turn, sources RGBA8 and compressed, levels given and built"""
    rng = np.random.default_rng(77)
    out = []
    for k in range(37):
        w, h = int(rng.integers(1, 22)), int(rng.integers(1, 22))
        stored = (RGBA8, BC1, BC3, BC5)[k % 4]
        given = bool((k // 4) % 2)
        out.append(_block_source(w, h, k, given, stored) if stored != RGBA8 and (k // 8) % 2 else _rgba_source(w, h, k, given, stored))
    return out


_reference = {}


def _sources_and_store(name):
    """(sources, (table, words, formats)) of a row or of the mixed store, computed once; callers must not modify it"""
    if name not in _reference:
        sources = _mixed_sources() if name == "mixed" else ROWS[name]()
        _reference[name] = (sources, xref.build_store(sources))
    return _reference[name]


def _api(sources):
    return [(data, w, h, mips, CODE_OF[fmt], CODE_OF[stored]) for data, w, h, mips, fmt, stored in sources]


@pytest.fixture(scope="module")
def scene(backend):
    i = ttf._scene_inputs()
    fp = ttf._pipeline(backend)
    fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
    state = dict(fp=fp, frames=0)
    yield state
    fp.destroy()


def _frame(scene):
    i = ttf._scene_inputs()
    scene["fp"].frame(i["cams"][1 + scene["frames"] % 3], 1.0 / 60.0, 0.5 + scene["frames"] / 60.0)
    scene["frames"] += 1


def _build_and_read(scene, sources):
    i = ttf._scene_inputs()
    scene["fp"].build_scene_textures(_api(sources), i["uvs"], i["materials"])
    _frame(scene)
    return scene["fp"].read_scene_texture_store()


def _assert_store(label, got, want):
    assert got.size == want.size, "%s: %d words, the reference store holds %d" % (label, got.size, want.size)
    differing = np.flatnonzero(got != want)
    print("texture build %-28s: %d of %d words differ" % (label, differing.size, want.size))
    assert differing.size == 0, "%s: first at word %d" % (label, differing[0])


@pytest.mark.gpu
@pytest.mark.parametrize("row", list(ROWS))
def test_gpu_the_store_equals_the_reference_store_word_for_word(scene, row):
    sources, (table, words, formats) = _sources_and_store(row)
    got = _build_and_read(scene, sources)
    _assert_store(row, got, words)
    stats = scene["fp"].texture_build_stats()
    built = row.endswith("chain_built")
    assert (stats["mip_chain_launches"] > 0) == built and (stats["block_encode_launches"] == 1) == (row != "rgba8_levels_given" and row != "rgba8_chain_built" and row != "bc_levels_given")
    assert stats["mip_chain_launches"] <= 14


@pytest.mark.gpu
def test_gpu_a_mixed_store_of_37_textures_takes_at_most_14_chain_launches_and_one_encode_launch(scene):
    sources, (table, words, formats) = _sources_and_store("mixed")
    assert sorted(set(formats.tolist())) == [RGBA8, BC1, BC3, BC5] and len(sources) == 37
    assert any(int(table[t, 0]) % 4 == 0 and t and (int(table[t - 1, 0]) + bref.texture_words(int(formats[t - 1]), *(int(v) for v in table[t - 1, 1:]))) % 4 for t in range(37)), "padding occurs"
    got = _build_and_read(scene, sources)
    _assert_store("37 mixed textures", got, words)
    stats = scene["fp"].texture_build_stats()
    print("texture build stats of the mixed store: %r" % (stats,))
    assert 1 <= stats["mip_chain_launches"] <= 14 and stats["block_encode_launches"] == 1
    # what the two passes did, from the sources: texels of the built levels; blocks of the encoded ones
    chain_texels = blocks = 0
    for data, w, h, mips, fmt, stored in sources:
        levels = [(max(1, w >> l), max(1, h >> l)) for l in range(max(w, h).bit_length())]
        if mips == 0:
            chain_texels += sum(lw * lh for lw, lh in levels[1:])
        if stored != RGBA8 and (fmt == RGBA8 or mips == 0):
            blocks += sum(int(np.prod(bref.level_blocks(lw, lh))) for lw, lh in (levels[:mips] if mips else levels)[0 if fmt == RGBA8 else 1:])
    assert (stats["chain_texels"], stats["blocks_encoded"]) == (chain_texels, blocks)
    assert stats["staging_bytes"] > 0 and stats["staging_bytes"] % 16 == 0


@pytest.mark.gpu
def test_gpu_level_0_of_a_compressed_source_is_the_caller_s_bytes(scene):
    sources, (table, words, formats) = _sources_and_store("bc_chain_built")
    got = _build_and_read(scene, sources)
    for t, (data, w, h, mips, fmt, stored) in enumerate(sources):
        at = int(table[t, 0])
        assert mips == 0 and got[at:at + len(data) // 4].tobytes() == data, "texture %d" % t
    assert any(int(table[t, 3]) > 1 for t in range(len(sources)))


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_leave_the_store_in_place(scene):
    from plainrenderer_amd.backend import PlrError
    fp, i = scene["fp"], ttf._scene_inputs()
    sources, (table, words, formats) = _sources_and_store("rgba8_to_bc_chain_built")

    def refused(call, *said):
        with pytest.raises(PlrError) as e:
            call()
        assert e.value.code == INVALID_ARGUMENT, e.value
        assert all(w in str(e.value) for w in said), e.value

    first = _build_and_read(scene, sources)
    _assert_store("before the refusals", first, words)
    good = _api(sources)
    change = lambda k, **f: [tuple(f.get(n, v) for n, v in zip(("data", "width", "height", "mips", "format", "store_format"), t)) if j == k else t for j, t in enumerate(good)]
    blocks = bref.random_blocks(BC1, 1, 9).tobytes()
    build = lambda textures: fp.build_scene_textures(textures, i["uvs"], i["materials"])
    # the format pairs outside the table: the message names the texture and both formats
    refused(lambda: build(change(3, data=blocks, width=4, height=4, mips=1, format=13, store_format=14)), "unsupported format pair", "texture 3", "format 13", "store_format 14")
    refused(lambda: build(change(2, data=blocks, width=4, height=4, mips=1, format=13, store_format=2)), "unsupported format pair", "texture 2", "format 13", "store_format 2")
    refused(lambda: build(change(1, format=1)), "unsupported format pair", "texture 1", "format 1", "store_format")
    refused(lambda: build(change(0, store_format=7)), "unsupported format pair", "texture 0", "format 2", "store_format 7")
    # a bytes mismatch: RGBA8 level 0 with a word too many; a compressed level 0 given two levels' bytes
    refused(lambda: build(change(4, data=np.zeros(2 * 2 + 1, U32), width=2, height=2, mips=0)), "bytes mismatch", "texture 4", "20 bytes", "hold 16")
    refused(lambda: build(change(5, data=blocks * 2, width=4, height=4, mips=0, format=13, store_format=13)), "bytes mismatch", "texture 5", "16 bytes", "hold 8")
    refused(lambda: build(good[:2] + [good[2][:3] + (9,) + good[2][4:]] + good[3:]), "too many mips", "texture 2")
    refused(lambda: fp.build_scene_textures(good, i["uvs"][:2], i["materials"]), "mesh count 2", "mesh count 3")
    # the store built before the refusals is the one the next frame samples and the readback returns
    _frame(scene)
    _assert_store("after the refusals", fp.read_scene_texture_store(), first)
    # a readback before the build frame says so, and changes nothing: the frame then builds the new store
    other, (_, other_words, _) = _sources_and_store("rgba8_chain_built")
    fp.build_scene_textures(_api(other), i["uvs"], i["materials"])
    refused(lambda: fp.read_scene_texture_store(), "not built yet", "no frame has run since plrf_build_scene_textures")
    _frame(scene)
    _assert_store("after the refused readback", fp.read_scene_texture_store(), other_words)
    # the host path's store reads back too, after its frame; no store: refused
    fp.set_scene_textures([(other[k][0], *other[k][1:4]) for k in range(len(other))], i["uvs"], i["materials"])
    refused(lambda: fp.read_scene_texture_store(), "no frame has run")
    _frame(scene)
    _assert_store("the host's chain", fp.read_scene_texture_store(), other_words)
    fp.build_scene_textures([], [], [])
    refused(lambda: fp.read_scene_texture_store(), "no texture store")
