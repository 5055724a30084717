"""The tests' own block decoder (tests/prepass_bc_reference.py) against hand-worked blocks, the host's decoder (plr_decode_bc_to_rgba8) against it word for word, the
store packer's offsets and alignment, the input conditions of the GPU cases (tests/prepass_bc_cases.py), the host's validation, packing and decoder under the
sanitizers (tools/scene_bc_check.cpp, a stand-alone program), and the entry point at the C boundary; no GPU."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import prepass_bc_cases as bc
import prepass_bc_reference as bref
import prepass_texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBA8, BC1, BC3, BC5 = bref.RGBA8, bref.BC1, bref.BC3, bref.BC5


def rgb565(r5, g6, b5):
    return (r5 << 11) | (g6 << 5) | b5


def colour_block(c0, c1, indices):
    """indices: 16 values 0 .. 3, texel i at bits 2 i"""
    return struct.pack("<HHI", c0, c1, sum(k << (2 * i) for i, k in enumerate(indices)))


def alpha_block(a0, a1, indices):
    """indices: 16 values 0 .. 7, texel i at bits 3 i of a 48-bit little-endian integer"""
    return struct.pack("<BB", a0, a1) + sum(k << (3 * i) for i, k in enumerate(indices)).to_bytes(6, "little")


def word(r, g, b, a):
    return r | (g << 8) | (b << 16) | (a << 24)


FOUR = [0, 1, 2, 3] * 4
# r5 = 25: (25 << 3) | (25 >> 2) = 200 + 6 = 206; g6 = 50: (50 << 2) | (50 >> 4) = 200 + 3 = 203; b5 = 4: 32 + 1 = 33
HI = rgb565(25, 50, 4), (206, 203, 33)
# r5 = 3: 24 + 0 = 24; g6 = 9: 36 + 0 = 36; b5 = 30: 240 + 7 = 247
LO = rgb565(3, 9, 30), (24, 36, 247)


def test_bc1_four_colour_mode_by_hand():
    """c0 > c1 as uint16: index 2 = (2 c0 + c1 + 1) / 3, index 3 = (c0 + 2 c1 + 1) / 3, floor division"""
    assert HI[0] > LO[0]
    got = bref.decode_blocks(BC1, np.frombuffer(colour_block(HI[0], LO[0], FOUR), np.uint8))[0]
    two = [(2 * 206 + 24 + 1) // 3, (2 * 203 + 36 + 1) // 3, (2 * 33 + 247 + 1) // 3]   # 437 / 3 = 145, 443 / 3 = 147, 314 / 3 = 104
    three = [(206 + 2 * 24 + 1) // 3, (203 + 2 * 36 + 1) // 3, (33 + 2 * 247 + 1) // 3]  # 255 / 3 = 85, 276 / 3 = 92, 528 / 3 = 176
    assert two == [145, 147, 104] and three == [85, 92, 176]
    assert got.tolist() == [word(*HI[1], 255), word(*LO[1], 255), word(*two, 255), word(*three, 255)] * 4


def test_bc1_three_colour_mode_by_hand_and_index_3_is_opaque_black():
    """c0 < c1 and c0 == c1: index 2 = (c0 + c1 + 1) >> 1, index 3 = (0, 0, 0) with alpha 255"""
    got = bref.decode_blocks(BC1, np.frombuffer(colour_block(LO[0], HI[0], FOUR), np.uint8))[0]
    mid = [(24 + 206 + 1) >> 1, (36 + 203 + 1) >> 1, (247 + 33 + 1) >> 1]  # 115, 120, 140
    assert mid == [115, 120, 140]
    assert got.tolist() == [word(*LO[1], 255), word(*HI[1], 255), word(*mid, 255), word(0, 0, 0, 255)] * 4
    same = bref.decode_blocks(BC1, np.frombuffer(colour_block(HI[0], HI[0], FOUR), np.uint8))[0]
    # (206 + 206 + 1) >> 1 = 206, (203 + 203 + 1) >> 1 = 203, (33 + 33 + 1) >> 1 = 33
    assert same.tolist() == [word(*HI[1], 255), word(*HI[1], 255), word(*HI[1], 255), word(0, 0, 0, 255)] * 4


def test_bc1_texel_order_is_row_major_within_the_block():
    """texel (x, y) is position 4 (y & 3) + (x & 3): index k only at position 4 * 2 + 1 -> texel (1, 2)"""
    indices = [0] * 16
    indices[9] = 1
    level = bref.decode_level(BC1, 4, 4, colour_block(HI[0], LO[0], indices))
    assert level[2, 1] == word(*LO[1], 255) and (np.delete(level.reshape(-1), 9) == word(*HI[1], 255)).all()


ALPHA_ALL = list(range(8)) * 2


def test_alpha_block_eight_value_mode_by_hand():
    """a0 = 200 > a1 = 31: index k = 2 .. 7 is ((8 - k) a0 + (k - 1) a1 + 3) / 7"""
    got = bref.decode_alpha_blocks(np.frombuffer(alpha_block(200, 31, ALPHA_ALL), np.uint8))[0]
    # k = 2: (1200 + 31 + 3) / 7 = 176; 3: (1000 + 62 + 3) / 7 = 152; 4: (800 + 93 + 3) / 7 = 128; 5: (600 + 124 + 3) / 7 = 103; 6: (400 + 155 + 3) / 7 = 79; 7: (200 + 186 + 3) / 7 = 55
    assert got.tolist() == [200, 31, 176, 152, 128, 103, 79, 55] * 2


def test_alpha_block_six_value_mode_by_hand_with_codes_6_and_7():
    """a0 = 31 <= a1 = 200: index k = 2 .. 5 is ((6 - k) a0 + (k - 1) a1 + 2) / 5, 6 is 0, 7 is 255; a0 == a1 is this mode too"""
    got = bref.decode_alpha_blocks(np.frombuffer(alpha_block(31, 200, ALPHA_ALL), np.uint8))[0]
    # k = 2: (124 + 200 + 2) / 5 = 65; 3: (93 + 400 + 2) / 5 = 99; 4: (62 + 600 + 2) / 5 = 132; 5: (31 + 800 + 2) / 5 = 166
    assert got.tolist() == [31, 200, 65, 99, 132, 166, 0, 255] * 2
    same = bref.decode_alpha_blocks(np.frombuffer(alpha_block(77, 77, ALPHA_ALL), np.uint8))[0]
    assert same.tolist() == [77, 77, 77, 77, 77, 77, 0, 255] * 2  # (4 * 77 + 77 + 2) / 5 = 77


def test_bc3_colour_block_is_four_colour_whatever_the_order_of_its_endpoints():
    """bytes 0 - 7 the alpha block, 8 - 15 the colour block with c0 <= c1: still (2 c0 + c1 + 1) / 3 and (c0 + 2 c1 + 1) / 3, not the mean and black"""
    for c0, c1 in ((LO, HI), (HI, HI)):
        got = bref.decode_blocks(BC3, np.frombuffer(alpha_block(200, 31, ALPHA_ALL) + colour_block(c0[0], c1[0], FOUR), np.uint8))[0]
        two = [(2 * a + b + 1) // 3 for a, b in zip(c0[1], c1[1])]
        three = [(a + 2 * b + 1) // 3 for a, b in zip(c0[1], c1[1])]
        alphas = [200, 31, 176, 152, 128, 103, 79, 55] * 2
        colours = [c0[1], c1[1], two, three] * 4
        assert got.tolist() == [word(*colours[i], alphas[i]) for i in range(16)]
    # LO, HI: index 2 = (48 + 206 + 1) / 3 = 85, (72 + 203 + 1) / 3 = 92, (494 + 33 + 1) / 3 = 176 - not the three-colour mean (115, 120, 140)
    assert [(2 * a + b + 1) // 3 for a, b in zip(LO[1], HI[1])] == [85, 92, 176]


def test_bc5_is_two_alpha_blocks_as_red_and_green():
    got = bref.decode_blocks(BC5, np.frombuffer(alpha_block(200, 31, ALPHA_ALL) + alpha_block(31, 200, ALPHA_ALL[::-1]), np.uint8))[0]
    red, green = [200, 31, 176, 152, 128, 103, 79, 55] * 2, ([31, 200, 65, 99, 132, 166, 0, 255] * 2)[::-1]
    assert got.tolist() == [word(red[i], green[i], 0, 255) for i in range(16)]


def test_levels_smaller_than_a_block_and_partial_blocks():
    """5 x 7 is 2 x 2 blocks; texel (4, 6) is position 4 * 2 + 0 of block (1, 1); a 1 x 1 level is position 0 of its one block"""
    assert bref.level_blocks(5, 7) == (2, 2) and bref.level_blocks(2, 3) == (1, 1) and bref.level_blocks(16384, 1) == (4096, 1)
    data = bref.random_blocks(BC3, 4, 5)
    level = bref.decode_level(BC3, 5, 7, data.tobytes())
    per_block = bref.decode_blocks(BC3, data)
    assert level.shape == (7, 5) and level[6, 4] == per_block[3, 8] and level[3, 3] == per_block[0, 15] and level[4, 0] == per_block[2, 0]
    assert bref.decode_level(BC3, 1, 1, data[:1].tobytes())[0, 0] == per_block[0, 0]
    assert bref.texture_words(BC1, 5, 7, 3) == 2 * (4 + 1 + 1) and bref.texture_words(BC5, 16, 16, 5) == 4 * (16 + 4 + 1 + 1 + 1)


@pytest.mark.parametrize("fmt, name", [(BC1, "BC1"), (BC3, "BC3"), (BC5, "BC5")])
def test_the_host_decoder_equals_the_numpy_decoder_on_4096_random_blocks(fmt, name):
    """through ctypes, word for word: as one 256 x 256 level, and block by block as 4 x 4 levels for the first 64"""
    from plainrenderer_amd import ImageFormat, image_io
    blocks = bref.random_blocks(fmt, 4096, 100 + fmt)
    want = bref.decode_level(fmt, 256, 256, blocks.tobytes())
    got = image_io.decode_bc_to_rgba8(ImageFormat[name], 256, 256, blocks)
    assert got.dtype == np.uint32 and np.array_equal(got, want), "first difference at %r" % (tuple(np.argwhere(got != want)[0]) if (got != want).any() else None,)
    per_block = bref.decode_blocks(fmt, blocks)
    for b in range(64):
        assert np.array_equal(image_io.decode_bc_to_rgba8(ImageFormat[name], 4, 4, blocks[b]).reshape(-1), per_block[b])


def test_the_host_decoder_on_odd_sizes_and_its_refusals():
    from plainrenderer_amd import ImageFormat, PlrError, image_io
    for width, height in ((1, 1), (5, 7), (2, 3), (64, 1)):
        for fmt, name in ((BC1, "BC1"), (BC3, "BC3"), (BC5, "BC5")):
            bw, bh = bref.level_blocks(width, height)
            blocks = bref.random_blocks(fmt, bw * bh, 7 * width + height)
            assert image_io.bc_level_bytes(ImageFormat[name], width, height) == blocks.size
            assert np.array_equal(image_io.decode_bc_to_rgba8(ImageFormat[name], width, height, blocks), bref.decode_level(fmt, width, height, blocks.tobytes()))
    one = bref.random_blocks(BC1, 1, 1)
    for call, words in ((lambda: image_io.decode_bc_to_rgba8(ImageFormat.RGBA8, 4, 4, one), ("format 2", "PLR_FORMAT_BC1")),
                        (lambda: image_io.decode_bc_to_rgba8(ImageFormat.BC1, 0, 4, one), ("0 x 4",)),
                        (lambda: image_io.decode_bc_to_rgba8(ImageFormat.BC1, 5, 4, one), ("bytes mismatch", "8 bytes", "holds 16")),
                        (lambda: image_io.decode_bc_to_rgba8(ImageFormat.BC3, 4, 4, one), ("bytes mismatch", "holds 16"))):
        with pytest.raises(PlrError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)


def test_the_packer_places_compressed_textures_at_multiples_of_16_bytes():
    rgba = (tc.chain(tc.pattern(5, 3, 1), 5, 3), 5, 3, 3, RGBA8)  # 18 words
    table, words, formats = bref.pack_store([rgba, bc.full(BC1, 4, 4, 2), (tc.pattern(1, 1, 3), 1, 1, 1, RGBA8), bc.full(BC5, 5, 7, 4), bc.full(BC3, 4, 4, 5)])
    # 18 -> BC1 at 20 with 3 levels of one block (6 words) -> RGBA8 at 26 -> BC5 at 28 (2 x 2 + 1 + 1 blocks: 24 words) -> BC3 at 52 (3 blocks: 12 words)
    assert table[:, 0].tolist() == [0, 20, 26, 28, 52] and words.size == 64 and formats.tolist() == [RGBA8, BC1, RGBA8, BC5, BC3]
    assert not words[18:20].any() and not words[27:28].any()
    assert all(int(o) % 4 == 0 for o, f in zip(table[:, 0], formats) if f != RGBA8)
    decoded = bref.decode_store(dict(textures=table, texels=words, formats=formats))
    assert decoded["textures"][:, 0].tolist() == [0, 18, 18 + 21, 40, 40 + 42] and "formats" not in decoded
    assert np.array_equal(decoded["texels"][:18], rgba[0]) and np.array_equal(decoded["texels"][40:75].reshape(7, 5), bc._level0(dict(textures=table, texels=words, formats=formats), 3))


@pytest.mark.parametrize("name", list(bc.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test"""
    bc.check_case_is_what_it_is_for(name)


def test_the_host_validation_packing_and_decoder_run_clean_under_the_sanitizers(tmp_path):
    """every refusal of the new entry point's validation, the packing and the decoder at 1 x 1, 5 x 7 and 16384 x 1: tools/scene_bc_check.cpp, a stand-alone program"""
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "scene_bc_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "scene_bc_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "scene_bc_check: ok", run.stdout + run.stderr


def test_the_entry_points_are_exported_and_the_structure_has_the_header_s_layout():
    from plainrenderer_amd import ImageFormat, backend
    from plainrenderer_amd.frame import FramePipeline, PlrfSceneTextureData
    lib = backend._load()
    assert getattr(lib, "plrf_set_scene_textures_formatted") is not None and getattr(lib, "plr_decode_bc_to_rgba8") is not None
    assert C.sizeof(PlrfSceneTextureData) == 32 and PlrfSceneTextureData.bytes.offset == 8 and PlrfSceneTextureData.format.offset == 28
    assert (int(ImageFormat.RGBA8), int(ImageFormat.BC1), int(ImageFormat.BC3), int(ImageFormat.BC5)) == (2, 13, 14, 15)
    assert hasattr(FramePipeline, "set_scene_textures_formatted")
    header = open(os.path.join(ROOT, "include", "plr_frame.h")).read()
    assert "int plrf_set_scene_textures_formatted(void* pipeline, const plrf_scene_texture_data* textures, uint32_t texture_count" in header
