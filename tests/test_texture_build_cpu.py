"""The texture build's contracts without a GPU: the numpy reference (tests/texture_build_reference.py) against a chain written as loops, the host's
plr_encode_rgba8_to_bc against the reference byte for byte, properties of the encode contract derived from its text and checked on the reference alone, and the DDS
writer's BC1 / BC3 / BC5 payloads.

The derived properties:
  constant block     q5 / q6 round v 31 / 255 (v 63 / 255) to the nearest code and the decode expands a code q to q 255 / 31 (q 255 / 63) rounded down to a whole number
                     by bit replication: half a code step is 255 / 62 = 4.11 (255 / 126 = 2.02), so |decode - v| <= 4 for r and b and <= 2 for g
  two values         an alpha block whose texels take two values has them as a0 and a1: palette entries 0 and 1, distance 0
  alpha bound        the eight palette values are a1 + (8 - k) R / 7 rounded to the nearest whole number, an error of at most 3 / 7 each; neighbours are R / 7 apart, so a
                     value between a1 and a0 is within R / 14 + 3 / 7 of one: 14 |d - v| <= R + 6
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepass_bc_reference as bref
import texture_build_reference as xref
from plainrenderer_amd import ImageDescription, ImageFormat, ImageType, MipCount, image_io

SIZES = [(1, 1), (2, 2), (3, 5), (5, 7), (1, 64), (16, 16), (130, 67)]  # (width, height)
FORMATS = {bref.BC1: ImageFormat.BC1, bref.BC3: ImageFormat.BC3, bref.BC5: ImageFormat.BC5}
U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pack(r, g, b, a):
    return (np.asarray(r, U32) | (np.asarray(g, U32) << U32(8)) | (np.asarray(b, U32) << U32(16)) | (np.asarray(a, U32) << U32(24))).astype(U32)


def inputs(width, height, seed=1):
    """name -> height x width words: seeded noise, a smooth gradient, two-colour blocks, blocks with anti-correlated channels (r rising while b falls), constant blocks"""
    rng = np.random.default_rng(seed + 1000 * width + height)
    y, x = np.mgrid[0:height, 0:width]
    noise = rng.integers(0, 2 ** 32, (height, width), dtype=np.uint64).astype(U32)
    gradient = pack((x * 255) // max(width - 1, 1), (y * 255) // max(height - 1, 1), ((x + y) * 255) // max(width + height - 2, 1), 255 - (x * 200) // max(width - 1, 1))
    colours = rng.integers(0, 2 ** 32, ((height + 3) // 4, (width + 3) // 4, 2), dtype=np.uint64).astype(U32)
    pick = rng.integers(0, 2, (height, width))
    two = colours[y // 4, x // 4, pick]
    ramp = ((x % 4) + 4 * (y % 4)) * 17
    anti = pack(ramp, (ramp * 3) // 4 + rng.integers(0, 8, (height, width)), 255 - ramp, 128 + ramp // 2)
    constant = rng.integers(0, 2 ** 32, ((height + 3) // 4, (width + 3) // 4), dtype=np.uint64).astype(U32)[y // 4, x // 4]
    return dict(noise=noise, gradient=gradient, two_colour=two, anti_correlated=anti, constant=constant)


def loop_chain(level0):
    """the chain rule as scalar loops: the second, independent statement"""
    levels = [[[int(v) for v in row] for row in level0]]
    while len(levels[-1]) > 1 or len(levels[-1][0]) > 1:
        src = levels[-1]
        h, w = len(src), len(src[0])
        dst = []
        for y in range(max(1, h >> 1)):
            row = []
            for x in range(max(1, w >> 1)):
                taps = [src[min(2 * y + j, h - 1)][min(2 * x + i, w - 1)] for j in (0, 1) for i in (0, 1)]
                word = 0
                for shift in (0, 8, 16, 24):
                    word |= ((sum((t >> shift) & 255 for t in taps) + 2) >> 2) << shift
                row.append(word)
            dst.append(row)
        levels.append(dst)
    return levels


@pytest.mark.parametrize("width,height", SIZES)
def test_the_reference_chain_equals_the_chain_written_as_loops(width, height):
    level0 = inputs(width, height)["noise"]
    got, want = xref.chain(level0), loop_chain(level0)
    assert len(got) == len(want) == max(width, height).bit_length()
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (max(1, height >> l), max(1, width >> l)) and g.tolist() == w, "level %d" % l


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("fmt", [bref.BC1, bref.BC3, bref.BC5], ids=["bc1", "bc3", "bc5"])
def test_the_host_encoder_equals_the_reference_byte_for_byte(fmt, width, height):
    for name, level in inputs(width, height).items():
        got = image_io.encode_rgba8_to_bc(FORMATS[fmt], width, height, level).tobytes()
        want = xref.encode_level(fmt, level)
        assert len(got) == image_io.bc_level_bytes(FORMATS[fmt], width, height)
        assert got == want, "%s %d x %d: %d bytes differ" % (name, width, height, sum(a != b for a, b in zip(got, want)))
        # ... and the two decoders agree on what it decodes to
        assert np.array_equal(image_io.decode_bc_to_rgba8(FORMATS[fmt], width, height, got), bref.decode_level(fmt, width, height, got))


def test_the_host_encoder_refuses_what_the_decoder_refuses():
    from plainrenderer_amd.backend import PlrError
    for call, words in ((lambda: image_io.encode_rgba8_to_bc(ImageFormat.RGBA8, 4, 4, np.zeros(16, U32)), ("not PLR_FORMAT_BC1",)),
                        (lambda: image_io.encode_rgba8_to_bc(ImageFormat.BC1, 0, 4, np.zeros(0, U32)), ("0 x 4",)),
                        (lambda: image_io.encode_rgba8_to_bc(ImageFormat.BC3, 16385, 1, np.zeros(16385, U32)), ("16385 x 1",))):
        with pytest.raises(PlrError) as e:
            call()
        assert all(w in str(e.value) for w in words), e.value


def _all_blocks():
    return np.concatenate([xref.gather(level) for width, height in SIZES for level in inputs(width, height).values()])


def test_a_constant_block_decodes_to_within_4_2_4():
    v = np.arange(256, dtype=U32)
    for r, g, b in ((v, v, v), (v, v[::-1], (v * 7) % 256)):
        t = np.repeat(pack(r, g, b, 255)[:, None], 16, axis=1)
        blocks = xref.encode_colour_blocks(t)
        assert not blocks[:, 4:].any(), "all indices are 0"
        for always_four in (False, True):
            d = bref.decode_colour_blocks(blocks, always_four).astype(np.int64)
            for c, (want, bound) in enumerate(((r, 4), (g, 2), (b, 4))):
                assert (np.abs(((d >> (8 * c)) & 255) - want.astype(np.int64)[:, None]) <= bound).all(), (always_four, c)


def test_an_alpha_block_with_at_most_two_values_decodes_exactly():
    rng = np.random.default_rng(5)
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    pick = rng.integers(0, 2, (a.size, 16))
    pick[:, 0], pick[:, 1] = 0, 1
    v = np.where(pick == 0, a.reshape(-1, 1), b.reshape(-1, 1))
    assert np.array_equal(bref.decode_alpha_blocks(xref.encode_alpha_blocks(v)), v)
    # BC5: both blocks
    t = pack(v[:4096], v[4096:8192], 0, 255)
    d = bref.decode_blocks(bref.BC5, xref.encode_blocks(bref.BC5, t))
    assert np.array_equal(d & U32(0xFFFF), t & U32(0xFFFF))


def test_every_decoded_alpha_is_within_the_proven_bound():
    """exhaustive over (min, max, v): 14 |d - v| <= R + 6, and the bound is met with equality somewhere (it is the proven one, not a loose one)"""
    worst = -10 ** 9
    hi, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for lo in range(255):
        use = (hi > lo) & (v >= lo) & (v <= hi)
        _, d = xref.alpha_choice(hi[use], np.full(int(use.sum()), lo), v[use])
        slack = 14 * np.abs(d - v[use]) - (hi[use] - lo)
        worst = max(worst, int(slack.max()))
    assert worst <= 6, worst
    assert worst == 6


def test_c0_is_never_below_c1_and_equal_endpoints_have_zero_indices():
    t = _all_blocks()
    blocks = xref.encode_colour_blocks(t).astype(np.int64)
    c0, c1 = blocks[:, 0] | (blocks[:, 1] << 8), blocks[:, 2] | (blocks[:, 3] << 8)
    assert (c0 >= c1).all() and (c0 > c1).any() and (c0 == c1).any()
    assert not blocks[c0 == c1, 4:].any()
    # so a BC1 block never decodes in three-colour mode with an index above 0: both decode variants agree on every encoded block
    assert np.array_equal(bref.decode_colour_blocks(blocks.astype(np.uint8), False), bref.decode_colour_blocks(blocks.astype(np.uint8), True))
    # the anti-correlated blocks put their high red with their low blue
    anti = xref.gather(inputs(16, 16)["anti_correlated"])
    e0, e1 = xref.colour_endpoints(anti)
    assert ((e0 >> 11) > (e1 >> 11)).all() and ((e0 & 31) < (e1 & 31)).all()


@pytest.mark.parametrize("fmt", [bref.BC1, bref.BC3, bref.BC5], ids=["bc1", "bc3", "bc5"])
def test_edge_positions_never_change_a_block(fmt):
    """the encode of a 5 x 7 level equals the encode of its edge-replicated 8 x 8"""
    for level in inputs(5, 7).values():
        padded = level[np.minimum(np.arange(8), 6)][:, np.minimum(np.arange(8), 4)]
        assert xref.encode_level(fmt, level) == xref.encode_level(fmt, padded)
        assert image_io.encode_rgba8_to_bc(FORMATS[fmt], 5, 7, level).tobytes() == image_io.encode_rgba8_to_bc(FORMATS[fmt], 8, 8, padded).tobytes()


def test_the_store_layout_pads_compressed_entries_and_keeps_level_0_verbatim():
    rgba = inputs(5, 3)["noise"]
    level0 = xref.encode_level(bref.BC3, inputs(8, 8)["gradient"])
    table, words, formats = xref.build_store([(rgba.reshape(-1), 5, 3, 0, bref.RGBA8, bref.RGBA8), (inputs(8, 8)["noise"].reshape(-1), 8, 8, 0, bref.RGBA8, bref.BC1),
                                              (level0, 8, 8, 0, bref.BC3, bref.BC3)])
    assert table.tolist() == [[0, 5, 3, 3], [20, 8, 8, 4], [36, 8, 8, 4]] and formats.tolist() == [bref.RGBA8, bref.BC1, bref.BC3]
    assert not words[18:20].any() and not words[34:36].any(), "15 + 2 + 1 words, then padding; 8 + 2 + 2 + 2 words, then padding"
    assert words[36:52].tobytes() == level0 and words.size == 36 + 16 + 12


@pytest.mark.parametrize("fmt", [bref.BC1, bref.BC3, bref.BC5], ids=["bc1", "bc3", "bc5"])
def test_dds_write_then_load_round_trips_a_compressed_chain(fmt, tmp_path):
    levels = xref.chain(inputs(16, 8)["gradient"])
    payload = b"".join(xref.encode_level(fmt, l) for l in levels)
    desc = ImageDescription(width=16, height=8, depth=1, type=ImageType.Type2D, format=FORMATS[fmt], usageFlags=1, mipCount=MipCount.Manual, manualMipCount=len(levels),
                            autoCreateMips=False)
    path = tmp_path / "chain.dds"
    image_io.write_dds_file(path, desc, np.frombuffer(payload, np.uint8))
    got, data = image_io.load_dds_file(path)
    assert (got.format, got.width, got.height, got.depth, got.manualMipCount) == (FORMATS[fmt], 16, 8, 1, len(levels))
    assert data.tobytes() == payload
    assert path.stat().st_size == 128 + len(payload), "the legacy header: no DX10 header behind it"
    first = image_io.bc_level_bytes(FORMATS[fmt], 16, 8)
    assert np.array_equal(image_io.decode_bc_to_rgba8(got.format, 16, 8, data[:first]), bref.decode_level(fmt, 16, 8, payload[:first]))


def test_the_host_layout_job_tables_and_encoder_run_clean_under_the_sanitizers(tmp_path):
    """tools/texture_build_check.cpp, a stand-alone program: the build's layout for every accepted pair at odd sizes, every job inside its buffers, the job tables
    executed on the host against the formatted packer fed the host-made levels, the refusals"""
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "texture_build_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "texture_build_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("texture build check: ok") and "0 words differ" in run.stdout, run.stdout + run.stderr


def test_the_entry_points_are_exported_and_the_structures_have_the_header_s_layout():
    from plainrenderer_amd import backend
    from plainrenderer_amd.frame import FramePipeline, PlrfSceneTextureSource, PlrfTextureBuildStats
    lib = backend._load()
    for name in ("plrf_build_scene_textures", "plrf_read_scene_texture_store", "plrf_get_texture_build_stats", "plr_encode_rgba8_to_bc"):
        assert getattr(lib, name) is not None
    assert C.sizeof(PlrfSceneTextureSource) == 40 and PlrfSceneTextureSource.format.offset == 28 and PlrfSceneTextureSource.store_format.offset == 32
    assert C.sizeof(PlrfTextureBuildStats) == 32 and PlrfTextureBuildStats.chain_texels.offset == 8
    assert all(hasattr(FramePipeline, n) for n in ("build_scene_textures", "read_scene_texture_store", "texture_build_stats"))
    from plainrenderer_amd import supported_shaders
    assert {"textureMipChain.comp", "textureBlockEncode.comp"} <= set(supported_shaders())
