"""The tests' own texture sampler (tests/prepass_texture_reference.py) against hand-computed values, the input conditions of the GPU cases
(tests/prepass_texture_cases.py), the host's validation and mip builder under a sanitizer, and the entry point at the C boundary; no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepass_texture_cases as tc
import prepass_texture_reference as tref

F32 = np.float32
F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample(entry, texels, u, v, du_dx=0.0, dv_dx=0.0, du_dy=0.0, dv_dy=0.0, mip_bias=0.0):
    a = lambda x: np.array([x], F64)
    return int(tref.sample_texture(entry, np.asarray(texels, np.uint32), a(u), a(v), a(du_dx), a(dv_dx), a(du_dy), a(dv_dy), mip_bias)[0])


def test_a_uv_on_a_texel_centre_with_zero_derivative_gives_the_exact_texel():
    """u = (x + 0.5) / W: Tu = floor((x + 0.5 - 0.5) * 256 + 0.5) = 256 x, fx = 0; rho2 = 0, log2 = -inf, lod = 0"""
    texels = tc.pattern(4, 4, 3)
    for y in range(4):
        for x in range(4):
            assert _sample((0, 4, 4, 1), texels, (x + 0.5) / 4.0, (y + 0.5) / 4.0) == int(texels[4 * y + x])
            assert _sample((0, 4, 4, 1), texels, (x + 0.5) / 4.0 - 3.0, (y + 0.5) / 4.0 + 2.0) == int(texels[4 * y + x]), "repeat"
    assert _sample((0, 5, 3, 1), tc.pattern(5, 3, 4), 4.5 / 5.0, 2.5 / 3.0) == int(tc.pattern(5, 3, 4)[14])


def test_the_midpoint_of_a_2x2_block_gives_the_rounded_mean_and_a_tie_goes_to_even():
    """u = 1 / W: Tu = 128: x0 = 0, fx = 128: four weights of 128 * 128, S = 2^22 * 256 / 256 * sum ... code = sum / 4 rounded half to even"""
    def block(r00, r10, r01, r11):
        t = np.zeros(16, np.uint32)
        t[0], t[1], t[4], t[5] = r00, r10, r01, r11
        return t
    assert _sample((0, 4, 4, 1), block(10, 20, 30, 41), 0.25, 0.25) == 25, "101 / 4 = 25.25"
    assert _sample((0, 4, 4, 1), block(10, 20, 30, 43), 0.25, 0.25) == 26, "103 / 4 = 25.75"
    assert _sample((0, 4, 4, 1), block(10, 20, 30, 42), 0.25, 0.25) == 26, "102 / 4 = 25.5: the tie goes to the even code 26"
    assert _sample((0, 4, 4, 1), block(10, 20, 30, 38), 0.25, 0.25) == 24, "98 / 4 = 24.5: the tie goes to the even code 24"
    word = _sample((0, 4, 4, 1), block(0xFF0000FF, 0xFF0000FF, 0xFF0000FE, 0xFF0000FF), 0.25, 0.25)
    assert word == 0xFF0000FF, "255 stays 255 in alpha; (3 * 255 + 254) / 4 = 254.75 in red"
    # across the edge: u = 0 is the midpoint of texels W - 1 and 0
    t = np.zeros(16, np.uint32)
    t[0], t[3], t[12], t[15] = 8, 16, 24, 32
    assert _sample((0, 4, 4, 1), t, 0.0, 0.0) == 20 and _sample((0, 4, 4, 1), t, -1.0, 2.0) == 20


def test_four_texels_per_pixel_select_level_2_exactly():
    texels, width, height, mips = tc._level_texture()
    entry = (0, width, height, mips)
    assert _sample(entry, texels, 0.3, 0.6, du_dx=4.0 / 64.0, dv_dy=4.0 / 64.0) == tc.LEVEL_COLOURS[2]
    assert _sample(entry, texels, 0.3, 0.6, du_dx=4.0 / 64.0, dv_dy=1.0 / 64.0) == tc.LEVEL_COLOURS[2], "the larger footprint decides"
    assert _sample(entry, texels, 0.3, 0.6, du_dx=1.0 / 64.0, dv_dy=1.0 / 64.0) == tc.LEVEL_COLOURS[0]
    assert _sample(entry, texels, 0.3, 0.6, du_dx=4.0 / 64.0, dv_dy=4.0 / 64.0, mip_bias=1.0) == tc.LEVEL_COLOURS[3]
    assert _sample(entry, texels, 0.3, 0.6, du_dx=1e9, dv_dy=1e9) == tc.LEVEL_COLOURS[6], "clamped to the last level"
    assert _sample(entry, texels, 0.3, 0.6, du_dx=np.nan) == tc.LEVEL_COLOURS[0], "a NaN footprint is level 0"
    # half way between levels 2 and 3: lod = 2.5, fw = 128
    both = _sample(entry, texels, 0.3, 0.6, du_dx=4.0 / 64.0, dv_dy=4.0 / 64.0, mip_bias=0.5)
    for k in range(4):
        a, b = (tc.LEVEL_COLOURS[2] >> (8 * k)) & 255, (tc.LEVEL_COLOURS[3] >> (8 * k)) & 255
        assert (both >> (8 * k)) & 255 in ((a + b) // 2, (a + b + 1) // 2)


def test_the_mip_chain_rule_by_hand():
    """3 x 2 -> 1 x 1: columns min(0, 2) | min(1, 2), rows 0 | 1"""
    level0 = np.array([10, 20, 99, 30, 43, 99], np.uint32)
    chain = tref.build_chain(level0, 3, 2)
    assert chain.tolist() == [10, 20, 99, 30, 43, 99, (10 + 20 + 30 + 43 + 2) >> 2]
    assert tref.full_mip_count(3, 2) == 2 and tref.full_mip_count(16384, 1) == 15 and tref.full_mip_count(1, 1) == 1
    assert tref.build_chain(np.arange(16, dtype=np.uint32), 16, 1).size == 31


@pytest.mark.parametrize("name", list(tc.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test"""
    tc.check_case_is_what_it_is_for(name)


def test_the_host_validation_and_mip_builder_run_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "scene_texture_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "scene_texture_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "scene_texture_check: ok", run.stdout + run.stderr


def test_the_scene_texture_entry_point_is_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_scene_textures") is not None
    from plainrenderer_amd.frame import NO_TEXTURE, PlrfSceneMaterial, PlrfSceneTexture
    assert C.sizeof(PlrfSceneTexture) == 24 and C.sizeof(PlrfSceneMaterial) == 8 and NO_TEXTURE == 0xFFFFFFFF


def test_the_mesh_generators_return_uvs_only_when_asked():
    from plainrenderer_amd import meshes
    for make in (meshes.uv_sphere, meshes.box, meshes.torus):
        plain, with_uvs = make(), make(with_uvs=True)
        assert len(plain) == 2 and len(with_uvs) == 3
        assert np.array_equal(plain[0], with_uvs[0]) and np.array_equal(plain[1], with_uvs[1])
        uvs = with_uvs[2]
        assert uvs.dtype == np.float32 and uvs.shape == (plain[0].shape[0], 2) and uvs.min() >= 0.0 and uvs.max() <= 1.0 and np.unique(uvs, axis=0).shape[0] > 8
