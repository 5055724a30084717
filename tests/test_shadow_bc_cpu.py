"""Block-compressed cutout textures of the shadow casters without a GPU: the format-aware reference (tests/shadow_bc_reference.py) against the cutout reference
(tests/shadow_alpha_reference.py) on the decoded store - the property the feature states, on the CPU -, the input conditions of the GPU cases
(tests/shadow_bc_cases.py), the host's validation and packing under a sanitizer, and the entry point at the C boundary."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepass_bc_reference as bc
import shadow_bc_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("submitted", "drawn", "rejects")


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_reference_equals_the_cutout_reference_on_the_decoded_store(name):
    """texel for texel and counter for counter; the decoded store is prepass_bc_reference.decode_store's: every usable row decoded block by block, a block that
    does not lie wholly inside `texels` as zeros, an unusable row as one"""
    for (case, tex, _, a, o, _), (flat, d) in zip(cases.reference(name), cases.decoded_reference(name)):
        assert "formats" not in flat and flat["texels"].size >= 1
        assert np.array_equal(a["map"], d["map"]), "%d texels differ" % int((a["map"] != d["map"]).sum())
        assert np.array_equal(a["coverage"], d["coverage"])
        assert [a[c] for c in COUNTERS] == [d[c] for c in COUNTERS]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test, among them: a BC3 entry in every case, a texel that differs from the all-opaque map, a texel that is covered"""
    cases.check_case_is_what_it_is_for(name)


def test_the_trilinear_case_has_a_record_whose_levels_differ():
    details = [t for run in cases.reference("alpha_mip_threshold") for t in run[5]]
    assert any(t["L1"] != t["L0"] and t["fw"] != 0 for t in details)
    assert all(t["format"] == bc.BC3 for t in details)


def test_both_alpha_modes_occur_among_the_sampled_blocks():
    modes = {m for run in cases.reference("alpha_modes") for t in run[5] for m in t["modes"]}
    assert modes == {"eight", "six"}
    everywhere = {m for name in cases.CASES for run in cases.reference(name) for t in run[5] for m in t["modes"]}
    assert everywhere == {"eight", "six"}


def test_the_host_validation_and_packing_run_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "shadow_cutout_bc_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "shadow_cutout_bc_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "shadow_cutout_bc_check: ok", run.stdout + run.stderr


def test_the_formatted_shadow_cutout_entry_point_is_exported():
    """fails on a library without the feature"""
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_shadow_caster_cutouts_formatted") is not None
    from plainrenderer_amd.frame import FramePipeline, PlrfSceneTextureData
    assert hasattr(FramePipeline, "set_shadow_caster_cutouts_formatted") and C.sizeof(PlrfSceneTextureData) == 32
    with open(os.path.join(ROOT, "include", "plr_frame.h")) as fh:
        header = " ".join(fh.read().split())
    assert ("int plrf_set_shadow_caster_cutouts_formatted(void* pipeline, const plrf_scene_texture_data* textures, uint32_t texture_count, const float* const* mesh_uvs, "
            "uint32_t mesh_count, const plrf_shadow_cutout* cutouts, uint32_t draw_count);") in header
