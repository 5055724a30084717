"""The alpha test's reference (tests/prepass_alpha_reference.py) against the textured reference where nothing is tested, the input conditions of the GPU cases
(tests/prepass_alpha_cases.py), the host's validation under a sanitizer, and the entry point at the C boundary; no GPU.
The input conditions of the crowded-tile cases (tests/prepass_crowd_cases.py): tests/test_prepass_crowd_cpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import prepass_texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = ("keys", "depth", "motion", "normal", "albedo", "specular")
COUNTERS = ("submitted", "clipped", "drawn", "rejects")


@pytest.mark.parametrize("name", list(tc.CASES))
def test_with_all_cutoffs_zero_the_alpha_reference_is_the_textured_reference(name):
    """on every case of the texture tests, the opaque route and, per triangle, the route a tested triangle takes"""
    for case, tex, r, s in tc.reference(name):
        zeros = np.zeros(case["draws"].shape[0], np.uint32)
        for alone in (False, True):
            a = aref.render(case, tex, zeros, every_triangle_alone=alone)
            want = dict(r, albedo=s["albedo"], specular=s["specular"])
            for image in IMAGES:
                assert np.array_equal(a[image], want[image]), (name, image, alone)
            assert all(a[c] == r[c] for c in COUNTERS)


def test_a_cutoff_word_above_255_is_256():
    assert aref.cutoff_codes([0, 1, 255, 256, 300, 0xFFFFFFFF]).tolist() == [0, 1, 255, 256, 256, 256]


@pytest.mark.parametrize("name", list(ac.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test"""
    ac.check_case_is_what_it_is_for(name)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_every_case_differs_from_its_opaque_image_and_winners_reach_their_cutoff(name):
    """what makes the GPU test fail on a launcher that ignores the fourth push-constant word; and the contract's consequence for the stored alpha"""
    for case, tex, cutoffs, a, o in ac.reference(name):
        assert not np.array_equal(a["depth"], o["depth"]) or not np.array_equal(a["albedo"], o["albedo"]), "(tie: equal depth, another winner)"
        assert [a[c] for c in COUNTERS] == [o[c] for c in COUNTERS], "the counters do not depend on alpha"
        own = aref.winner_draw(case, a["keys"])
        codes = aref.cutoff_codes(cutoffs)
        assert ((a["albedo"][own >= 0] >> np.uint32(24)).astype(np.int64) >= codes[own[own >= 0]]).all()
        assert not a["albedo"][own < 0].any() and not a["normal"][own < 0].any()


def test_the_host_validation_runs_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "scene_alpha_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "scene_alpha_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "scene_alpha_check: ok", run.stdout + run.stderr


def test_the_alpha_cutoff_entry_point_is_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_scene_alpha_cutoffs") is not None
    from plainrenderer_amd.frame import ALPHA_CUTOFF_REFERENCE, FramePipeline, PlrfSceneMaterial, PlrfSceneTexture
    assert ALPHA_CUTOFF_REFERENCE == 128 and hasattr(FramePipeline, "set_scene_alpha_cutoffs")
    assert C.sizeof(PlrfSceneTexture) == 24 and C.sizeof(PlrfSceneMaterial) == 8, "materials keeps its 8-byte stride"
    with open(os.path.join(ROOT, "include", "plr_frame.h")) as fh:
        header = fh.read()
    assert "#define PLRF_ALPHA_CUTOFF_REFERENCE 128u" in header
    assert "int plrf_set_scene_alpha_cutoffs(void* pipeline, const uint32_t* cutoffs, uint32_t draw_count);" in header
