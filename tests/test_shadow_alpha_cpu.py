"""The cutout reference (tests/shadow_alpha_reference.py) against the opaque reference where nothing is tested, the input conditions of the GPU cases
(tests/shadow_alpha_cases.py), the host's validation under a sanitizer, and the entry point at the C boundary; no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import shadow_alpha_cases as ac
import shadow_alpha_reference as aref
import shadow_raster_cases as sc
import test_shadow_raster as tsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("submitted", "drawn", "rejects")
OPAQUE_CASES = list(tsr.CASES)


@pytest.mark.parametrize("name", OPAQUE_CASES)
def test_with_all_cutoffs_zero_the_alpha_reference_is_the_opaque_reference(name):
    """on every case of the opaque pass' tests, texel for texel and counter for counter"""
    for case, _, r in tsr.reference(name):
        a = aref.rasterise(case, aref.opaque_inputs(case))
        assert np.array_equal(a["map"], r["map"]) and np.array_equal(a["coverage"], r["coverage"]), name
        assert all(a[c] == r[c] for c in COUNTERS) and a["tested"] == 0


def test_mesh_cases_with_all_cutoffs_zero_are_the_opaque_reference():
    """shadow_raster_cases.mesh_case under each light matrix, and a texture table that every draw names with cutoff 0"""
    lights = aref.ref.light_matrices(sc.mesh_scene()["info"])
    for c in range(3):
        case = sc.mesh_case(lights[c], 120)
        tex = aref.opaque_inputs(case)
        tex["materials"][:, 0] = 0
        a, r = aref.rasterise(case, tex), sc.rasterise(case)
        assert np.array_equal(a["map"], r["map"]) and all(a[k] == r[k] for k in COUNTERS) and a["tested"] == 0


def test_a_cutoff_word_above_255_is_256():
    assert aref.cutoff_codes([0, 1, 255, 256, 300, 0xFFFFFFFF]).tolist() == [0, 1, 255, 256, 256, 256]
    (case, tex, _, a, o, _), = ac.reference("cutout_over_opaque")
    maps = []
    for word in (256, 300, 0xFFFFFFFF):
        materials = tex["materials"].copy()
        materials[1, 1] = word
        maps.append(aref.rasterise(case, dict(tex, materials=materials))["map"])
    alone = sc.rasterise(ac.only(case, tex, 0)[0])["map"]
    assert all(np.array_equal(m, alone) for m in maps), "the card draws nothing: not what 255 does"
    materials = tex["materials"].copy()
    materials[1, 1] = 255
    assert not np.array_equal(aref.rasterise(case, dict(tex, materials=materials))["map"], alone)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test"""
    ac.check_case_is_what_it_is_for(name)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_every_case_differs_from_its_opaque_image_and_tests_both_ways(name):
    """what makes the GPU test fail on a launcher that ignores the third push-constant word, and what keeps it from passing vacuously"""
    for case, tex, _, a, o, _ in ac.reference(name):
        assert not np.array_equal(a["map"], o["map"]), "the opaque image is another one"
        assert [a[c] for c in COUNTERS] == [o[c] for c in COUNTERS], "the counters do not depend on alpha"
        assert 0 < a["passed"] < a["tested"], "tested fragments that pass and tested fragments that fail"


def test_the_host_validation_runs_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "shadow_cutout_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "shadow_cutout_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "shadow_cutout_check: ok", run.stdout + run.stderr


def test_the_shadow_cutout_entry_point_is_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_shadow_caster_cutouts") is not None
    from plainrenderer_amd.frame import FramePipeline, PlrfShadowCutout
    assert hasattr(FramePipeline, "set_shadow_caster_cutouts") and C.sizeof(PlrfShadowCutout) == 8
    with open(os.path.join(ROOT, "include", "plr_frame.h")) as fh:
        header = " ".join(fh.read().split())
    assert "typedef struct plrf_shadow_cutout { uint32_t albedo_texture, alpha_cutoff; } plrf_shadow_cutout;" in header
    assert ("int plrf_set_shadow_caster_cutouts(void* pipeline, const plrf_scene_texture* textures, uint32_t texture_count, const float* const* mesh_uvs, "
            "uint32_t mesh_count, const plrf_shadow_cutout* cutouts, uint32_t draw_count);") in header
