"""The cull contract of "drawCulling.comp" on the CPU (no GPU): tests/draw_culling_reference.py against the two raster references.

  conservativeness  for seeded random views of 257 draws per mode, every draw the cull reference drops, fed alone to tests/prepass_raster_reference.py or
                    tests/shadow_raster_reference.py, leaves a cleared image; the whole scene's images with the culled draw array equal those with the original;
                    the raster references given the culled array report `submitted` equal to the cull reference's visibleTriangles
  the case set      every named draw of tests/draw_culling_cases.py is what it is there for, every plane's counter is non-zero over the case set, the odd inputs
                    of the pass-level tests are kept
  the host          tools/draw_bounds_check.cpp runs clean under the address and undefined-behaviour sanitizers; the entry points are exported
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import draw_culling_cases as cc
import draw_culling_reference as ref
import prepass_raster_cases as pc
import shadow_raster_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = 5
PREPASS_IMAGES = ("depth", "motion", "normal", "albedo", "specular")
CONSERVATIVE_DRAWS = 257

EXPECTED_MAIN = dict(in_view=KEPT, culled_near=0, behind_camera=0, straddles_near=KEPT, contains_camera=KEPT, within_tolerance=KEPT, across_corner=KEPT, rotated_in=KEPT,
                     rotated_out=2, empty=KEPT, short=3, **{"culled_+x": 1, "culled_-x": 2, "culled_+y": 3, "culled_-y": 4, "straddles_+x": KEPT, "straddles_-x": KEPT,
                                                          "straddles_+y": KEPT, "straddles_-y": KEPT})
EXPECTED_SHADOW = dict(in_view=KEPT, around_map=KEPT, in_front_of_range=KEPT, behind_range=KEPT, within_tolerance=KEPT, across_corner=KEPT, rotated_in=KEPT, rotated_out=2,
                       empty=KEPT, short=3, **{"culled_+x": 1, "culled_-x": 2, "culled_+y": 3, "culled_-y": 4, "straddles_+x": KEPT, "straddles_-x": KEPT,
                                               "straddles_+y": KEPT, "straddles_-y": KEPT})


def _case(main, count):
    return cc.main_case(count) if main else cc.shadow_case(count)


def _rasterise(case, main, draws=None):
    c = case if draws is None else dict(case, draws=draws)
    return pc.rasterise(c) if main else sc.rasterise(c)


def _cleared(r, main):
    if main:
        return not any(np.asarray(r[k]).any() for k in PREPASS_IMAGES) and not r["coverage"].any()
    return not r["map"].any() and not r["coverage"].any()


@pytest.mark.parametrize("main", [True, False], ids=["main", "shadow"])
def test_named_draws_are_what_they_are_for(main):
    case = _case(main, max(cc.DRAW_COUNTS))
    r = cc.cull(case, main)
    expected = EXPECTED_MAIN if main else EXPECTED_SHADOW
    assert set(case["names"]) == set(expected)
    for name, plane in expected.items():
        assert int(r["plane"][case["names"][name]]) == plane, name
    # culled by that plane and by no earlier one: in float64, some corner is inside every earlier plane
    for plane, name in ((1, "culled_+x"), (2, "culled_-x"), (3, "culled_+y"), (4, "culled_-y")):
        d = case["names"][name]
        g, tol = cc.corner_g(case, main, d, plane)
        assert g.min() > 4.0 * tol
        for earlier in range(0 if main else 1, plane):
            assert cc.corner_g(case, main, d, earlier)[0].min() < 0.0, (name, earlier)
    # a straddling box has corners on both sides of its plane
    for plane, name in ((0, "straddles_near"), (1, "straddles_+x"), (2, "straddles_-x"), (3, "straddles_+y"), (4, "straddles_-y")):
        if name in case["names"]:
            g, _ = cc.corner_g(case, main, case["names"][name], plane)
            assert g.min() < 0.0 < g.max(), name
    # outside +x, by less than the tolerance: an exact test would drop it
    g, tol = cc.corner_g(case, main, case["names"]["within_tolerance"], 1)
    assert (g > 0.0).all() and g.max() < 0.75 * tol
    # across the corner: outside no single plane, yet nothing of it is in the view
    d = case["names"]["across_corner"]
    for plane in range(0 if main else 1, 5):
        assert cc.corner_g(case, main, d, plane)[0].min() < 0.0
    assert case["draws"][d, 1] == 36 and _cleared(_rasterise(case, main, case["draws"][d:d + 1]), main), "the known false positive draws nothing"
    if main:
        for name in ("behind_camera", "culled_near"):
            g, tol = cc.corner_g(case, True, case["names"][name], 0)
            assert g.min() > tol
        t = case["transforms"][case["draws"][case["names"]["behind_camera"], 3]]
        assert t[16 + 15] < -3.0, "the clip w of the model origin: behind the camera"
        lo, hi = case["bounds"][case["names"]["contains_camera"], :3], case["bounds"][case["names"]["contains_camera"], 3:]
        model = case["transforms"][case["draws"][case["names"]["contains_camera"], 3]][:16]
        local = np.linalg.solve(cc._math(model), np.array([0.0, 0.0, 0.0, 1.0]))[:3]  # the camera, at the world's origin, in the box's space
        assert (local > lo).all() and (local < hi).all(), "the camera lies inside the box"
    assert case["draws"][case["names"]["empty"], 1] == 0 and case["draws"][case["names"]["short"], 1] == 2
    # the rotated, non-uniformly scaled draw in view is drawn
    d = case["names"]["rotated_in"]
    assert not _cleared(_rasterise(case, main, case["draws"][d:d + 1]), main)


@pytest.mark.parametrize("main", [True, False], ids=["main", "shadow"])
def test_the_case_set_covers_every_plane_and_both_outcomes(main):
    for count in cc.DRAW_COUNTS:
        case = _case(main, count)
        r = cc.cull(case, main)
        assert case["draws"].shape[0] == count == case["bounds"].shape[0]
        assert int(r["stats"][0]) + int(r["stats"][2:].sum()) == count
        assert int(r["stats"][1]) == int((r["draws"][:, 1] // 3).sum())
        assert np.array_equal(np.delete(r["draws"], 1, axis=1), np.delete(case["draws"], 1, axis=1)), "only indexCount changes"
    stats = r["stats"]  # of the largest case
    planes = range(0 if main else 1, 5)
    for plane in planes:
        assert stats[2 + plane] > 0, "no draw of the case set is culled by plane %s" % ref.PLANES[plane]
    if not main:
        assert stats[2] == 0, "a shadow view has no near plane"
    assert 3 * int(stats[0]) >= count and 3 * int(stats[2:].sum()) >= count, "the reference keeps at least a third and culls at least a third"
    # wave and block edges carry both outcomes
    for edge in (63, 64, 256):
        assert len({int(p) == KEPT for p in r["plane"][edge - 2:edge + 2]}) == 2 or len({int(p) == KEPT for p in r["plane"][edge - 8:edge + 8]}) == 2


@pytest.mark.parametrize("main", [True, False], ids=["main", "shadow"])
def test_odd_inputs_are_kept(main):
    case = cc.with_odd_inputs(_case(main, 65), main)
    r = cc.cull(case, main)
    assert int(r["plane"][case["names"]["culled_+x"]]) == 1
    for name in cc.ODD_INPUTS:
        d = case["names"][name]
        assert int(r["plane"][d]) == KEPT and r["draws"][d, 1] == case["draws"][d, 1] == 36, name
    assert case["draws"][case["names"]["transform_out_of_range"], 3] == case["transforms"].shape[0]


def _views(main):
    """two seeded views per mode: the case's own, and one with the camera (the light) turned and moved and a sub-pixel jitter"""
    rng = np.random.default_rng(0x56494557 + (1 if main else 0))
    if main:
        moved = pc.camera(position=tuple(rng.uniform(-1.0, 1.0, 3)), forward=(float(rng.uniform(-0.3, 0.3)), float(rng.uniform(-0.2, 0.2)), 1.0), aspect=cc.WIDTH / cc.HEIGHT)
        jitter = tuple(float(v) for v in rng.uniform(-1.0, 1.0, 2) / np.array([cc.WIDTH, cc.HEIGHT]))
        return [cc.main_case(CONSERVATIVE_DRAWS), cc.main_case(CONSERVATIVE_DRAWS, cam=moved, jitter=jitter)]
    light = cc.model((1.0 / 17.0, 1.0 / 23.0, 1.0 / 50.0), float(rng.uniform(0.3, 0.8)), float(rng.uniform(-1.1, -0.7)), float(rng.uniform(-0.3, 0.3)), tuple(rng.uniform(-0.2, 0.2, 3)))
    return [cc.shadow_case(CONSERVATIVE_DRAWS), cc.shadow_case(CONSERVATIVE_DRAWS, light=light)]


@pytest.mark.parametrize("main", [True, False], ids=["main", "shadow"])
def test_a_culled_draw_has_no_fragment_and_the_images_do_not_change(main):
    for v, case in enumerate(_views(main)):
        r = cc.cull(case, main)
        dropped = np.flatnonzero(r["plane"] < KEPT)
        assert case["draws"].shape[0] >= 200 and dropped.size >= 50 and int(r["stats"][0]) >= 50
        for d in dropped:
            assert _cleared(_rasterise(case, main, case["draws"][d:d + 1]), main), "view %d: draw %d is culled by %s and has a fragment" % (v, d, ref.PLANES[int(r["plane"][d])])
        whole, culled = _rasterise(case, main), _rasterise(case, main, r["draws"])
        for image in (PREPASS_IMAGES if main else ("map",)):
            assert np.array_equal(whole[image], culled[image]), "view %d: %s changes under culling" % (v, image)
        assert (whole["depth"] if main else whole["map"]).any(), "the view shows something"
        assert culled["submitted"] == int(r["stats"][1]) < whole["submitted"], "submitted counts the kept draws' triangles"


def test_local_bounds_are_exact_minima_and_maxima():
    p = np.array([[-3, 2, 5], [1, -7, 0.5], [0.25, 9, -1], [4, 0, 6]], np.float32)
    assert ref.local_bounds(p).tolist() == [-3, -7, -1, 4, 9, 6] and ref.local_bounds(np.zeros((0, 3), np.float32)).tolist() == [0] * 6
    b = ref.draw_bounds([p, p[:1]], [1, 0, 0])
    assert b.shape == (3, 6) and b[0].tolist() == [-3, 2, 5, -3, 2, 5] and np.array_equal(b[1], b[2])


def test_the_host_packing_runs_clean_under_the_sanitizers(tmp_path):
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "draw_bounds_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "draw_bounds_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "draw_bounds_check: ok", run.stdout + run.stderr


def test_the_entry_points_are_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert getattr(lib, "plrf_set_draw_culling") is not None and getattr(lib, "plrf_get_draw_culling_stats") is not None
    from plainrenderer_amd.frame import CULL_SCENE, CULL_SHADOW_CASTERS, FramePipeline, PlrfDrawCullingStats
    assert hasattr(FramePipeline, "set_draw_culling") and hasattr(FramePipeline, "draw_culling_stats")
    assert (CULL_SCENE, CULL_SHADOW_CASTERS) == (1, 2) and C.sizeof(PlrfDrawCullingStats) == 48
