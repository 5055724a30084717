"""The input conditions of the crowded-tile tests (tests/test_prepass_crowd.py) on the references alone, no GPU: every case of tests/prepass_crowd_cases.py and the
shadow crowd of tests/shadow_crowd_cases.py reaches what it is there for, the alpha reference agrees with itself when every triangle goes the per-triangle route,
and `queue_model` - a model of the scan's schedule that serves the case conditions only - is checked by hand on one quad and run over the most crowded case of
tests/prepass_alpha_cases.py.

References are computed once per process (the cases modules cache them) and shared by all tests and both math modes. Measured CPU times of one reference, on the
machine the cases were made on: one_wave 1.0 s (and 0.4 s for its model), formats_and_normals 1.0 s with the shading normal (0.7 s for its model), four_waves
1.3 s, the shadow crowd 0.3 s.
"""
import numpy as np
import pytest

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import prepass_crowd_cases as cc
import shadow_crowd_cases as scc

IMAGES = ("keys", "depth", "motion", "normal", "albedo", "specular")
COUNTERS = ("submitted", "clipped", "drawn", "rejects")


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_are_what_they_are_for(name):
    """the input conditions of the GPU test"""
    cc.check_case_is_what_it_is_for(name)


def test_shadow_crowd_is_what_it_is_for():
    scc.check_case_is_what_it_is_for()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_every_case_differs_from_its_untested_image_and_winners_reach_their_cutoff(name):
    r = cc.reference(name)
    a, o = r["a"], r["o"]
    assert not np.array_equal(a["depth"], o["depth"]) and not np.array_equal(a["albedo"], o["albedo"])
    assert [a[c] for c in COUNTERS] == [o[c] for c in COUNTERS], "the counters do not depend on alpha"
    own = aref.winner_draw(r["case"], a["keys"])
    assert ((a["albedo"][own >= 0] >> np.uint32(24)).astype(np.int64) >= aref.cutoff_codes(r["cutoffs"])[own[own >= 0]]).all()
    assert not a["albedo"][own < 0].any() and not a["normal"][own < 0].any()


def test_the_alpha_reference_agrees_with_itself_with_every_triangle_alone():
    """the opaque triangles of one_wave rasterised one by one, as the tested ones are: the same images and counters"""
    r = cc.reference("one_wave")
    alone = aref.render(r["case"], r["tex"], r["cutoffs"], every_triangle_alone=True)
    for image in IMAGES:
        assert np.array_equal(alone[image], r["a"][image]), image
    assert all(alone[c] == r["a"][c] for c in COUNTERS)
    assert len(alone["fragments"]) > len(r["a"]["fragments"])


def test_the_model_by_hand_on_one_quad():
    """an 8 x 8 tested quad on the stamp grid, everything passing: its two triangles are one stamp each and share the 64 pixels. The first push leaves fewer than
    64 pending, the second takes `pending` to exactly 64: one sample, no remainder, and nothing left for the flush"""
    from shadow_raster_cases import quad
    case = cc.pc.pixel_case([quad(0.0, 0.0, 8.0, 8.0, 0.5, 0.5)], 64, 64)
    case, tex = cc.tc.textured(case, cc.screen_uvs(case), [(0, cc.NONE)], cc.checker_textures())
    cutoffs = np.array([1], np.uint32)
    tex["texels"] = tex["texels"] | np.uint32(0xFF000000)
    a = aref.render(case, tex, cutoffs)
    m = cc.queue_model((case, tex, cutoffs), (a, cc.pc.rasterise(case, diagnostics=True)))
    assert np.array_equal(m["keys"], a["keys"]) and (a["keys"][:8, :8] != 0).all() and (a["keys"] != 0).sum() == 64
    assert (m["carries"], m["max_pending"], m["flushes"], m["dropped_queued"], m["dropped_sampled"]) == (0, 64, 0, 0, 0) and m["steps"] == [{("tested", "large")}]


def test_what_the_model_finds_in_the_most_crowded_alpha_case():
    """cutoff_values has the most tested triangles in one tile of all cases of tests/prepass_alpha_cases.py (16). The model is faithful there too, and finds one step
    per tile, no opaque, tested and discard-all records of both sizes side by side and no carry out of the lane path. It does find carries on the stamp path: one
    stamp of a 14 x 25 triangle pushes up to 64 candidates onto a queue that is not empty (measured: 16 carries, against 46 in one_wave)"""
    (case, tex, cutoffs, a, o), = ac.reference("cutoff_values")
    m = cc.queue_model((case, tex, cutoffs), (a, o))
    assert np.array_equal(m["keys"], a["keys"])
    assert len(m["steps"]) == 2 and m["flushes"] >= 1, "two tiles (70 x 50), one step each"
    assert m["lane_carries"] == 0 and not any(step == cc.SIX_KINDS for step in m["steps"]) and not any(size == "small" for step in m["steps"] for _, size in step)
    assert 0 < m["carries"] < 20
    crowded = cc.model_of("one_wave")
    assert crowded["carries"] >= 10 and crowded["lane_carries"] >= 1 and len(crowded["steps"]) >= 3
