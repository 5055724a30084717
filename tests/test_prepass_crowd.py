"""Crowded tiles through the alpha-tested "depthPrepassRaster.comp" and the cutout casters of "sunShadowRaster.comp", in both math modes, against
tests/prepass_alpha_reference.py and tests/shadow_alpha_reference.py: hundreds of records in one tile, so that the scan takes several steps of 64 hits, several
windows of 256 rectangles and all four waves, and its candidate queue carries remainders (tests/prepass_crowd_cases.py, tests/shadow_crowd_cases.py; the input
conditions: tests/test_prepass_crowd_cpu.py).

All five images (six with shadingNormal) and the four counters must be bit-identical to the reference, no pixel left out. Every execution is run twice and both
results must be the reference's: the waves race on the tile, and the image must not depend on which arrives first. The same inputs with alphaTest 0 (textureCount 0
for the shadow pass) must give the untested reference: the untested kernels on the same crowd.
"""
import struct

import numpy as np
import pytest

import prepass_alpha_reference as aref
import prepass_crowd_cases as cc
import prepass_normal_reference as nref
import shadow_crowd_cases as scc
import test_prepass_alpha as tpa
import test_prepass_bc as tpb
import test_prepass_raster as tpr
import test_shadow_alpha as tsa

TWICE = ("first", "second")


def _winners_reach_their_cutoff(r, out):
    """from the GPU images alone: a winner's stored alpha reaches its draw's cutoff"""
    own = aref.winner_draw(r["case"], r["a"]["keys"])
    won = out["depth"] != 0
    assert np.array_equal(won, own >= 0)
    assert ((out["albedo"][won] >> np.uint32(24)).astype(np.int64) >= aref.cutoff_codes(r["cutoffs"])[own[won]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", ["one_wave", "four_waves"])
def test_gpu_crowded_alpha_tested_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    cc.check_case_is_what_it_is_for(name)
    r = cc.reference(name)
    case, tex, cutoffs = r["case"], r["tex"], r["cutoffs"]
    backend.setMathMode(fast)
    try:
        for attempt in TWICE:
            out, counted = tpa.gpu_alpha(backend, case, tex, cutoffs)
            general = backend.getGeneralKernelExecutions()
            tpr.compare("crowd %s %s, %s" % (name, "fast" if fast else "exact", attempt), out, counted, r["a"])
            _winners_reach_their_cutoff(r, out)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
        counts = (case["draws"].shape[0], int((case["draws"][:, 1] // 3).sum()))
        out, counted = tpa.gpu_alpha(backend, case, tex, cutoffs, push=struct.pack("<4I", *counts, tex["texture_count"], 0))
        tpr.compare("crowd %s %s, alphaTest 0" % (name, "fast" if fast else "exact"), out, counted, r["o"])
    finally:
        backend.setMathMode(False)


FORMAT_RUNS = {"decoded": ("tex", False), "decoded_normals": ("tex", True), "formatted": ("store", False), "formatted_normals": ("store", True)}
_untested_shading_normal = {}


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("run", list(FORMAT_RUNS))
def test_gpu_crowded_alpha_tested_instantiations_agree_with_the_decoded_reference(backend, run, fast):
    """the four alpha-tested instantiations of the tile kernel - {RGBA8, formats} x {no normal maps, normal maps} - on formats_and_normals: the expected images of all
    four are the reference's for the store decoded to RGBA8"""
    cc.check_case_is_what_it_is_for("formats_and_normals")
    r = cc.reference("formats_and_normals")
    which, normals = FORMAT_RUNS[run]
    case, tex, cutoffs = r["case"], r[which], r["cutoffs"]
    nm, sn = (r["nm"], r["sn"]) if normals else (None, None)
    assert ("formats" in tex) == (which == "store")
    backend.setMathMode(fast)
    try:
        for attempt in TWICE:
            out, counted = tpb.gpu_bc(backend, case, tex, nm, cutoffs)
            general = backend.getGeneralKernelExecutions()
            tpb.compare_six("crowd %s %s, %s" % (run, "fast" if fast else "exact", attempt), out, counted, r["a"], sn)
            _winners_reach_their_cutoff(r, out)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
        if normals and "sn" not in _untested_shading_normal:
            _untested_shading_normal["sn"] = nref.shade(case, r["tex"], nm, r["o"]["keys"], r["o"]["normal"])
        out, counted = tpb.gpu_bc(backend, case, tex, nm, None)
        tpb.compare_six("crowd %s %s, alphaTest 0" % (run, "fast" if fast else "exact"), out, counted, r["o"], _untested_shading_normal["sn"] if normals else None)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_crowded_cutout_casters_are_bit_identical_to_the_reference(backend, fast):
    scc.check_case_is_what_it_is_for()
    case, tex, cascade, a, o = scc.reference()
    backend.setMathMode(fast)
    try:
        for attempt in TWICE:
            out, counters = tsa.gpu_cutouts(backend, case, tex, cascade)
            general = backend.getGeneralKernelExecutions()
            tsa.compare("shadow crowd %s, %s" % ("fast" if fast else "exact", attempt), out, counters, a)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
        triangles = int((case["draws"][:, 1] // 3).sum())
        out, counters = tsa.gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<3I", case["draws"].shape[0], triangles, 0))
        tsa.compare("shadow crowd %s, textureCount 0" % ("fast" if fast else "exact"), out, counters, o)
    finally:
        backend.setMathMode(False)
