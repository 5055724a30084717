"""The alpha test of the "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_alpha_reference.py, in both math modes: all five images and the
four counters must be bit-identical to the reference, and no pixel is left out. The cases and what each is for: tests/prepass_alpha_cases.py.
Tiles with hundreds of records (several steps, windows and waves of the scan): tests/prepass_crowd_cases.py, tests/test_prepass_crowd.py.

A record with the 8- or 12-byte push constants, or with alphaTest 0, is the pass without the test whatever is bound at 10; with alphaTest != 0 the launcher
refuses a missing or short binding 10, textureCount 0 and a scratch buffer that is also binding 10, by name.
"""
import struct

import numpy as np
import pytest

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import test_prepass_raster as tpr
import test_prepass_texture as tpt
from util import ComputePassExecution, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

ALPHA_CUTOFFS = 10


def gpu_alpha(be, case, tex, cutoffs, push=None, omit=(), sizes=None, scratch_as=None):
    """one execution with the test's own buffers -> (the five images as uint32 h x w, counters). push: the push constant bytes (default: the 16-byte record with
    alphaTest 1); omit: bindings of 6 - 10 left unbound; sizes: {binding: bytes} a buffer is cut to; scratch_as: the binding that gets the scratch buffer as well"""
    import passes
    w, h = case["width"], case["height"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    passes.global_binding(be).set(tpt.globals_of(case, tex))
    arrays = [case["transforms"], case["positions"], case["normals"], case["indices"], case["draws"], None, tex["uvs"], tex["materials"], tex["textures"], tex["texels"],
              np.asarray(cutoffs, np.uint32)]
    buffers = {}
    for binding, a in enumerate(arrays):
        if binding in omit:
            continue
        b = b"\xa5" * tpr.scratch_bytes(triangles) if a is None else np.ascontiguousarray(a).tobytes()
        if sizes and binding in sizes:
            b = b[:sizes[binding]]
        buffers[binding] = be.createStorageBuffer(len(b), b)
    if scratch_as is not None:
        buffers[scratch_as] = buffers[5]
    images = [be.createImage(image_desc_2d(w, h, fmt), tpr.prefill_pattern(w * h, 17 * k + 3)) for k, fmt in enumerate(tpr.FORMATS)]
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]),
        struct.pack("<4I", case["draws"].shape[0], triangles, tex["texture_count"], 1) if push is None else push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(tpr.IMAGES, images)}
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(ac.CASES))
def test_gpu_alpha_tested_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    ac.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, tex, cutoffs, a, o) in enumerate(ac.reference(name)):
            assert not np.array_equal(a["depth"], o["depth"]) or not np.array_equal(a["albedo"], o["albedo"]), "the opaque image is another one"
            out, counted = gpu_alpha(backend, case, tex, cutoffs)
            general = backend.getGeneralKernelExecutions()
            tpr.compare("alpha %s[%d] %s" % (name, k, "fast" if fast else "exact"), out, counted, a)
            # from the GPU images alone: a winner's stored alpha reaches its draw's cutoff
            own = aref.winner_draw(case, a["keys"])
            won = out["depth"] != 0
            assert np.array_equal(won, own >= 0)
            assert ((out["albedo"][won] >> np.uint32(24)).astype(np.int64) >= aref.cutoff_codes(cutoffs)[own[won]]).all()
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_alpha_test_is_the_pass_it_was(backend, fast):
    """the 8-byte push constants (untextured), the 12-byte ones and the 16-byte ones with alphaTest 0 (textured), each with binding 10 bound and unbound"""
    backend.setMathMode(fast)
    try:
        for name in ("cutout_over_opaque", "cutoff_values"):
            (case, tex, cutoffs, a, o), = ac.reference(name)
            counts = (case["draws"].shape[0], int((case["draws"][:, 1] // 3).sum()))
            untextured = tpr.pc.rasterise(case)
            for omit in ((), (ALPHA_CUTOFFS,)):
                bound = "binding 10 %s" % ("unbound" if omit else "bound")
                out, counted = gpu_alpha(backend, case, tex, cutoffs, push=struct.pack("<2I", *counts), omit=omit)
                tpr.compare("%s, 8-byte push, %s" % (name, bound), out, counted, untextured)
                out, counted = gpu_alpha(backend, case, tex, cutoffs, push=struct.pack("<3I", *counts, tex["texture_count"]), omit=omit)
                tpr.compare("%s, 12-byte push, %s" % (name, bound), out, counted, o)
                out, counted = gpu_alpha(backend, case, tex, cutoffs, push=struct.pack("<4I", *counts, tex["texture_count"], 0), omit=omit)
                tpr.compare("%s, alphaTest 0, %s" % (name, bound), out, counted, o)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_all_cutoffs_zero_with_alpha_test_set_is_the_textured_pass(backend):
    (case, tex, cutoffs, a, o), = ac.reference("stacked")
    out, counted = gpu_alpha(backend, case, tex, np.zeros_like(cutoffs))
    tpr.compare("stacked, alphaTest 1, all cutoffs 0", out, counted, o)


@pytest.mark.gpu
def test_gpu_launcher_refuses_by_name_and_leaves_nothing_behind(backend):
    from plainrenderer_amd.backend import PlrError
    (case, tex, cutoffs, a, o), = ac.reference("cutout_over_opaque")
    counts = (case["draws"].shape[0], int((case["draws"][:, 1] // 3).sum()))
    with pytest.raises(PlrError, match=r"missing storage buffer at binding 10 \(depthPrepassRaster alphaCutoffs"):
        gpu_alpha(backend, case, tex, cutoffs, omit=(ALPHA_CUTOFFS,))
    with pytest.raises(PlrError, match=r"depthPrepassRaster alphaCutoffs.*binding 10 has 4 bytes, needs 8"):
        gpu_alpha(backend, case, tex, cutoffs, sizes={ALPHA_CUTOFFS: 4})
    with pytest.raises(PlrError, match=r"depthPrepassRaster: alphaTest is set and textureCount is 0"):
        gpu_alpha(backend, case, tex, cutoffs, push=struct.pack("<4I", *counts, 0, 1))
    with pytest.raises(PlrError, match=r"depthPrepassRaster: the scratch buffer is also bound as an input \(binding 10"):
        gpu_alpha(backend, case, tex, cutoffs, omit=(ALPHA_CUTOFFS,), scratch_as=ALPHA_CUTOFFS)
    out, counted = gpu_alpha(backend, case, tex, cutoffs)
    tpr.compare("cutout_over_opaque after the refusals", out, counted, a)
