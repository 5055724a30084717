"""Normal maps of the "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_normal_reference.py, in both math modes: every texel of shadingNormal
must be bit-identical to the reference, and the other five images and the four counters to the same record run without the fifth push-constant word. No pixel is
left out. The cases and what each is for: tests/prepass_normal_cases.py.

A record with a push of 16 bytes or fewer, or with normalMap 0, is the pass it was whatever is bound at 11 - 13 and at storage image 5, which it does not write;
with normalMap != 0 the launcher refuses a value other than 1 or 2, textureCount 0 and a missing, short or mis-formatted binding by name.
"""
import struct

import numpy as np
import pytest

import prepass_normal_cases as nc
import test_prepass_raster as tpr
import test_prepass_texture as tpt
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

ALPHA_CUTOFFS, TANGENTS, BITANGENTS, NORMAL_MATERIALS, SHADING_NORMAL = 10, 11, 12, 13, 5
SENTINEL_SALT = 17 * 5 + 3


def counts_of(case):
    return case["draws"].shape[0], int((case["draws"][:, 1] // 3).sum())


def gpu_normal(be, case, tex, nm, cutoffs=None, push=None, omit=(), sizes=None, shading_normal=(None, ImageFormat.RGBA8)):
    """one execution with the test's own buffers -> (the six images as uint32 h x w - shadingNormal None where it is not bound -, counters). push: the push
    constant bytes (default: the 20-byte record with the case's decode); omit: storage buffer bindings left unbound, SHADING_NORMAL + 100 for the image; sizes:
    {binding: bytes} a buffer is cut to; shading_normal: ((width, height) or None for the frame's, format) of storage image 5"""
    import passes
    w, h = case["width"], case["height"]
    draws, triangles = counts_of(case)
    passes.global_binding(be).set(tpt.globals_of(case, tex))
    arrays = [case["transforms"], case["positions"], case["normals"], case["indices"], case["draws"], None, tex["uvs"], tex["materials"], tex["textures"], tex["texels"],
              None if cutoffs is None else np.asarray(cutoffs, np.uint32), nm["tangents"], nm["bitangents"], nm["normal_materials"]]
    buffers = {}
    for binding, a in enumerate(arrays):
        if binding in omit or (a is None and binding != 5):
            continue
        b = b"\xa5" * tpr.scratch_bytes(triangles) if a is None else np.ascontiguousarray(a).tobytes()
        if sizes and binding in sizes:
            b = b[:sizes[binding]]
        buffers[binding] = be.createStorageBuffer(len(b), b)
    images = [be.createImage(image_desc_2d(w, h, fmt), tpr.prefill_pattern(w * h, 17 * k + 3)) for k, fmt in enumerate(tpr.FORMATS)]
    if SHADING_NORMAL + 100 not in omit:
        sw, sh = shading_normal[0] or (w, h)
        images.append(be.createImage(image_desc_2d(sw, sh, shading_normal[1]), tpr.prefill_pattern(sw * sh, SENTINEL_SALT)))
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]),
        struct.pack("<5I", draws, triangles, tex["texture_count"], 0 if cutoffs is None else 1, nm["decode"]) if push is None else push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(tpr.IMAGES, images)}
    out["shadingNormal"] = be.downloadImage(images[5], 0, np.uint32).reshape(h, w).copy() if len(images) > 5 and shading_normal[0] is None else None
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


def old_push(case, tex, cutoffs):
    draws, triangles = counts_of(case)
    return struct.pack("<4I", draws, triangles, tex["texture_count"], 0 if cutoffs is None else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", [n for n in nc.CASES if n not in nc.REFUSED_BY_THE_LAUNCHER])
def test_gpu_normal_mapped_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    nc.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, tex, nm, cutoffs, base, sn, details) in enumerate(nc.reference(name)):
            label = "normal %s[%d] %s" % (name, k, "fast" if fast else "exact")
            out, counted = gpu_normal(backend, case, tex, nm, cutoffs)
            general = backend.getGeneralKernelExecutions()
            differing = int((out["shadingNormal"] != sn).sum())
            print("prepass raster %-28s: shadingNormal texels that differ %d of %d" % (label, differing, sn.size))
            assert differing == 0, "shadingNormal: %d texels differ from the reference, first at %r" % (differing, tuple(np.argwhere(out["shadingNormal"] != sn)[0]))
            tpr.compare(label, out, counted, base)
            plain, plain_counted = gpu_normal(backend, case, tex, nm, cutoffs, push=old_push(case, tex, cutoffs))
            for image in tpr.IMAGES:
                assert np.array_equal(out[image], plain[image]), "%s depends on normalMap" % image
            assert counted == plain_counted
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_normal_map_is_the_pass_it_was_and_leaves_the_image_alone(backend, fast):
    """bindings 11 - 13 and storage image 5 bound: the 16-byte push constants, and the 20-byte ones with normalMap 0"""
    backend.setMathMode(fast)
    try:
        for name in ("material_mix", "with_alpha"):
            (case, tex, nm, cutoffs, base, sn, details), = nc.reference(name)
            sentinel = tpr.prefill_pattern(sn.size, SENTINEL_SALT).reshape(sn.shape)
            for label, push in (("16-byte push", old_push(case, tex, cutoffs)), ("normalMap 0", old_push(case, tex, cutoffs) + struct.pack("<I", 0))):
                out, counted = gpu_normal(backend, case, tex, nm, cutoffs, push=push)
                tpr.compare("%s, %s" % (name, label), out, counted, base)
                assert np.array_equal(out["shadingNormal"], sentinel), "%s, %s: shadingNormal was written" % (name, label)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_launcher_refuses_by_name_and_leaves_nothing_behind(backend):
    from plainrenderer_amd.backend import PlrError
    (case, tex, nm, cutoffs, base, sn, details), = nc.reference("material_mix")
    draws, triangles = counts_of(case)
    with pytest.raises(PlrError, match=r"depthPrepassRaster: normalMap is 3, it must be 0 \(none\), 1 \(the reference's decode\) or 2 \(the unit decode\)"):
        gpu_normal(backend, case, tex, nm, push=struct.pack("<5I", draws, triangles, tex["texture_count"], 0, 3))
    with pytest.raises(PlrError, match=r"depthPrepassRaster: normalMap is set and textureCount is 0"):
        gpu_normal(backend, case, tex, nm, push=struct.pack("<5I", draws, triangles, 0, 0, 1))
    for binding, word in ((TANGENTS, "tangents"), (BITANGENTS, "bitangents"), (NORMAL_MATERIALS, "normalMaterials")):
        with pytest.raises(PlrError, match=r"missing storage buffer at binding %d \(depthPrepassRaster %s" % (binding, word)):
            gpu_normal(backend, case, tex, nm, omit=(binding,))
    with pytest.raises(PlrError, match=r"missing storage image at binding 5 \(depthPrepassRaster shadingNormal"):
        gpu_normal(backend, case, tex, nm, omit=(SHADING_NORMAL + 100,))
    with pytest.raises(PlrError, match=r"depthPrepassRaster shadingNormal: storage binding 5 expects"):
        gpu_normal(backend, case, tex, nm, shading_normal=(None, ImageFormat.RG16_sNorm))
    with pytest.raises(PlrError, match=r"depthPrepassRaster: shadingNormal \(storage binding 5\) is 32 x 16, it must have the size of the other five: depth is 48 x 16"):
        gpu_normal(backend, case, tex, nm, shading_normal=((32, 16), ImageFormat.RGBA8))
    with pytest.raises(PlrError, match=r"depthPrepassRaster normalMaterials.*binding 13 has 8 bytes, needs 12"):
        gpu_normal(backend, case, tex, nm, sizes={NORMAL_MATERIALS: 8})
    # the hazard case: normalMaterials shorter than the draw count is refused rather than read
    (hcase, htex, hnm, _, _, _, _), = nc.reference("hazard_short_materials")
    with pytest.raises(PlrError, match=r"depthPrepassRaster normalMaterials.*binding 13 has 4 bytes, needs 8"):
        gpu_normal(backend, hcase, htex, hnm)
    # a refusal leaves nothing behind
    out, counted = gpu_normal(backend, case, tex, nm)
    assert np.array_equal(out["shadingNormal"], sn)
    tpr.compare("material_mix after the refusals", out, counted, base)
