"""Material texture sampling of the "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_texture_reference.py, in both math modes: every texel
of albedo and specular must be bit-identical to the reference's sample, and depth, motion, normal and the four counters to the untextured reference of the same
record (tests/prepass_raster_reference.py). No pixel is left out. The cases and what each is for: tests/prepass_texture_cases.py.

A record with the 8-byte push constants, or with textureCount 0, is the untextured pass whatever is bound at 6 - 9; with textureCount > 0 the launcher refuses a
missing or short binding 6 - 9 by name.
"""
import struct

import numpy as np
import pytest

import prepass_texture_cases as tc
import test_prepass_raster as tpr
from util import ComputePassExecution, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

F32 = np.float32
UVS, MATERIALS, TEXTURES, TEXELS = 6, 7, 8, 9


def globals_of(case, tex):
    g = np.frombuffer(tpr.globals_with_jitter(case), F32).copy()
    g[79] = tex["mip_bias"]  # offset 316 of the 340-byte global block: mipBias
    return g.tobytes()


def gpu_textured(be, case, tex, push=None, omit=(), sizes=None):
    """one execution with the test's own buffers -> (the five images as uint32 h x w, counters). push: the push constant bytes (default: the 12-byte record);
    omit: bindings of 6 - 9 left unbound; sizes: {binding: bytes} a buffer is cut to"""
    import passes
    w, h = case["width"], case["height"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    passes.global_binding(be).set(globals_of(case, tex))
    arrays = [case["transforms"], case["positions"], case["normals"], case["indices"], case["draws"], None, tex["uvs"], tex["materials"], tex["textures"], tex["texels"]]
    buffers = {}
    for binding, a in enumerate(arrays):
        if binding in omit:
            continue
        b = b"\xa5" * tpr.scratch_bytes(triangles) if a is None else np.ascontiguousarray(a).tobytes()
        if sizes and binding in sizes:
            b = b[:sizes[binding]]
        buffers[binding] = be.createStorageBuffer(len(b), b)
    images = [be.createImage(image_desc_2d(w, h, fmt), tpr.prefill_pattern(w * h, 17 * k + 3)) for k, fmt in enumerate(tpr.FORMATS)]
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]),
        struct.pack("<3I", case["draws"].shape[0], triangles, tex["texture_count"]) if push is None else push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(tpr.IMAGES, images)}
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


def textured_reference(r, s):
    """the untextured reference with the sampled albedo and specular"""
    return dict(r, albedo=s["albedo"], specular=s["specular"])


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_gpu_textured_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    tc.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, tex, r, s) in enumerate(tc.reference(name)):
            out, counted = gpu_textured(backend, case, tex)
            general = backend.getGeneralKernelExecutions()
            tpr.compare("textured %s[%d] %s" % (name, k, "fast" if fast else "exact"), out, counted, textured_reference(r, s))
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_texture_count_is_the_untextured_pass(backend, fast):
    """bindings 6 - 9 bound both times: the 8-byte push constants, and the 12-byte ones with textureCount 0; and with 6 - 9 unbound as well"""
    backend.setMathMode(fast)
    try:
        for name in ("material_mix", "ragged"):
            (case, tex, r, s), = tc.reference(name)
            assert not np.array_equal(s["albedo"], r["albedo"]) and not np.array_equal(s["specular"], r["specular"]), "textures would show"
            counts = (case["draws"].shape[0], int((case["draws"][:, 1] // 3).sum()))
            for label, push, omit in (("8-byte push", struct.pack("<2I", *counts), ()), ("textureCount 0", struct.pack("<3I", *counts, 0), ()),
                                      ("textureCount 0, nothing bound", struct.pack("<3I", *counts, 0), (UVS, MATERIALS, TEXTURES, TEXELS))):
                out, counted = gpu_textured(backend, case, tex, push=push, omit=omit)
                tpr.compare("%s, %s" % (name, label), out, counted, r)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_launcher_refuses_a_missing_or_short_texture_binding(backend):
    from plainrenderer_amd.backend import PlrError
    (case, tex, r, s), = tc.reference("material_mix")
    for binding, word in ((UVS, "uvs"), (MATERIALS, "materials"), (TEXTURES, "textures"), (TEXELS, "texels")):
        with pytest.raises(PlrError, match=r"missing storage buffer at binding %d \(depthPrepassRaster %s" % (binding, word)):
            gpu_textured(backend, case, tex, omit=(binding,))
    with pytest.raises(PlrError, match=r"depthPrepassRaster materials.*binding 7 has 16 bytes, needs 24"):
        gpu_textured(backend, case, tex, sizes={MATERIALS: 16})
    with pytest.raises(PlrError, match=r"depthPrepassRaster textures.*binding 8 has 16 bytes, needs 32"):
        gpu_textured(backend, case, tex, sizes={TEXTURES: 16})
    # a refusal leaves nothing behind
    out, counted = gpu_textured(backend, case, tex)
    tpr.compare("material_mix after the refusals", out, counted, textured_reference(r, s))
