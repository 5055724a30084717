"""Block-compressed textures of the "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_bc_reference.py, in both math modes: all six images
(shadingNormal where the case has a normal map) and the four counters must be bit-identical to the reference, and no pixel is left out. The cases and what each
is for: tests/prepass_bc_cases.py. For every case that is no hazard the same scene with the store decoded to RGBA8 on the host and the old push constants must
give the same bytes.

A record with a push of 20 bytes or fewer, or with textureFormats 0, is the pass it was whatever is bound at 14; with textureFormats != 0 the launcher refuses a
value other than 1, textureCount 0, a missing or short binding 14 and a scratch buffer that is also binding 14, by name.
"""
import struct

import numpy as np
import pytest

import prepass_bc_cases as bc
import test_prepass_normal as tpn
import test_prepass_raster as tpr
import test_prepass_texture as tpt
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

TEXTURE_FORMATS = 14


def push_of(case, tex, nm, cutoffs, words=6, formats=1):
    draws, triangles = tpn.counts_of(case)
    return struct.pack("<6I", draws, triangles, tex["texture_count"], 0 if cutoffs is None else 1, 0 if nm is None else nm["decode"], formats)[:4 * words]


def gpu_bc(be, case, tex, nm=None, cutoffs=None, push=None, omit=(), sizes=None, scratch_as=None):
    """one execution with the test's own buffers -> (the six images as uint32 h x w - shadingNormal None without normal inputs -, counters). tex: a mixed store
    (`formats` goes to binding 14) or an all-RGBA8 one (nothing is bound there). push: the push constant bytes (default: the 24-byte record with textureFormats 1
    for a mixed store, the 20-byte one otherwise); omit: storage buffer bindings left unbound; sizes: {binding: bytes} a buffer is cut to; scratch_as: the binding
    that gets the scratch buffer as well"""
    import passes
    w, h = case["width"], case["height"]
    draws, triangles = tpn.counts_of(case)
    passes.global_binding(be).set(tpt.globals_of(case, tex))
    arrays = {0: case["transforms"], 1: case["positions"], 2: case["normals"], 3: case["indices"], 4: case["draws"], 5: None, 6: tex["uvs"], 7: tex["materials"],
              8: tex["textures"], 9: tex["texels"]}
    if cutoffs is not None:
        arrays[tpn.ALPHA_CUTOFFS] = np.asarray(cutoffs, np.uint32)
    if nm is not None:
        arrays.update({tpn.TANGENTS: nm["tangents"], tpn.BITANGENTS: nm["bitangents"], tpn.NORMAL_MATERIALS: nm["normal_materials"]})
    if "formats" in tex:
        arrays[TEXTURE_FORMATS] = np.asarray(tex["formats"], np.uint32)
    buffers = {}
    for binding, a in arrays.items():
        if binding in omit:
            continue
        b = b"\xa5" * tpr.scratch_bytes(triangles) if a is None else np.ascontiguousarray(a).tobytes()
        if sizes and binding in sizes:
            b = b[:sizes[binding]]
        buffers[binding] = be.createStorageBuffer(max(len(b), 4), b if b else b"\0" * 4)
    if scratch_as is not None:
        buffers[scratch_as] = buffers[5]
    images = [be.createImage(image_desc_2d(w, h, fmt), tpr.prefill_pattern(w * h, 17 * k + 3)) for k, fmt in enumerate(tpr.FORMATS)]
    if nm is not None:
        images.append(be.createImage(image_desc_2d(w, h, ImageFormat.RGBA8), tpr.prefill_pattern(w * h, tpn.SENTINEL_SALT)))
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    if push is None:
        push = push_of(case, tex, nm, cutoffs) if "formats" in tex else push_of(case, tex, nm, cutoffs, words=5)
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]), push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(tpr.IMAGES, images)}
    out["shadingNormal"] = be.downloadImage(images[5], 0, np.uint32).reshape(h, w).copy() if nm is not None else None
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


def compare_six(label, out, counted, base, sn):
    tpr.compare(label, out, counted, base)
    if sn is not None:
        differing = int((out["shadingNormal"] != sn).sum())
        print("prepass raster %-28s: shadingNormal texels that differ %d of %d" % (label, differing, sn.size))
        assert differing == 0, "shadingNormal: %d texels differ from the reference, first at %r" % (differing, tuple(np.argwhere(out["shadingNormal"] != sn)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_gpu_block_compressed_prepass_is_bit_identical_to_the_reference(backend, name, fast):
    bc.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, tex, nm, cutoffs, decoded, base, sn) in enumerate(bc.reference(name)):
            label = "bc %s[%d] %s" % (name, k, "fast" if fast else "exact")
            out, counted = gpu_bc(backend, case, tex, nm, cutoffs)
            general = backend.getGeneralKernelExecutions()
            compare_six(label, out, counted, base, sn)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
            if name in bc.HAZARDS:
                continue
            # the store decoded on the host, as RGBA8 under the old push constants: the same bytes
            plain, plain_counted = gpu_bc(backend, case, decoded, nm, cutoffs)
            for image in tpr.IMAGES + (("shadingNormal",) if nm is not None else ()):
                assert np.array_equal(out[image], plain[image]), "%s: %s differs from the pre-decoded RGBA8 store's" % (label, image)
            assert counted == plain_counted
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_texture_formats_is_the_pass_it_was(backend, fast):
    """an all-RGBA8 store with binding 14 bound (to codes that would change the image): the 20-byte push constants, and the 24-byte ones with textureFormats 0, give
    the same bytes as the 20-byte record with nothing bound at 14; and the 24-byte record with textureFormats 1 and codes 0 gives them too"""
    backend.setMathMode(fast)
    try:
        for name in ("mixed", "normal_bc5", "alpha_holes"):
            case, tex, nm, cutoffs, decoded, base, sn = bc.reference(name)[0]
            rows = decoded["textures"].shape[0]
            want, want_counted = gpu_bc(backend, case, decoded, nm, cutoffs)
            compare_six("%s decoded" % name, want, want_counted, base, sn)
            bound = dict(decoded, formats=np.full(rows, bc.BC3, np.uint32))
            for label, push in (("20-byte push", push_of(case, decoded, nm, cutoffs, words=5)), ("textureFormats 0", push_of(case, decoded, nm, cutoffs, formats=0))):
                out, counted = gpu_bc(backend, case, bound, nm, cutoffs, push=push)
                for image in want:
                    assert want[image] is None or out[image].tobytes() == want[image].tobytes(), "%s, %s: %s" % (name, label, image)
                assert counted == want_counted
            out, counted = gpu_bc(backend, case, dict(decoded, formats=np.zeros(rows, np.uint32)), nm, cutoffs)
            compare_six("%s, codes 0 under textureFormats 1" % name, out, counted, base, sn)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_launcher_refuses_by_name_and_leaves_nothing_behind(backend):
    from plainrenderer_amd.backend import PlrError
    (case, tex, nm, cutoffs, decoded, base, sn), = bc.reference("mixed")
    with pytest.raises(PlrError, match=r"depthPrepassRaster: textureFormats is 2, it must be 0 \(every texture is RGBA8\) or 1"):
        gpu_bc(backend, case, tex, push=push_of(case, tex, None, None, formats=2))
    with pytest.raises(PlrError, match=r"depthPrepassRaster: textureFormats is set and textureCount is 0"):
        gpu_bc(backend, case, tex, push=struct.pack("<6I", *tpn.counts_of(case), 0, 0, 0, 1))
    with pytest.raises(PlrError, match=r"missing storage buffer at binding 14 \(depthPrepassRaster textureFormats"):
        gpu_bc(backend, case, tex, omit=(TEXTURE_FORMATS,))
    with pytest.raises(PlrError, match=r"depthPrepassRaster textureFormats.*binding 14 has 12 bytes, needs 16"):
        gpu_bc(backend, case, tex, sizes={TEXTURE_FORMATS: 12})
    with pytest.raises(PlrError, match=r"depthPrepassRaster: the scratch buffer is also bound as an input \(binding 14, textureFormats\)"):
        gpu_bc(backend, case, tex, scratch_as=TEXTURE_FORMATS)
    # a refusal leaves nothing behind
    out, counted = gpu_bc(backend, case, tex)
    compare_six("mixed after the refusals", out, counted, base, sn)
