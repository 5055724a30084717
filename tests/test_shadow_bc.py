"""Block-compressed cutout textures of the "sunShadowRaster.comp" pass through the C-ABI against tests/shadow_bc_reference.py, in both math modes: every texel of
the Depth16 map and the three counters must be bit-identical, and identical to the same execution whose store holds the decoded RGBA8 levels under the 12-byte
push. The cases and what each is for: tests/shadow_bc_cases.py.

A record without the fourth push word, or with textureFormats 0, is the pass it was whatever is bound at 14; with textureFormats 1 the launcher refuses a missing
or short binding 14, the scratch buffer bound at 14 and textureCount 0, by name, and leaves the map as it was.
"""
import struct

import numpy as np
import pytest

import shadow_alpha_cases as ac
import shadow_bc_cases as cases
import test_shadow_alpha as tsa
import test_shadow_raster as tsr
from plainrenderer_amd.backend import spec_uint
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

FORMATS = 14
JUNK = tsa.JUNK


def gpu_formatted(be, case, tex, cascade, push=None, omit=(), sizes=None, scratch_as=None, formats=None, target=None):
    """one execution with the test's own buffers -> (map, (submitted, drawn, rejects)). push: the push constant bytes (default: the 16-byte record with the case's
    textureCount and textureFormats 1); omit: bindings left unbound; sizes: {binding: bytes} a buffer is cut to; scratch_as: the binding that gets the scratch
    buffer as well; formats: the bytes bound at 14 (default: the case's format codes); target: an image to draw into instead of a new one"""
    res = case["res"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    info = np.full(76, 7.25, np.float32)  # anything but the cascade's own matrix is garbage
    info[4 + 16 * cascade:4 + 16 * (cascade + 1)] = case["light"]
    arrays = {0: info, 1: case["transforms"], 2: case["positions"], 3: case["indices"], 4: case["draws"], 5: None, 6: tex["uvs"], 7: tex["materials"], 8: tex["textures"],
              9: tex["texels"], FORMATS: np.asarray(tex["formats"], np.uint32) if formats is None and "formats" in tex else formats}
    buffers = {}
    for binding, a in arrays.items():
        if binding in omit or (a is None and binding != 5):
            continue
        if a is None:
            b = b"\xa5" * tsa.cutout_scratch_bytes(triangles)  # the tested size: a format-aware execution's records are no larger
        else:
            b = (a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()) or b"\xa5" * 64
        if sizes and binding in sizes:
            b = b[:sizes[binding]]
        buffers[binding] = be.createStorageBuffer(len(b), b)
    if scratch_as is not None:
        buffers[scratch_as] = buffers[5]
    if target is None:
        target = be.createImage(image_desc_2d(res, res, ImageFormat.Depth16), tsr.prefill_pattern(res))
    p = be.createComputePass("sunShadowRaster.comp", [spec_uint(0, cascade)], "Sun shadow cascade %d" % cascade)
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(target, 0, 0)], storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]),
        struct.pack("<4I", case["draws"].shape[0], triangles, tex["texture_count"], 1) if push is None else push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = be.downloadImage(target, 0, np.uint16).reshape(res, res).copy()
    header = be.downloadStorageBuffer(buffers[5], 16, dtype=np.uint32)
    assert int(header[0]) == int(header[2]), "the cursor counts the drawn triangles"
    return out, (int(header[1]), int(header[2]), int(header[3]))


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_compressed_cutouts_equal_the_reference_and_the_decoded_store(backend, name, fast):
    cases.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, ((case, tex, cascade, a, o, _), (flat, d)) in enumerate(zip(cases.reference(name), cases.decoded_reference(name))):
            what = "%s[%d] %s" % (name, k, "fast" if fast else "exact")
            assert not np.array_equal(a["map"], o["map"]), "the opaque image is another one"
            out, counters = gpu_formatted(backend, case, tex, cascade)
            general = backend.getGeneralKernelExecutions()
            tsa.compare("compressed cutouts " + what, out, counters, a)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
            # the property: the same execution whose store holds the decoded levels, under the 12-byte push, gives the same bytes
            plain, plain_counters = tsa.gpu_cutouts(backend, case, flat, cascade)
            tsa.compare("decoded store " + what, plain, plain_counters, d)
            assert np.array_equal(out, plain) and counters == plain_counters, what
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_texture_formats_is_the_pass_it_was(backend, fast):
    """against the existing reference on the existing RGBA8 cases: the 12-byte push with binding 14 unbound and holding junk, the 16-byte push with textureFormats 0
    with binding 14 unbound and holding junk (a junk format code would make every entry unusable, were it read); and the opaque pass under its 8-byte push"""
    backend.setMathMode(fast)
    try:
        for name in ("cutout_over_opaque", "paths", "uv_edges"):
            for case, tex, cascade, a, o, _ in ac.reference(name):
                triangles = int((case["draws"][:, 1] // 3).sum())
                counts = (case["draws"].shape[0], triangles, tex["texture_count"])
                short, long = struct.pack("<3I", *counts), struct.pack("<4I", *counts, 0)
                for what, push, formats in (("12-byte push, 14 unbound", short, None), ("12-byte push, junk at 14", short, JUNK), ("textureFormats 0, 14 unbound", long, None),
                                            ("textureFormats 0, junk at 14", long, JUNK)):
                    out, counted = gpu_formatted(backend, case, tex, cascade, push=push, formats=formats)
                    tsa.compare("%s, %s" % (name, what), out, counted, a)
                out, counted = gpu_formatted(backend, case, tex, cascade, push=struct.pack("<2I", *counts[:2]), formats=JUNK)
                tsa.compare("%s, 8-byte push, junk at 14" % name, out, counted, o)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_launcher_refuses_by_name_and_leaves_the_map_untouched(backend, fast):
    from plainrenderer_amd.backend import PlrError
    (case, tex, cascade, a, o, _), = cases.reference("mixed_store")
    res = case["res"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    prefill = tsr.prefill_pattern(res)
    backend.setMathMode(fast)
    try:
        target = backend.createImage(image_desc_2d(res, res, ImageFormat.Depth16), prefill)
        with pytest.raises(PlrError, match=r"missing storage buffer at binding 14 \(sunShadowRaster textureFormats"):
            gpu_formatted(backend, case, tex, cascade, omit=(FORMATS,), target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster textureFormats.*binding 14 has 20 bytes, needs 24"):
            gpu_formatted(backend, case, tex, cascade, sizes={FORMATS: 20}, target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster: the scratch buffer is also bound as an input \(binding 14, textureFormats\)"):
            gpu_formatted(backend, case, tex, cascade, omit=(FORMATS,), scratch_as=FORMATS, target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster: textureFormats is set and textureCount is 0"):
            gpu_formatted(backend, case, tex, cascade, push=struct.pack("<4I", case["draws"].shape[0], triangles, 0, 1), target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster: textureFormats is 2, it must be 0 .* or 1"):
            gpu_formatted(backend, case, tex, cascade, push=struct.pack("<4I", case["draws"].shape[0], triangles, tex["texture_count"], 2), target=target)
        # what a tested execution refuses, it still refuses
        with pytest.raises(PlrError, match=r"missing storage buffer at binding 9 \(sunShadowRaster texels"):
            gpu_formatted(backend, case, tex, cascade, omit=(9,), target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster scratch of an execution with textureCount > 0.*binding 5 has %d bytes, needs %d"
                           % (tsa.opaque_scratch_bytes(triangles), tsa.cutout_scratch_bytes(triangles))):
            gpu_formatted(backend, case, tex, cascade, sizes={5: tsa.opaque_scratch_bytes(triangles)}, target=target)
        assert np.array_equal(backend.downloadImage(target, 0, np.uint16).reshape(-1), prefill), "a refused execution writes nothing"
        out, counted = gpu_formatted(backend, case, tex, cascade, target=target)
        tsa.compare("mixed_store after the refusals", out, counted, a)
    finally:
        backend.setMathMode(False)
