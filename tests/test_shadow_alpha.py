"""Alpha-tested cutout casters of the "sunShadowRaster.comp" pass through the C-ABI against tests/shadow_alpha_reference.py, in both math modes: every texel of
the Depth16 map and the three counters must be bit-identical. The cases and what each is for: tests/shadow_alpha_cases.py.
A tile with 650 records from three set-up blocks: tests/shadow_crowd_cases.py, tests/test_prepass_crowd.py.

A record with the 8-byte push constants, or with textureCount 0, is the opaque pass whatever is bound at 6 - 9; with textureCount > 0 the launcher refuses a
missing or short binding 6 - 9, a scratch buffer of the opaque size and a scratch buffer that is also bound at 6 - 9, by name, and leaves the map as it was.
"""
import struct

import numpy as np
import pytest

import shadow_alpha_cases as ac
import shadow_alpha_reference as aref
import test_shadow_raster as tsr
from plainrenderer_amd.backend import spec_uint
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

UVS, MATERIALS, TEXTURES, TEXELS = 6, 7, 8, 9
JUNK = b"\x5a\xc3\x99\x17" * 24


def opaque_scratch_bytes(triangles):
    return 64 + 16 * ((triangles + 3) // 4) + 80 * triangles


def cutout_scratch_bytes(triangles):
    return 64 + 16 * ((triangles + 3) // 4) + 128 * triangles


def gpu_cutouts(be, case, tex, cascade, push=None, omit=(), sizes=None, scratch_as=None, scratch_bytes=None, junk=False, target=None):
    """one execution with the test's own buffers -> (map, (submitted, drawn, rejects)). push: the push constant bytes (default: the 12-byte record with the
    case's textureCount); omit: bindings of 6 - 9 left unbound; sizes: {binding: bytes} a buffer is cut to; scratch_as: the binding that gets the scratch buffer
    as well; junk: bindings 6 - 9 hold junk bytes; target: an image to draw into instead of a new one"""
    res = case["res"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    info = np.full(76, 7.25, np.float32)  # anything but the cascade's own matrix is garbage
    info[4 + 16 * cascade:4 + 16 * (cascade + 1)] = case["light"]
    arrays = [info, case["transforms"], case["positions"], case["indices"], case["draws"], None, tex["uvs"], tex["materials"], tex["textures"], tex["texels"]]
    buffers = {}
    for binding, a in enumerate(arrays):
        if binding in omit:
            continue
        if a is None:
            b = b"\xa5" * (cutout_scratch_bytes(triangles) if scratch_bytes is None else scratch_bytes)
        else:
            b = JUNK if junk and binding >= UVS else np.ascontiguousarray(a).tobytes() or b"\xa5" * 64
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
        struct.pack("<3I", case["draws"].shape[0], triangles, tex["texture_count"]) if push is None else push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = be.downloadImage(target, 0, np.uint16).reshape(res, res).copy()
    header = be.downloadStorageBuffer(buffers[5], 16, dtype=np.uint32)
    assert int(header[0]) == int(header[2]), "the cursor counts the drawn triangles"
    return out, (int(header[1]), int(header[2]), int(header[3]))


def compare(what, out, counters, r):
    differing = int((out != r["map"]).sum())
    print("%s: %d of %d texels differ, counters %r (reference %r)" % (what, differing, out.size, counters, (r["submitted"], r["drawn"], r["rejects"])))
    assert differing == 0, "%s: %d texels differ from the reference, first at %r" % (what, differing, tuple(np.argwhere(out != r["map"])[0]))
    assert counters == (r["submitted"], r["drawn"], r["rejects"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(ac.CASES))
def test_gpu_cutout_casters_are_bit_identical_to_the_reference(backend, name, fast):
    ac.check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, tex, cascade, a, o, _) in enumerate(ac.reference(name)):
            assert not np.array_equal(a["map"], o["map"]), "the opaque image is another one"
            assert 0 < a["passed"] < a["tested"]
            out, counters = gpu_cutouts(backend, case, tex, cascade)
            general = backend.getGeneralKernelExecutions()
            compare("cutouts %s[%d] %s" % (name, k, "fast" if fast else "exact"), out, counters, a)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_a_record_without_texture_count_is_the_pass_it_was(backend, fast):
    """the 8-byte push constants with bindings 6 - 9 unbound, bound and holding junk, and the 12-byte ones with textureCount 0 and junk bound; the scratch buffer
    has the opaque size"""
    backend.setMathMode(fast)
    try:
        for name in ("cutout_over_opaque", "paths"):
            for case, tex, cascade, a, o, _ in ac.reference(name):
                triangles = int((case["draws"][:, 1] // 3).sum())
                counts = (case["draws"].shape[0], triangles)
                small = opaque_scratch_bytes(triangles)
                want, counted = tsr.gpu_raster(backend, case, cascade)
                compare("%s through the opaque test's own record" % name, want, counted, o)
                out, counted = gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<2I", *counts), omit=(UVS, MATERIALS, TEXTURES, TEXELS), scratch_bytes=small)
                compare("%s, 8-byte push, 6 - 9 unbound" % name, out, counted, o)
                out, counted = gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<2I", *counts), scratch_bytes=small)
                compare("%s, 8-byte push, 6 - 9 bound" % name, out, counted, o)
                out, counted = gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<2I", *counts), junk=True, scratch_bytes=small)
                compare("%s, 8-byte push, junk at 6 - 9" % name, out, counted, o)
                out, counted = gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<3I", *counts, 0), junk=True, scratch_bytes=small)
                compare("%s, textureCount 0, junk at 6 - 9" % name, out, counted, o)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_all_cutoffs_zero_with_texture_count_set_is_the_opaque_image(backend):
    for name in ("stacked", "transformed"):
        (case, tex, cascade, a, o, _), = ac.reference(name)
        materials = tex["materials"].copy()
        materials[:, 1] = 0
        out, counted = gpu_cutouts(backend, case, dict(tex, materials=materials), cascade)
        compare("%s, textureCount %d, all cutoffs 0" % (name, tex["texture_count"]), out, counted, o)


@pytest.mark.gpu
def test_gpu_launcher_refuses_by_name_and_leaves_the_map_untouched(backend):
    from plainrenderer_amd.backend import PlrError
    (case, tex, cascade, a, o, _), = ac.reference("cutout_over_opaque")
    res = case["res"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    prefill = tsr.prefill_pattern(res)
    target = backend.createImage(image_desc_2d(res, res, ImageFormat.Depth16), prefill)
    names = {UVS: "uvs", MATERIALS: "casterMaterials", TEXTURES: "textures", TEXELS: "texels"}
    for binding, what in names.items():
        with pytest.raises(PlrError, match=r"missing storage buffer at binding %d \(sunShadowRaster %s" % (binding, what)):
            gpu_cutouts(backend, case, tex, cascade, omit=(binding,), target=target)
        with pytest.raises(PlrError, match=r"sunShadowRaster: the scratch buffer is also bound as an input \(binding %d\)" % binding):
            gpu_cutouts(backend, case, tex, cascade, omit=(binding,), scratch_as=binding, target=target)
    with pytest.raises(PlrError, match=r"sunShadowRaster casterMaterials.*binding 7 has 8 bytes, needs 16"):
        gpu_cutouts(backend, case, tex, cascade, sizes={MATERIALS: 8}, target=target)
    with pytest.raises(PlrError, match=r"sunShadowRaster textures.*binding 8 has 16 bytes, needs 32"):
        gpu_cutouts(backend, case, tex, cascade, push=struct.pack("<3I", case["draws"].shape[0], triangles, 2), target=target)
    with pytest.raises(PlrError, match=r"sunShadowRaster scratch of an execution with textureCount > 0.*binding 5 has %d bytes, needs %d"
                       % (opaque_scratch_bytes(triangles), cutout_scratch_bytes(triangles))):
        gpu_cutouts(backend, case, tex, cascade, scratch_bytes=opaque_scratch_bytes(triangles), target=target)
    assert np.array_equal(backend.downloadImage(target, 0, np.uint16).reshape(-1), prefill), "a refused execution writes nothing"
    out, counted = gpu_cutouts(backend, case, tex, cascade, target=target)
    compare("cutout_over_opaque after the refusals", out, counted, a)
