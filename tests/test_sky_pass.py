"""The "skyAndSunSprite.comp" pass through the C-ABI against tests/sky_reference.py, in both math modes.

The colour buffer is pre-filled with a bit pattern (the pass must leave geometry pixels alone and may not read the buffer), the depth has 8 x 8 blocks
of sky and geometry with rows 0 - 3 all geometry, the froxel volume is random RGBA16F with maxDistance = 70 (depth 30 lies between slices 5 and 6 of 8).
Cases, the smallest that reach every way the kernels can go wrong:
  disc200    200 x 120, vertical fov 4 degrees: the disc is 16 pixels wide and straddles x = 64 - a wave boundary of the general kernel's 64 x 4 blocks and an
             edge between a sky and a geometry block; 200 = 3 x 64 + 8 is ragged for the 64-wide blocks and one partial 256-wide tile row for the fast kernel
  corner67   67 x 35 at the same pixel scale, all sky (odd pitch: no 16-byte rows, texel-by-texel loads and stores), the disc's centre half a radius outside the frame corner
  pixel96    96 x 54, fov 90 degrees: the disc is a quarter of a pixel wide and centred on one pixel centre
  behind96   the same frame with the sun behind the camera: no disc anywhere
For each case the test first asserts, on the reference, that no pixel centre lies within 1e-3 of the disc's rim in d2 - a condition on the inputs that
makes disc membership the same decision on both sides; then geometry pixels must equal the pre-fill bit for bit and every sky pixel must be within one
R11G11B10 code per channel of the reference (README: "one R11G11B10 code wherever their discrete decisions agree"). The share of sky pixels that are not
bit-identical is printed and appended to the file PLR_SKY_PASS_REPORT names, if set.
"""
import math
import os
import struct

import numpy as np
import pytest

import sky_reference as sr
from passes import global_binding
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.backend import ImageDescription, ImageType, ImageUsageFlags
from plainrenderer_amd.scene import Camera, GlobalShaderInfo
from util import (ComputePassExecution, ImageFormat, ImageResource, MipCount, RenderPassResources, StorageBufferResource, UniformBufferResource, image_desc_2d)

F = ImageFormat
MAX_DISTANCE = 70.0
LIGHT = struct.pack("<5f", 1.0, 0.9, 0.8, 1e-4, 12.8)
FROXEL_DEPTH = 8

# name: (w, h, fov, aim in pixel coordinates of the disc centre (None: behind the camera), all sky, time)
CASES = {
    "disc200": (200, 120, 4.0, (64.3, 43.7), False, 13.37),
    # the pixel scale of disc200 (4 degrees over 120 rows); aim filled in below: half a disc radius outside corner (0, 0), on the diagonal
    "corner67": (67, 35, 4.0 * 35 / 120, None, True, 0.0),
    "pixel96": (96, 54, 90.0, (48.5, 20.5), False, 0.75),
    "behind96": (96, 54, 90.0, None, False, 0.75),
}


def _camera(w, h, fov):
    return Camera.look((1.0, 2.0, 3.0), (0.3, -0.5, 0.8), fov=fov, aspect=w / h)


def build_case(name):
    w, h, fov, aim, all_sky, time = CASES[name]
    cam = _camera(w, h, fov)
    if name == "corner67":
        radius_px = float(sr.SUN_SPRITE_SCALE) / (2.0 * cam.tan_fov_half() / h)
        aim = (-0.5 * radius_px / math.sqrt(2.0), -0.5 * radius_px / math.sqrt(2.0))
    sun = sr.aim_ray(cam, w, h, *aim) if aim is not None else -np.asarray(cam.forward, np.float64)
    g = cam.fill_global(GlobalShaderInfo(), w, h)
    g.sunDirection = (*[float(x) for x in sun.astype(np.float32)], 0.0)
    g.time = time
    rng = np.random.default_rng(0x534B59 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if all_sky:
        depth = np.zeros((h, w), np.float32)
    else:
        geometry = (((xx // 8) + (yy // 8)) % 2 == 1) | (yy < 4)
        depth = np.where(geometry, rng.uniform(0.05, 0.9, (h, w)), 0.0).astype(np.float32)
    prefill = ((np.arange(w * h, dtype=np.uint64) * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF).astype(np.uint32).reshape(h, w)
    vw, vh = (w + 7) // 8, (h + 7) // 8
    volume = pixfmt.pack_half(rng.uniform(0.0, 1.0, (FROXEL_DEPTH, vh, vw, 4)).astype(np.float32))
    return dict(name=name, w=w, h=h, g=g.pack(), depth=depth, prefill=prefill, volume=(volume, vw, vh, FROXEL_DEPTH), sky=(synth.sky_lut(), 200, 100),
                transmission=(synth.transmission_lut(), 128, 128), aim=aim)


_reference_cache = {}


def reference(name):
    """computed once per case and shared by the modes; callers must not modify it"""
    if name not in _reference_cache:
        c = build_case(name)
        c["ref"] = sr.sky_pass(c["g"], c["w"], c["h"], c["sky"], c["transmission"], c["volume"], MAX_DISTANCE, LIGHT)
        _reference_cache[name] = c
    return _reference_cache[name]


def gpu_sky_pass(be, c, dispatch=None, base=None):
    w, h = c["w"], c["h"]
    global_binding(be).set(c["g"])
    color = be.createImage(image_desc_2d(w, h, F.R11G11B10_uFloat), c["prefill"])
    depth = be.createImage(image_desc_2d(w, h, F.Depth32), c["depth"])
    lut = be.createImage(image_desc_2d(c["sky"][1], c["sky"][2], F.R11G11B10_uFloat), c["sky"][0])
    trans = be.createImage(image_desc_2d(c["transmission"][1], c["transmission"][2], F.R11G11B10_uFloat), c["transmission"][0])
    vol = be.createImage(ImageDescription(width=c["volume"][1], height=c["volume"][2], depth=c["volume"][3], type=ImageType.Type3D, format=F.RGBA16_sFloat,
                                          usageFlags=int(ImageUsageFlags.Storage) | int(ImageUsageFlags.Sampled), mipCount=MipCount.One, manualMipCount=1), c["volume"][0])
    settings = be.createUniformBuffer(64, synth.volumetric_settings_bytes(MAX_DISTANCE))
    light = be.createStorageBuffer(20, LIGHT)
    p = be.createComputePass("skyAndSunSprite.comp", [], "Sky and sun sprite")
    be.newFrame()
    exe = ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(color, 0, 0)],
        sampledImages=[ImageResource(depth, 0, 1), ImageResource(lut, 0, 2), ImageResource(vol, 0, 3), ImageResource(trans, 0, 4)],
        uniformBuffers=[UniformBufferResource(settings, 5)], storageBuffers=[StorageBufferResource(light, True, 6)]),
        b"", dispatch or (math.ceil(w / 8.0), math.ceil(h / 8.0), 1))
    if base is not None:
        exe.dispatchBase = base
    be.setComputePassExecution(exe)
    be.prepareForDrawcallRecording()
    be.renderFrame()
    return be.downloadImage(color, 0, np.uint32).reshape(h, w).copy()


def _report(line):
    print(line)
    path = os.environ.get("PLR_SKY_PASS_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


@pytest.mark.parametrize("name", list(CASES))
def test_cases_keep_every_pixel_centre_off_the_rim(oracle, name):
    """not gpu: the input condition of the GPU test, and that each case is what its name says"""
    c = reference(name)
    ref = c["ref"]
    sr.assert_disc_membership_is_decided(ref)
    sky = c["depth"] == 0
    lit = ref["in_disc"] & sky
    if name == "disc200":
        xs = np.flatnonzero(ref["in_disc"].any(0))
        assert xs.min() < 64 <= xs.max() and 14 <= xs.max() - xs.min() + 1 <= 18, "the disc straddles x = 64 and is about 16 pixels wide"
        assert lit.any() and (ref["in_disc"] & ~sky).any(), "the disc lies over sky and over geometry blocks"
        assert (c["depth"][:4] != 0).all()
    elif name == "corner67":
        assert sky.all() and lit[0, 0] and not lit[:, 12:].any() and not lit[12:].any() and 4 <= lit.sum() <= 40
    elif name == "pixel96":
        assert lit.sum() == 1 and lit[20, 48]
    else:
        assert not ref["in_disc"].any() and (ref["cos_t"] <= 0).all()
    g = sr.globals_of(c["g"])
    assert (c["w"] + 165.0) * c["w"] * float(g["time"]) < 2.0 ** 31 and (c["h"] + 1292.0) * c["h"] * float(g["time"]) < 2.0 ** 31


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_sky_pass_against_the_reference(backend, oracle, name, fast):
    c = reference(name)
    ref = c["ref"]
    sr.assert_disc_membership_is_decided(ref)
    backend.setMathMode(fast)
    try:
        out = gpu_sky_pass(backend, c)
        general = backend.getGeneralKernelExecutions()
    finally:
        backend.setMathMode(False)
    sky = c["depth"] == 0
    assert np.array_equal(out[~sky], c["prefill"][~sky]), "a geometry pixel was written"
    apart = sr.codes_apart(out[sky], ref["stored"][sky])
    differing = float((out[sky] != ref["stored"][sky]).mean())
    _report("sky pass %-9s %-5s: %d sky pixels, %d in the disc, %.5f not bit-identical to the reference, at most %d code(s) apart"
            % (name, "fast" if fast else "exact", int(sky.sum()), int((ref["in_disc"] & sky).sum()), differing, int(apart.max())))
    assert apart.max() <= 1, "%d sky pixels more than one R11G11B10 code from the reference (worst %d)" % (int((apart > 1).sum()), int(apart.max()))
    if fast:
        assert general[0] == 0, "the fast kernel declined: %r" % (general,)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_sky_pass_honours_the_dispatch_base(backend, oracle, fast):
    """workgroups [8, 16) x [5, 10) of disc200 = pixels [64, 128) x [40, 80): everything outside keeps the pre-fill, the rectangle equals the whole-frame run"""
    c = reference("disc200")
    backend.setMathMode(fast)
    try:
        whole = gpu_sky_pass(backend, c)
        part = gpu_sky_pass(backend, c, dispatch=(8, 5, 1), base=(8, 5, 0))
    finally:
        backend.setMathMode(False)
    inside = np.zeros((c["h"], c["w"]), bool)
    inside[40:80, 64:128] = True
    assert np.array_equal(part[inside], whole[inside])
    assert np.array_equal(part[~inside], c["prefill"][~inside])
    assert (part[inside] != c["prefill"][inside]).any()
