""""blueNoiseVoidAndCluster.comp" and "perlinNoise3D.comp" through the C-ABI against tests/noise_reference.py, in both kernel sets, byte for byte.

The tables handed to the passes are numpy's own (noise_reference.gaussian_table / perlin_gradients), so the comparison does not depend on the host's libm: every
byte of the image and every status word {swaps, converged, ones, 0} must equal the reference's.
Blue noise: the cases of tests/noise_cases.py - 8 x 8 R8 (one wave holds every pixel), 20 x 12 RG8 (N no multiple of 64, not square, two blocks), 32 x 32 RG8 (the
pipeline's shape), 64 x 64 R8 (four pixels per lane, denormal and zero table entries) -, two seeds each.
Perlin: 8^3, 20^3 and 32^3 with 8 cells, 12^3 with 5.
The launchers refuse, with a message that names the cause, a size outside 4 .. 64, a missing or short buffer, a read-only status buffer, a wrong dispatch, a
format that is neither R8 nor RG8, a volume that is no cube, a cell count outside 1 .. 32.
"""
import struct

import numpy as np
import pytest

import noise_cases as nc
import noise_reference as ref
from util import F, ComputePassExecution, ImageDescription, ImageResource, ImageType, ImageUsageFlags, RenderPassResources, StorageBufferResource, image_desc_2d

SENTINEL = 0xA5


def gpu_blue_pass(be, width, height, fmt, seed, first_stream, table, drop=None, table_bytes=None, status_bytes=None, status_read_only=False, dispatch=None):
    """-> (image bytes (H, W, channels) uint8, status (channels, 4) uint32). drop: a binding left out; *_bytes: a buffer created at that size"""
    channels = {F.R8: 1, F.RG8: 2}.get(fmt, 4)
    texel = {F.R8: 1, F.RG8: 2}.get(fmt, 4)
    image = be.createImage(image_desc_2d(width, height, fmt), np.full(width * height * texel, SENTINEL, np.uint8))
    data = np.ascontiguousarray(table, np.float32).tobytes()
    data = data[:table_bytes] if table_bytes is not None else data
    buffers = {1: be.createStorageBuffer(max(len(data), 4), data), 2: be.createStorageBuffer(status_bytes or 16 * channels, bytes([SENTINEL]) * (status_bytes or 16 * channels))}
    p = be.createComputePass("blueNoiseVoidAndCluster.comp", [], "Blue noise void and cluster")
    be.newFrame()
    res = RenderPassResources(storageBuffers=[StorageBufferResource(h, b == 1 or status_read_only, b) for b, h in buffers.items() if b != drop],
                              storageImages=[] if drop == 0 else [ImageResource(image, 0, 0)])
    be.setComputePassExecution(ComputePassExecution(p, res, struct.pack("<2I", seed, first_stream), dispatch or (channels, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    return be.downloadImage(image).reshape(height, width, texel).copy(), be.downloadStorageBuffer(buffers[2], 16 * channels, dtype=np.uint32).reshape(channels, 4).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("name", list(nc.BLUE_CASES))
def test_gpu_blue_noise_equals_the_reference_byte_for_byte(backend, name, seed, fast):
    w, h, channels = nc.BLUE_CASES[name]
    want, want_status = nc.blue_texture(name, seed)
    backend.setMathMode(fast)
    try:
        got, status = gpu_blue_pass(backend, w, h, F.R8 if channels == 1 else F.RG8, seed, nc.FIRST_STREAM, ref.gaussian_table(w, h))
    finally:
        backend.setMathMode(False)
    differing = int((got != want).sum())
    print("blue noise %-9s seed %4d %s: %d of %d bytes differ; status %r, the reference's %r" % (name, seed, "fast" if fast else "exact", differing, want.size, status.tolist(), want_status.tolist()))
    assert np.array_equal(status, want_status)
    assert differing == 0, "first differing byte (y, x, channel) = %r" % (tuple(int(v[0]) for v in np.nonzero(got != want)),)


def gpu_perlin_pass(be, size, g, gradients, drop=None, gradient_bytes=None, dispatch=None, fmt=F.R8):
    """-> (D, H, W) uint8. size: the resolution or (w, h, d)"""
    w, h, d = (size, size, size) if isinstance(size, int) else size
    desc = ImageDescription(width=w, height=h, depth=d, type=ImageType.Type3D, format=fmt, usageFlags=int(ImageUsageFlags.Storage) | int(ImageUsageFlags.Sampled))
    image = be.createImage(desc, np.full(w * h * d * (1 if fmt == F.R8 else 2), SENTINEL, np.uint8))
    data = np.ascontiguousarray(gradients, np.float32).tobytes()
    data = data[:gradient_bytes] if gradient_bytes is not None else data
    buffer = be.createStorageBuffer(max(len(data), 16), data)
    p = be.createComputePass("perlinNoise3D.comp", [], "Perlin noise 3D")
    be.newFrame()
    res = RenderPassResources(storageBuffers=[] if drop == 1 else [StorageBufferResource(buffer, True, 1)], storageImages=[] if drop == 0 else [ImageResource(image, 0, 0)])
    be.setComputePassExecution(ComputePassExecution(p, res, struct.pack("<I", g), dispatch or ((w * h * d + 255) // 256, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    return be.downloadImage(image).reshape(d, h, -1).copy()


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(nc.PERLIN_CASES))
def test_gpu_perlin_volume_equals_the_reference_byte_for_byte(backend, name, fast):
    res, g = nc.PERLIN_CASES[name]
    gradients, want = nc.perlin(name)
    backend.setMathMode(fast)
    try:
        got = gpu_perlin_pass(backend, res, g, gradients)
    finally:
        backend.setMathMode(False)
    differing = int((got != want).sum())
    print("perlin %-8s %s: %d of %d bytes differ" % (name, "fast" if fast else "exact", differing, want.size))
    assert differing == 0, "first differing voxel (z, y, x) = %r" % (tuple(int(v[0]) for v in np.nonzero(got != want)),)


BLUE_REFUSALS = {
    "no image": (dict(drop=0), "missing storage image"),
    "no table": (dict(drop=1), "Gaussian table"),
    "short table": (dict(table_bytes=4 * 16 * 16 - 4), "Gaussian table"),
    "no status": (dict(drop=2), "status"),
    "short status": (dict(status_bytes=16), "status"),
    "read-only status": (dict(status_read_only=True), "read-only"),
    "size 3": (dict(width=3), "outside 4 .. 64"),
    "size 65": (dict(height=65), "outside 4 .. 64"),
    "format": (dict(fmt=F.RGBA8), "neither R8 nor RG8"),
    "dispatch of one channel": (dict(dispatch=(1, 1, 1)), "one block per channel"),
    "dispatch in y": (dict(dispatch=(2, 2, 1)), "one block per channel"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(BLUE_REFUSALS))
def test_gpu_blue_noise_launcher_refuses(backend, what):
    from plainrenderer_amd.backend import PlrError
    overrides, message = BLUE_REFUSALS[what]
    args = dict(width=16, height=16, fmt=F.RG8, seed=1, first_stream=0, table=ref.gaussian_table(16, 16))
    args.update(overrides)
    if args["width"] != 16 or args["height"] != 16:
        args["table"] = np.zeros(args["width"] * args["height"], np.float32)
    with pytest.raises(PlrError, match=message):
        gpu_blue_pass(backend, **args)


PERLIN_REFUSALS = {
    "no volume": (dict(drop=0), "missing storage image"),
    "no gradients": (dict(drop=1), "gradients"),
    "short gradients": (dict(gradient_bytes=16 * 5 ** 3 - 16), "gradients"),
    "no cube": (dict(size=(12, 12, 8)), "must be a cube"),
    "format": (dict(fmt=F.RG8), "expects R8"),
    "no cells": (dict(g=0), "1 .. 32"),
    "33 cells": (dict(g=33), "1 .. 32"),
    "dispatch": (dict(dispatch=(1, 1, 1)), "a lane per voxel"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(PERLIN_REFUSALS))
def test_gpu_perlin_launcher_refuses(backend, what):
    from plainrenderer_amd.backend import PlrError
    overrides, message = PERLIN_REFUSALS[what]
    args = dict(size=12, g=5, gradients=nc.perlin("12^3 g5")[0])
    args.update(overrides)
    with pytest.raises(PlrError, match=message):
        gpu_perlin_pass(backend, **args)
