"""The "sunShadowRaster.comp" pass through the C-ABI against tests/shadow_raster_reference.py, in both math modes: every texel of the Depth16 map and the three
counters must be bit-identical.

The map is pre-filled with a bit pattern (the pass clears: an untouched texel would keep it) and the scratch buffer with 0xA5 bytes (the pass resets its own
header). Every case binds a sunShadowInfo block whose other light matrices are garbage, so the cascade index constant is what selects the matrix.
Cases, the smallest that reach every way the kernels can go wrong:
  unit96    res 96 = 1.5 tiles per axis (a ragged tile column and row, 16-byte rows). Hand-made triangles on the sub-pixel grid: a quad split along a diagonal
            through pixel centres and an axis-aligned quad with edges on pixel centres, two depths per half; a triangle whose pixel box is exactly 4 x 4 (the
            lane-per-triangle path's largest) and one that is 5 x 4 (the wave path's smallest); a triangle that straddles the tile boundary x = 64 and a small
            one that does; overlapping triangles at three depths in the second tile row; two long triangles, one
            just inside and one outside the span the kernel evaluates in 32-bit arithmetic; a front face and a zero-area triangle that draw nothing
  mesh200   res 200 (3.125 tiles, rows of 400 bytes: 16-byte stores), box + uv_sphere + torus under three affine transforms, 1496 triangles, once per cascade
            with the three matrices of SynthScene.shadow_cascades
  dense64   res 64, one tile, 20 011 random triangles a quarter of a pixel to 3 pixels across (not a multiple of 64: the list's tail), some outside the map,
            two fifths of them clustered so that texels collect eight fragments and more
  big130    res 130 (odd rows: texel-by-texel stores): a triangle over the whole map with one vertex 99 970 pixels outside and depths from below 0 to above 1,
            two slivers narrower than a pixel across the whole map (apex 270 pixels outside), one triangle with a vertex 2^21 pixels out (the guard band's reject)
"""
import struct

import numpy as np
import pytest

import shadow_raster_cases as sc
import shadow_raster_reference as ref
from plainrenderer_amd.backend import spec_uint
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

TRI_4X4 = [(40.0, 40.0, 0.35), (44.0, 40.0, 0.35), (44.0, 44.0, 0.45)]
TRI_5X4 = [(50.0, 40.0, 0.55), (55.0, 40.0, 0.55), (55.0, 44.0, 0.65)]
# the kernel evaluates a triangle whose snapped vertices span less than 2^15 sub-pixel units on both axes in 32-bit arithmetic: the widest that does, and one that does not
TRI_SPAN_32767 = [(-20.0, 60.0, 0.45), (107.99609375, 61.0, 0.45), (-20.0, 63.0, 0.7)]
TRI_SPAN_33280 = [(-20.0, 56.0, 0.4), (110.0, 57.0, 0.4), (-20.0, 59.0, 0.6)]


def _unit96():
    tris = sc.quad(2.5, 2.5, 10.5, 10.5, 0.3, 0.6) + sc.quad(20.5, 4.5, 30.5, 9.5, 0.4, 0.7) + [TRI_4X4, TRI_5X4]
    tris += [[(60.25, 20.5, 0.2), (70.75, 22.0, 0.5), (66.0, 30.25, 0.8)], [(62.0, 50.0, 0.3), (66.0, 50.0, 0.3), (66.0, 53.0, 0.9)]]
    tris += [[(5.0, 66.0, 0.5), (60.0, 66.0, 0.5), (60.0, 94.0, 0.5)], [(10.0, 70.0, 0.25), (50.0, 70.0, 0.25), (50.0, 90.0, 0.25)],
             [(30.0, 68.0, 0.8), (58.0, 68.0, 0.8), (58.0, 96.0, 0.8)]]
    tris += sc.quad(70.5, 70.5, 90.5, 95.5, 0.2, 0.9) + [TRI_SPAN_32767, TRI_SPAN_33280]
    tris += [[(10.0, 40.0, 0.5), (10.0, 50.0, 0.5), (20.0, 40.0, 0.5)]]  # A < 0: a front face
    tris += [[(30.0, 60.0, 0.5), (35.0, 65.0, 0.5), (40.0, 70.0, 0.5)]]  # A == 0
    return [(sc.pixel_case(tris, 96), 2)]


def _mesh200():
    lights = ref.light_matrices(sc.mesh_scene()["info"])
    return [(sc.mesh_case(lights[c], 200), c) for c in range(3)]


def _dense64():
    """three fifths of the triangles uniform over the tile and 2 pixels around it, two fifths clustered (sigma 3 pixels) so that some texels collect many fragments;
    each triangle three points on a circle of diameter `across` at roughly 120 degrees, random winding"""
    rng = np.random.default_rng(0x53484457)
    n = 20011
    centre = np.where(rng.random((n, 1)) < 0.6, rng.uniform(-2.0, 66.0, (n, 2)), rng.normal((21.3, 40.7), 3.0, (n, 2)))[:, None, :]
    across = rng.uniform(0.25, 3.0, (n, 1))
    angle = rng.uniform(0.0, 2.0 * np.pi, (n, 1)) + np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0) * (np.arange(3)[None, :] * 2.0 * np.pi / 3.0 + rng.uniform(-0.4, 0.4, (n, 3)))
    px = centre + 0.5 * across[:, :, None] * np.stack([np.cos(angle), np.sin(angle)], -1)
    pos = np.concatenate([2.0 * px / 64.0 - 1.0, rng.uniform(0.05, 0.95, (n, 3, 1))], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(3 * n, dtype=np.uint32)
    return [(dict(res=64, light=sc.IDENTITY.copy(), transforms=sc.IDENTITY.reshape(1, 16).copy(), positions=pos, indices=idx, draws=np.array([[0, 3 * n, 0, 0]], np.uint32)), 1)]


SLIVERS = [[(-5.0, 30.25, 0.9), (400.0, 75.0, 0.9), (-5.0, 30.875, 0.9)], [(-3.0, -3.0, 0.95), (400.0, 399.0, 0.95), (-3.0, -2.25, 0.95)]]


def _big130():
    tris = [[(-200.0, -20.0, -0.5), (99970.0, 60.0, 0.5), (-200.0, 150.0, 1.5)],
            SLIVERS[0], SLIVERS[1],
            [(float(2 ** 21), 10.0, 0.5), (5.0, 5.0, 0.5), (5.0, 20.0, 0.5)]]
    return [(sc.pixel_case(tris, 130), 3)]


CASES = {"unit96": _unit96, "mesh200": _mesh200, "dense64": _dense64, "big130": _big130}
_reference_cache = {}


def reference(name):
    """[(case, cascade index, reference result)], computed once per case and shared by the modes; callers must not modify it"""
    if name not in _reference_cache:
        _reference_cache[name] = [(case, cascade, sc.rasterise(case)) for case, cascade in CASES[name]()]
    return _reference_cache[name]


def _pixel_box(tri, res):
    case = sc.pixel_case([tri], res)
    X, Y, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], res)
    return ((int(X.max()) - 128) >> 8) - ((int(X.min()) + 127) >> 8) + 1, ((int(Y.max()) - 128) >> 8) - ((int(Y.min()) + 127) >> 8) + 1, sc.rasterise(case)["coverage"].sum()


def check_case_is_what_it_is_for(name):
    """on the reference alone: the properties the case is there for"""
    runs = reference(name)
    assert [r["rejects"] for _, _, r in runs] == ([1] if name == "big130" else [0] * len(runs))
    assert all(r["drawn"] > 0 and r["map"].any() for _, _, r in runs)
    if name == "unit96":
        w, h, covered = _pixel_box(TRI_4X4, 96)
        assert (w, h) == (4, 4) and covered > 0
        w, h, covered = _pixel_box(TRI_5X4, 96)
        assert (w, h) == (5, 4) and covered > 0
        r = runs[0][2]
        assert r["submitted"] == 17 and r["drawn"] == 15, "the front face and the zero-area triangle are not drawn"
        for tri, span in ((TRI_SPAN_32767, 32767), (TRI_SPAN_33280, 33280)):
            case = sc.pixel_case([tri], 96)
            X, _, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], 96)
            assert int(X.max() - X.min()) == span and sc.rasterise(case)["coverage"].sum() > 100
        assert r["coverage"][:, 63].any() and r["coverage"][:, 64].any() and r["coverage"][64:, :].any() and r["coverage"].max() == 3
    elif name == "mesh200":
        assert all(1400 <= r["submitted"] <= 1600 for _, _, r in runs)
        assert len({r["map"].tobytes() for _, _, r in runs}) == 3
    elif name == "dense64":
        assert runs[0][2]["submitted"] == 20011 and 20011 % 64 != 0
        assert runs[0][2]["coverage"].max() >= 8
    else:
        r = runs[0][2]
        assert (r["coverage"] >= 1).all(), "the large triangle covers the whole map"
        assert (r["map"] == 0).any() and (r["map"] == 65535).any(), "depths below 0 and above 1 on covered texels"
        assert r["drawn"] == 3 and r["submitted"] == 4
        for sliver in SLIVERS:  # at most 5 / 8 of a pixel high at the left edge, tapering to 2 / 5 at the right: never two centres of a column, centres all the way across
            alone = sc.rasterise(sc.pixel_case([sliver], 130))["coverage"]
            columns = np.flatnonzero(alone.any(axis=0))
            assert alone.sum(axis=0).max() == 1 and columns.min() < 15 and columns.max() >= 115 and alone.sum() >= 40


def gpu_raster(be, case, cascade):
    """one execution through the C-ABI with the test's own buffers -> (map, (submitted, drawn, rejects))"""
    res = case["res"]
    triangles = int(case["draws"][:, 1].sum()) // 3
    info = np.full(76, 7.25, np.float32)  # splits, 4 matrices, scales: anything but the cascade's own matrix is garbage
    info[4 + 16 * cascade:4 + 16 * (cascade + 1)] = case["light"]
    scratch_bytes = 64 + 16 * ((triangles + 3) // 4) + 80 * triangles
    prefill = ((np.arange(res * res, dtype=np.uint64) * 40503 + 0x1234) & 0xFFFF).astype(np.uint16)
    buffers = [be.createStorageBuffer(304, info.tobytes())]
    for a in (case["transforms"], case["positions"], case["indices"], case["draws"]):
        b = np.ascontiguousarray(a).tobytes()
        buffers.append(be.createStorageBuffer(len(b), b))
    buffers.append(be.createStorageBuffer(scratch_bytes, b"\xa5" * scratch_bytes))
    target = be.createImage(image_desc_2d(res, res, ImageFormat.Depth16), prefill)
    p = be.createComputePass("sunShadowRaster.comp", [spec_uint(0, cascade)], "Sun shadow cascade %d" % cascade)
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(target, 0, 0)], storageBuffers=[StorageBufferResource(b, i != 5, i) for i, b in enumerate(buffers)]),
        struct.pack("<2I", case["draws"].shape[0], triangles), (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = be.downloadImage(target, 0, np.uint16).reshape(res, res).copy()
    header = be.downloadStorageBuffer(buffers[5], 16, dtype=np.uint32)
    assert int(header[0]) == int(header[2]), "the cursor counts the drawn triangles"
    return out, (int(header[1]), int(header[2]), int(header[3]))


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_are_for(name):
    """not gpu: the input conditions of the GPU test"""
    check_case_is_what_it_is_for(name)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_shadow_raster_is_bit_identical_to_the_reference(backend, name, fast):
    check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for case, cascade, r in reference(name):
            out, counters = gpu_raster(backend, case, cascade)
            general = backend.getGeneralKernelExecutions()
            differing = int((out != r["map"]).sum())
            print("shadow raster %-8s cascade %d %-5s: %d of %d texels differ, counters %r (reference %r)"
                  % (name, cascade, "fast" if fast else "exact", differing, out.size, counters, (r["submitted"], r["drawn"], r["rejects"])))
            assert differing == 0, "%d texels differ from the reference, first at %r" % (differing, tuple(np.argwhere(out != r["map"])[0]))
            assert counters == (r["submitted"], r["drawn"], r["rejects"])
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_launcher_refuses_what_it_cannot_run(backend):
    """fails loudly: a scratch buffer too small for the triangle count, a map that is not Depth16"""
    from plainrenderer_amd.backend import PlrError
    case, cascade = _unit96()[0]
    small = dict(case)
    be = backend
    with pytest.raises(PlrError, match="scratch"):
        _run_with(be, small, cascade, scratch_bytes=64)
    with pytest.raises(PlrError, match="Depth16"):
        _run_with(be, small, cascade, fmt=ImageFormat.R16_sFloat)


def _run_with(be, case, cascade, scratch_bytes=None, fmt=ImageFormat.Depth16):
    res = case["res"]
    triangles = int(case["draws"][:, 1].sum()) // 3
    info = np.zeros(76, np.float32)
    buffers = [be.createStorageBuffer(304, info.tobytes())]
    for a in (case["transforms"], case["positions"], case["indices"], case["draws"]):
        b = np.ascontiguousarray(a).tobytes()
        buffers.append(be.createStorageBuffer(len(b), b))
    buffers.append(be.createStorageBuffer(scratch_bytes or 64 + 96 * triangles))
    target = be.createImage(image_desc_2d(res, res, fmt))
    p = be.createComputePass("sunShadowRaster.comp", [spec_uint(0, cascade)], "Sun shadow cascade refused")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(target, 0, 0)], storageBuffers=[StorageBufferResource(b, i != 5, i) for i, b in enumerate(buffers)]),
        struct.pack("<2I", case["draws"].shape[0], triangles), (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
