"""The packed-only output of the fast SDF trace (csrc/kernels_fast/sdf_trace_fast.hip sdfDiffuseTraceFastKernel<..., PACKED_ONLY>).

At pass fusion level 2 the trace leaves out its two image stores when the only reader of its result, spatial filter 0, gathers the packed texels the trace
writes for it (PassCtx::elidableStorage). PLR_TRACE_PACKED_ONLY is read per launch; "0" keeps the stores. Nothing else may change: frames are compared byte
for byte with the switch on and off, the images are written at fusion level 1 and in a decision-signature run, and a download of an image that was left
unwritten fails loudly. The backend has no download for the packed texels themselves: they are compared through their only reader, the filter's output.
(The same change also shortened the kernel's prologue - pixel loads ahead of the instance staging, staging in two levels; bit-identical in the tests this
file had for them, but without effect on the frame time and therefore not in the tree: profiles/r09_trace_prologue.txt.)
These sizes are small: a rounding that differs in one texel of thousands between the storing and the packed-only kernel is what tests/test_fusion.py holds at 1280 x 720.
Inputs come from seeded generators only (plainrenderer_amd.synth)."""
import math
import struct

import numpy as np
import pytest

import passes
from passes import F
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.backend import spec_bool, spec_int
from plainrenderer_amd.scene import Camera, GlobalShaderInfo
from util import (ComputePassExecution, ImageResource, RenderPassResources, StorageBufferResource, UniformBufferResource, image_desc_2d, light_buffer_bytes)

SDF_RES = 16
INFLUENCE = 5.0
ALL_SWITCHES = ("PLR_TRACE_PACKED_ONLY",)


class Scene:
    pass


def build_scene(w, h, grid, cell, seed_id, cam_pos, cam_dir):
    """the set-up of tests/test_sdfgi.py's scenes at a frame size of the caller's choice; culled on the CPU by the oracle"""
    s = Scene()
    s.w, s.h, s.tw, s.th = w, h, w // 2, h // 2
    sc = synth.SynthScene(grid=grid, cell=cell, seed_id=seed_id)
    cam = Camera.look(cam_pos, cam_dir, aspect=w / h)
    s.gb = sc.gbuffer(cam, w, h, cam)
    s.inst_bytes, s.bb_bytes, s.vols = sc.sdf_instances(SDF_RES)
    s.noise = synth.blue_noise_standins()
    s.sky = synth.sky_lut()
    sun = np.array([0.35, -0.8, 0.45])
    sun /= np.linalg.norm(sun)
    s.shadow_info, s.shadow_maps = sc.shadow_cascades(cam, sun, 2.0, 60.0, 256)
    g = GlobalShaderInfo(frameIndex=6, sunDirection=(*sun.tolist(), 0.0), time=3.0)
    g.viewProjectionPrevious = cam.view_projection()
    cam.fill_global(g, w, h)
    s.g = g
    s.light = light_buffer_bytes(sun_color=(1.0, 0.92, 0.8), prev_exposure=8e-5, sun_strength_exposed=128000 * 8e-5)
    fpts, fnrm = cam.frustum_points_normals()
    hiz = passes.orc_hiz(s.gb["depth"], w, h)
    s.half_depth = passes.orc_depth_downscale(s.gb["depth"], w, h)
    _, s.tiles = passes.orc_sdf_culling(s.inst_bytes, s.bb_bytes, fpts, fnrm, INFLUENCE, hiz[4], s.tw, s.th, g.pack())
    return s


def tile_counts(s):
    """objectCount of the culling tiles the trace reads (the buffer's rows are as long as the full-resolution frame's)"""
    stride, tcx, tcy = math.ceil(s.w / 32.0), math.ceil(s.tw / 32.0), math.ceil(s.th / 32.0)
    return s.tiles.reshape(-1, passes.TILE_UINTS)[:, 0].reshape(tcy, stride)[:, :tcx]


@pytest.fixture(scope="module")
def grid_scene():
    # 200 x 120: a 100 x 60 trace, a multiple of neither 8, 16 nor 32 - partial 8 x 8 groups, partial blocks and partial culling tiles
    return build_scene(200, 120, 4, 8.0, 300, (16.0, -7.0, -6.0), (0.0, 0.16, 1.0))


class TraceRig:
    """images, buffers and passes of one scene on the backend, created once; run() records one frame"""

    def __init__(self, be, s):
        self.be, self.s = be, s
        vol_idx, noise_idx = passes.make_bindless(be, s.vols, SDF_RES, s.noise)
        s.g.noiseTextureIndices = tuple(noise_idx)
        self.gp = s.g.pack()
        w, h, tw, th = s.w, s.h, s.tw, s.th
        mk = lambda fmt, ww=tw, hh=th, data=None: be.createImage(image_desc_2d(ww, hh, fmt), data)
        self.out_ysh, self.out_cocg = mk(F.RGBA16_sFloat), mk(F.RG16_sFloat)
        self.sp_ysh, self.sp_cocg = mk(F.RGBA16_sFloat), mk(F.RG16_sFloat)
        self.depth = mk(F.Depth32, w, h, np.ascontiguousarray(s.gb["depth"], np.float32))
        self.normal = mk(F.RGBA8, w, h, np.ascontiguousarray(s.gb["normal"]))
        self.half_depth = mk(F.R16_sFloat, tw, th, np.ascontiguousarray(s.half_depth))
        self.sky = mk(F.R11G11B10_uFloat, 200, 100, s.sky)
        self.shadow = mk(F.Depth16, 256, 256, np.ascontiguousarray(s.shadow_maps[2]))
        self.light = be.createStorageBuffer(20, s.light)
        self.tiles = be.createStorageBuffer(s.tiles.nbytes, s.tiles.tobytes())
        self.infl = be.createUniformBuffer(4, struct.pack("<f", INFLUENCE))
        self.sinfo = be.createStorageBuffer(304, s.shadow_info)
        self.trace = be.createComputePass("sdfDiffuseTrace.comp", [spec_bool(0, True), spec_int(1, 2)], "Indirect diffuse SDF trace")
        self.spatial = be.createComputePass("filterIndirectDiffuseSpatial.comp", [spec_int(0, 0)], "Indirect diffuse spatial filter")
        inst_bytes = passes.patch_instance_texture_indices(s.inst_bytes, vol_idx)
        self.inst = be.createStorageBuffer(len(inst_bytes), inst_bytes)

    def _record(self, with_spatial):
        be, s = self.be, self.s
        groups = (math.ceil(s.tw / 8.0), math.ceil(s.th / 8.0), 1)
        passes.global_binding(be).set(self.gp)
        be.newFrame()
        be.setComputePassExecution(ComputePassExecution(self.trace, RenderPassResources(
            storageImages=[ImageResource(self.out_ysh, 0, 0), ImageResource(self.out_cocg, 0, 1)],
            sampledImages=[ImageResource(self.depth, 0, 2), ImageResource(self.normal, 0, 3), ImageResource(self.sky, 0, 4), ImageResource(self.shadow, 0, 10)],
            storageBuffers=[StorageBufferResource(self.light, True, 5), StorageBufferResource(self.inst, True, 6), StorageBufferResource(self.tiles, True, 7),
                            StorageBufferResource(self.sinfo, True, 9)],
            uniformBuffers=[UniformBufferResource(self.infl, 8)]), b"", groups))
        if with_spatial:
            be.setComputePassExecution(ComputePassExecution(self.spatial, RenderPassResources(
                storageImages=[ImageResource(self.sp_ysh, 0, 0), ImageResource(self.sp_cocg, 0, 1)],
                sampledImages=[ImageResource(self.out_ysh, 0, 2), ImageResource(self.out_cocg, 0, 3), ImageResource(self.half_depth, 0, 4),
                               ImageResource(self.normal, 0, 5)]), b"", groups))
        be.renderFrame()
        general, which = be.getGeneralKernelExecutions()
        assert general == 0, "not the fast kernels: %s" % which

    def _get(self, *images):
        return [self.be.downloadImage(i, 0, np.uint16).copy() for i in images]

    def run(self):
        """-> dict of arrays: the three kernel families (fast math, fusion level 1: every image is written)"""
        be, out = self.be, {}
        be.setMathMode(True)
        be.setPassFusion(1)
        try:
            self._record(False)
            out["alone Y_SH"], out["alone CoCg"] = self._get(self.out_ysh, self.out_cocg)
            self._record(True)
            out["packing Y_SH"], out["packing CoCg"], out["filtered Y_SH"], out["filtered CoCg"] = self._get(self.out_ysh, self.out_cocg, self.sp_ysh, self.sp_cocg)
            with passes.gpu_signature(be, self.s.tw * self.s.th) as sig:
                self._record(False)
            out["signature words"] = sig.words.copy()
            out["signed Y_SH"], out["signed CoCg"] = self._get(self.out_ysh, self.out_cocg)
        finally:
            be.setPassFusion(2)
            be.setMathMode(False)
        return out


# ------------------------------------------------------------------ CPU
def test_scene_sizes_are_ragged(grid_scene):
    s = grid_scene
    assert (s.tw, s.th) == (100, 60) and s.tw % 8 and s.th % 8 and s.tw % 16 and s.th % 16 and s.tw % 32 and s.th % 32
    counts = tile_counts(s)
    assert counts.shape == (2, 4) and 1 <= counts.max() <= 16


@pytest.fixture(scope="module")
def grid_rig(backend, grid_scene):
    return TraceRig(backend, grid_scene)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_packed_only_trace_changes_no_frame(backend, monkeypatch):
    from plainrenderer_amd.frame import FramePipeline, SyntheticInputs
    w, h, n_frames = 200, 120, 4
    cams = [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=w / h) for i in range(n_frames + 1)]
    scene = synth.SynthScene(grid=4, cell=8.0, seed_id=514)
    names = ["swapchain", "post1"]
    inputs, results = None, {}
    for n in ALL_SWITCHES:
        monkeypatch.delenv(n, raising=False)
    try:
        backend.setMathMode(True)
        for mode, level in (("off", 2), ("on", 2), ("off level 1", 1), ("on level 1", 1)):
            if mode.startswith("off"):
                monkeypatch.setenv("PLR_TRACE_PACKED_ONLY", "0")
            else:
                monkeypatch.delenv("PLR_TRACE_PACKED_ONLY", raising=False)
            backend.setPassFusion(level)
            fp = FramePipeline(backend, w, h, shadow_map_res=256, brdf_lut_res=32, froxel_depth=16, max_sdf_instances=64, sdf_half_res_trace=1)
            if inputs is None:
                inputs = SyntheticInputs(scene, cams[1], cams[0], w, h, sdf_res=16, shadow_res=256, froxel_depth=16, sun_direction=(0.35, -0.8, 0.45))
            inputs.upload(fp)
            out = []
            for f in range(n_frames):
                fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
                general, which = backend.getGeneralKernelExecutions()
                assert general == 0, which
                arrays = [backend.downloadImage(fp.image(name), 0, np.uint8).copy() for name in names]
                arrays += [backend.downloadStorageBuffer(fp.storage_buffer("light"), 20, dtype=np.uint8).copy(),
                           backend.downloadStorageBuffer(fp.storage_buffer("histogram"), 512, dtype=np.uint8).copy()]
                if level == 1:
                    arrays += [backend.downloadImage(fp.image("giYSH0"), 0, np.uint8).copy(), backend.downloadImage(fp.image("giCoCg0"), 0, np.uint8).copy()]
                elif mode == "on":
                    with pytest.raises(RuntimeError, match="not written in the last frame"):
                        backend.downloadImage(fp.image("giYSH0"), 0, np.uint8)
                out.append(arrays)
            results[mode] = out
            fp.destroy()
    finally:
        monkeypatch.delenv("PLR_TRACE_PACKED_ONLY", raising=False)
        backend.setPassFusion(2)
        backend.setMathMode(False)
    what = names + ["light buffer", "histogram", "giYSH0", "giCoCg0"]
    assert len(np.unique(results["on"][-1][0])) > 8 and len(np.unique(results["on level 1"][-1][4])) > 16, "neither the swapchain nor the GI image is constant"
    for a_mode, b_mode in (("off", "on"), ("off level 1", "on level 1"), ("off level 1", "on")):
        for f in range(n_frames):
            for a, b, name in zip(results[a_mode][f], results[b_mode][f], what):
                assert np.array_equal(a, b), "%s differs between %s and %s, frame %d" % (name, a_mode, b_mode, f)
    assert any(x.any() for x in results["on level 1"][-1][4:]), "the GI images of the level 1 run are written"


@pytest.mark.gpu
def test_gpu_packed_only_trace_leaves_its_images_unwritten_and_a_signature_run_does_not(grid_rig, monkeypatch):
    """the trace with spatial filter 0 behind it and nothing else in the frame, fusion level 2: with the switch on the trace's images are not written (a download
    fails loudly) and the filter, which gathers the packed texels, writes what it writes at level 1 and with the switch off; a decision-signature run stores"""
    rig, be = grid_rig, grid_rig.be
    for n in ALL_SWITCHES:
        monkeypatch.delenv(n, raising=False)
    level1 = rig.run()
    be.setMathMode(True)
    try:
        be.setPassFusion(2)
        rig._record(True)
        for image in (rig.out_ysh, rig.out_cocg):
            with pytest.raises(RuntimeError, match="not written in the last frame"):
                be.downloadImage(image, 0, np.uint16)
        on = rig._get(rig.sp_ysh, rig.sp_cocg)
        monkeypatch.setenv("PLR_TRACE_PACKED_ONLY", "0")
        rig._record(True)
        off = rig._get(rig.out_ysh, rig.out_cocg, rig.sp_ysh, rig.sp_cocg)
        monkeypatch.delenv("PLR_TRACE_PACKED_ONLY", raising=False)
        with passes.gpu_signature(be, rig.s.tw * rig.s.th) as sig:
            rig._record(False)
        signed = rig._get(rig.out_ysh, rig.out_cocg)
    finally:
        monkeypatch.delenv("PLR_TRACE_PACKED_ONLY", raising=False)
        be.setPassFusion(2)
        be.setMathMode(False)
    for got, key in zip(on, ("filtered Y_SH", "filtered CoCg")):
        assert np.array_equal(got, level1[key]), key
    for got, key in zip(off, ("packing Y_SH", "packing CoCg", "filtered Y_SH", "filtered CoCg")):
        assert np.array_equal(got, level1[key]), key
    for got, key in zip(signed, ("signed Y_SH", "signed CoCg")):
        assert np.array_equal(got, level1[key]), key
    assert np.array_equal(sig.words, level1["signature words"])
