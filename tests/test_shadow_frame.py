"""Mesh shadow casters in the frame pipeline (plrf_set_shadow_casters): 96 x 54, shadow_map_res 128, run_light_matrix = 1, the casters of mesh200.

After a frame the three cascade maps must be bit-identical to tests/shadow_raster_reference.py evaluated with the light matrices DOWNLOADED from sunShadowInfo
(the cascade fit runs on the GPU in front of the pass), shadow3 - above the cascade count - must still hold the bytes uploaded into it, and a pipeline without
casters must keep all four uploaded maps. All four maps are uploaded as bit patterns first. New transforms move the shadow in the next frame, draw_count 0
stops the writes, the counters equal the reference's, a fast-set frame runs no general kernel, and the refusals return their codes and name their causes.
Replacing the casters by a larger set (300 draws, a mesh without indices among their meshes) and then by a single draw in buffers that stay larger gives the
reference's maps and counters in the frame after each call.
"""
import copy

import numpy as np
import pytest

import shadow_raster_cases as sc
import shadow_raster_reference as ref
from plainrenderer_amd import synth
from plainrenderer_amd.scene import Camera

W, H, RES = 96, 54, 128
FP_ARGS = dict(shadow_map_res=RES, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64, run_light_matrix=1)
INVALID_ARGUMENT, UNSUPPORTED = -1, -6

_inputs = {}


def _scene_inputs():
    """generated once for the module; never modified"""
    if not _inputs:
        from plainrenderer_amd.frame import SyntheticInputs
        s = sc.mesh_scene()
        cams = [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=W / H) for i in range(3)]
        inp = SyntheticInputs(s["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45))
        patterns = [((np.arange(RES * RES, dtype=np.uint64) * (40503 + 2 * i) + 77 * i) & 0xFFFF).astype(np.uint16).reshape(RES, RES) for i in range(4)]
        moved = [(m, t.copy()) for m, t in s["draws"]]
        for _, t in moved:
            t[12:15] += np.asarray(s["cam"].right, np.float32) * np.float32(0.75)
        _inputs.update(inp=inp, cams=cams, patterns=patterns, moved=moved)
    return _inputs


def _pipeline(be, **extra):
    from plainrenderer_amd.frame import FramePipeline
    s = _scene_inputs()
    fp = FramePipeline(be, W, H, **dict(FP_ARGS, **extra))
    inp = copy.copy(s["inp"])
    inp.upload(fp)
    for i in range(4):
        be.uploadImage(fp.image("shadow%d" % i), s["patterns"][i])
    return fp


def _maps(be, fp):
    return [be.downloadImage(fp.image("shadow%d" % i), 0, np.uint16).reshape(RES, RES).copy() for i in range(4)]


_reference_cache = {}


def _reference(info_bytes, cascade, draws_key):
    """the reference for one cascade under the downloaded matrices; shared between the modes when the matrices agree"""
    s, i = sc.mesh_scene(), _scene_inputs()
    key = (bytes(info_bytes[16 + 64 * cascade:16 + 64 * (cascade + 1)]), draws_key)
    if key not in _reference_cache:
        draws = s["draws"] if draws_key == "first" else i["moved"]
        _reference_cache[key] = sc.rasterise(sc.mesh_case(ref.light_matrices(info_bytes)[cascade], RES, draws))
    return _reference_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frame_rasterises_the_casters_into_the_cascades(backend, fast):
    s, i = sc.mesh_scene(), _scene_inputs()
    backend.setMathMode(fast)
    fp = None
    try:
        fp = _pipeline(backend)
        assert fp.shadow_raster_stats(0) == (0, 0, 0), "no frame yet"
        fp.set_shadow_casters(s["meshes"], s["draws"])
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        general = backend.getGeneralKernelExecutions()
        info = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
        first = _maps(backend, fp)
        drawn = 0
        for c in range(3):
            r = _reference(info, c, "first")
            differing = int((first[c] != r["map"]).sum())
            print("shadow frame %s cascade %d: %d of %d texels differ, %d texels covered, counters %r" % ("fast" if fast else "exact", c, differing, RES * RES, int((r["map"] > 0).sum()), fp.shadow_raster_stats(c)))
            assert differing == 0
            assert fp.shadow_raster_stats(c) == (r["submitted"], r["drawn"], r["rejects"])
            drawn += r["drawn"]
        assert drawn > 0 and any(m.any() for m in first[:3]), "the casters lie in no cascade: the test would compare cleared maps"
        assert np.array_equal(first[3], i["patterns"][3]), "shadow3 lies above the cascade count and was written"
        if fast:
            assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)

        # new transforms: applied in call order in front of the next frame
        fp.set_shadow_caster_transforms([t for _, t in i["moved"]])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        info2 = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
        second = _maps(backend, fp)
        for c in range(3):
            assert np.array_equal(second[c], _reference(info2, c, "moved")["map"])
        assert any(not np.array_equal(second[c], first[c]) for c in range(3)), "the shadow did not move"

        # draw_count 0: nothing is recorded any more, an uploaded map stays
        fp.set_shadow_casters([], [])
        backend.uploadImage(fp.image("shadow0"), i["patterns"][0])
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        assert np.array_equal(_maps(backend, fp)[0], i["patterns"][0])
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


EMPTY_MESH = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.zeros(0, np.uint32))  # three vertices and no index


def replacement_scene():
    """the second caster set of test_gpu_frame_replaces_its_casters: mesh200's three meshes and an empty one, 300 draws in front of the camera (as
    tools/shadow_raster_cost.py places its instances); every second draw names the empty mesh, the first and the last draw among them"""
    if "replacement" not in _inputs:
        s = sc.mesh_scene()
        cam = s["cam"]
        rng = np.random.default_rng(0x5245504C)
        pos, fwd = np.asarray(cam.position, np.float64), np.asarray(cam.forward, np.float64)
        right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)
        draws = []
        for k in range(300):
            d = rng.uniform(4.0, 40.0)
            at = pos + d * fwd + rng.uniform(-0.45, 0.45) * d * right + rng.uniform(-0.2, 0.2) * d * up
            scale = rng.uniform(0.5, 1.5, 3) * (0.15 + d / 40.0)
            draws.append((3 if k % 2 == 0 or k == 299 else (k // 2) % 3, sc.affine(scale, rng.uniform(0, 6.28), rng.uniform(-1.0, 1.0), at)))
        _inputs["replacement"] = (list(s["meshes"]) + [EMPTY_MESH], draws)
    return _inputs["replacement"]


def test_replacement_scene_is_what_it_is_for():
    """not gpu: more than 256 draws (a second chunk of the draw lookup), empty draws at both ends and in between, and - under the light matrices the CPU fits to the
    smoke camera, close to those the frame downloads - triangles drawn in every cascade"""
    s = sc.mesh_scene()
    meshes, draws = replacement_scene()
    pos, idx, dr, tr = ref.merge_meshes(meshes, draws)
    assert dr.shape == (300, 4) and dr[0, 1] == 0 and dr[-1, 1] == 0 and int((dr[:, 1] == 0).sum()) == 151 and int((dr[256:, 1] > 0).sum()) > 10
    assert pos.shape[0] == sum(m[0].shape[0] for m in s["meshes"]) + 3 and idx.size == sum(m[1].size for m in s["meshes"])
    for c in range(3):
        r = ref.rasterise(ref.light_matrices(s["info"])[c], tr, pos, idx, dr, RES)
        assert r["submitted"] == int((dr[:, 1] // 3).sum()) and r["drawn"] > 100 and r["map"].any()


@pytest.mark.gpu
def test_gpu_frame_replaces_its_casters(backend):
    """three draws, then 300 draws over four meshes (the caster buffers grow into new handles, the scratch buffers are resized), then one draw (the buffers are
    kept and larger than needed: the vertex, index and transform counts the launcher derives from their sizes exceed the scene's). After each replacement a frame's
    cascades equal the reference under the downloaded light matrices and the stats agree."""
    s, i = sc.mesh_scene(), _scene_inputs()
    many_meshes, many_draws = replacement_scene()
    fp = _pipeline(backend)
    try:
        steps = (("three draws", s["meshes"], s["draws"]), ("300 draws", many_meshes, many_draws), ("one draw", s["meshes"][1:2], [(0, s["draws"][1][1])]))
        for f, (what, meshes, draws) in enumerate(steps):
            fp.set_shadow_casters(meshes, draws)
            fp.frame(i["cams"][1 + f % 2], 1.0 / 60.0, 0.5 + f / 60.0)
            info = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
            maps = _maps(backend, fp)
            pos, idx, dr, tr = ref.merge_meshes(meshes, draws)
            drawn = 0
            for c in range(3):
                r = ref.rasterise(ref.light_matrices(info)[c], tr, pos, idx, dr, RES)
                differing = int((maps[c] != r["map"]).sum())
                print("shadow frame, %s, cascade %d: %d of %d texels differ, %d texels covered, counters %r (reference %r)"
                      % (what, c, differing, RES * RES, int((r["map"] > 0).sum()), fp.shadow_raster_stats(c), (r["submitted"], r["drawn"], r["rejects"])))
                assert differing == 0, what
                assert fp.shadow_raster_stats(c) == (r["submitted"], r["drawn"], r["rejects"]), what
                drawn += r["drawn"]
            assert drawn > 0 and any(m.any() for m in maps[:3]), "the casters lie in no cascade: the test would compare cleared maps"
            assert np.array_equal(maps[3], i["patterns"][3]), "shadow3 lies above the cascade count and was written"
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_pipeline_without_casters_keeps_the_uploaded_maps(backend):
    i = _scene_inputs()
    fp = _pipeline(backend)
    try:
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        for m, pattern in zip(_maps(backend, fp), i["patterns"]):
            assert np.array_equal(m, pattern)
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_casters_survive_a_resize(backend):
    """live resize keeps the shadow maps and the casters: the next frame's maps equal the reference under the matrices fitted at the new size"""
    s, i = sc.mesh_scene(), _scene_inputs()
    fp = _pipeline(backend)
    try:
        fp.set_shadow_casters(s["meshes"], s["draws"])
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        fp.set_resolution(64, 40)
        fp.apply_changes()
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        info = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
        maps = _maps(backend, fp)
        for c in range(3):
            r = sc.rasterise(sc.mesh_case(ref.light_matrices(info)[c], RES))
            assert np.array_equal(maps[c], r["map"])
        assert np.array_equal(maps[3], i["patterns"][3])
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    s, i = sc.mesh_scene(), _scene_inputs()
    fp = _pipeline(backend)
    try:
        def refused(call, code, *words):
            with pytest.raises(PlrError) as e:
                call()
            assert e.value.code == code, e.value
            assert all(w in str(e.value) for w in words), e.value

        refused(lambda: fp.set_shadow_casters(s["meshes"], [(3, sc.IDENTITY)]), INVALID_ARGUMENT, "mesh index", "draw 0")
        pos, idx = s["meshes"][0]
        bad = idx.copy()
        bad[7] = pos.shape[0]
        refused(lambda: fp.set_shadow_casters([(pos, bad)], [(0, sc.IDENTITY)]), INVALID_ARGUMENT, "vertex index", "index 7")
        projective = sc.IDENTITY.copy()
        projective[11] = 0.01
        refused(lambda: fp.set_shadow_casters(s["meshes"], [(0, projective)]), INVALID_ARGUMENT, "affine")
        # nothing was set by the refused calls: a frame records no cascade and the uploaded maps stay
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        assert all(fp.shadow_raster_stats(c) == (0, 0, 0) for c in range(3))
        for m, pattern in zip(_maps(backend, fp), i["patterns"]):
            assert np.array_equal(m, pattern)
        fp.set_shadow_casters(s["meshes"], s["draws"])
        refused(lambda: fp.set_shadow_caster_transforms([sc.IDENTITY, sc.IDENTITY]), INVALID_ARGUMENT, "transform count", "2", "3")
        refused(lambda: fp.set_shadow_caster_transforms([sc.IDENTITY, projective, sc.IDENTITY]), INVALID_ARGUMENT, "affine", "draw 1")
        refused(lambda: fp.shadow_raster_stats(3), INVALID_ARGUMENT, "cascade")
        refused(lambda: fp.set_shadow_casters(s["meshes"], [(3, sc.IDENTITY)]), INVALID_ARGUMENT, "mesh index")
        refused(lambda: fp.set_shadow_casters(s["meshes"], [s["draws"][0], (1, projective)]), INVALID_ARGUMENT, "affine", "draw 1")
        # the casters set before the refusals are the ones the next frame draws
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        info = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
        maps = _maps(backend, fp)
        drawn = 0
        for c in range(3):
            r = _reference(info, c, "first")
            assert np.array_equal(maps[c], r["map"]), "after refused calls, cascade %d" % c
            assert fp.shadow_raster_stats(c) == (r["submitted"], r["drawn"], r["rejects"])
            drawn += r["drawn"]
        assert drawn > 0
        assert np.array_equal(maps[3], i["patterns"][3])
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_shadow_casters(s["meshes"], s["draws"])
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
