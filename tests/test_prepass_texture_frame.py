"""Material textures in the frame pipeline (plrf_set_scene_textures): 96 x 64, the three meshes of the shadow tests' scene with the generators' UVs, a moving
camera and TAA jitter.

Every frame's albedo and specular must equal tests/prepass_texture_reference.py for the MainPassMatrices buffer downloaded from the pipeline and the jitters and
mipBias of the submitted global block; depth, motion and normal must equal the same frames of a pipeline without textures. Removing the textures
(texture_count 0) and plrf_set_scene_meshes both restore the constant words; textures survive a resize and a transform update; a host-built chain (mip_count 0)
equals the same chain supplied by the caller; every refusal names its cause and leaves the next frame unchanged; a band pipeline refuses.
"""
import copy

import numpy as np
import pytest

import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
import shadow_raster_cases as sc
from plainrenderer_amd.scene import Camera

W, H, RES = 96, 64, 128
FP_ARGS = dict(shadow_map_res=RES, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64)
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
FRAMES = 3
NONE = tref.NONE

_inputs = {}
_expected_cache = {}


def _scene_inputs():
    """generated once for the module; never modified"""
    if not _inputs:
        from plainrenderer_amd import meshes
        from plainrenderer_amd.frame import SyntheticInputs
        s = sc.mesh_scene()
        cams = [Camera.look((15.0 + 0.03 * i, -7.0 + 0.01 * i, -6.0 + 0.05 * i), (0.002 * i, 0.16, 1.0), aspect=W / H) for i in range(FRAMES + 2)]
        inp = SyntheticInputs(s["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45))
        raw = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_uvs=True), meshes.uv_sphere(1.25, segments=28, rings=14, with_uvs=True),
               meshes.torus(1.5, 0.5, segments=24, sides=12, with_uvs=True)]
        ms = [pc.mesh_arrays(raw[0], False), pc.mesh_arrays(raw[1], True), pc.mesh_arrays(raw[2], True)]
        uvs = [np.asarray(m[2], np.float32) * np.float32(scale) for m, scale in zip(raw, (1.0, 3.0, 2.0))]  # the sphere and the torus repeat theirs
        models = [np.asarray(t, np.float32).copy() for _, t in s["draws"]]
        # 16 x 16 with the full chain; 8 x 4 with its first two levels; 5 x 3, level 0 alone
        chains = [(tc.chain(tc.pattern(16, 16, 31), 16, 16), 16, 16, 5), (tc.chain(tc.pattern(8, 4, 32), 8, 4, 2), 8, 4, 2), (tc.pattern(5, 3, 33), 5, 3, 1)]
        _inputs.update(inp=inp, cams=cams, meshes=ms, uvs=uvs, mesh_of=[m for m, _ in s["draws"]], models=models, chains=chains,
                       materials=[(0, 1), (NONE, 2), (1, NONE)])
    return _inputs


def _draws(models):
    return [(m, t, *pc.material(d)) for d, (m, t) in enumerate(zip(_scene_inputs()["mesh_of"], models))]


def _pipeline(be, **extra):
    from plainrenderer_amd.frame import FramePipeline
    fp = FramePipeline(be, W, H, **dict(FP_ARGS, **extra))
    copy.copy(_scene_inputs()["inp"]).upload(fp)
    return fp


def _set_textures(fp, host_built_first=True, materials=None):
    """the module's three textures; host_built_first: texture 0 as level 0 with mip_count 0 (the host builds the chain) instead of the whole chain"""
    i = _scene_inputs()
    textures = list(i["chains"])
    if host_built_first:
        textures[0] = (textures[0][0][:256], 16, 16, 0)
    fp.set_scene_textures(textures, i["uvs"], i["materials"] if materials is None else materials)


def _expected(be, fp, textured=True, width=W, height=H, materials=None):
    """(case, rasterise result, sample result or None) for the frame the pipeline just rendered, from ITS matrices, jitters and mipBias"""
    i = _scene_inputs()
    n = len(i["mesh_of"])
    matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192 * n, dtype=np.float32).reshape(n, 48).copy()
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    key = (matrices.tobytes(), g[64:68].tobytes(), width, height)
    if key not in _expected_cache:
        pos, nrm, idx, draws, _ = pc.merge_meshes(i["meshes"], [(m, pc.IDENTITY) for m in i["mesh_of"]])
        case = pc.make_case(width, height, matrices, pos, idx, draws, nrm, tuple(float(v) for v in g[64:66]), tuple(float(v) for v in g[66:68]))
        _expected_cache[key] = (case, pc.rasterise(case))
    case, r = _expected_cache[key]
    if not textured:
        return case, r, None
    tex = tc.textured(case, np.concatenate(i["uvs"]), i["materials"] if materials is None else materials, list(i["chains"]), mip_bias=float(g[79]))[1]
    return case, r, tref.sample(case, tex, r["keys"])


def _g_buffer(be, fp, target, width=W, height=H):
    names = dict(depth="depth%d" % target, motion="motion%d" % target, normal="normal", albedo="albedo", specular="specular")
    return {k: be.downloadImage(fp.image(v), 0, np.uint32).reshape(height, width).copy() for k, v in names.items()}


def _assert_materials(label, got, want_albedo, want_specular):
    differing = {"albedo": int((got["albedo"] != want_albedo).sum()), "specular": int((got["specular"] != want_specular).sum())}
    print("prepass texture frame %-40s: texels that differ %r of %d" % (label, differing, got["albedo"].size))
    assert differing == {"albedo": 0, "specular": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frames_sample_the_textures_and_leave_the_rest_alone(backend, fast):
    i = _scene_inputs()
    backend.setMathMode(fast)
    fp = None
    try:
        # the frames without textures first
        fp = _pipeline(backend)
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        untextured = []
        for k in range(FRAMES):
            fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            case, r, _ = _expected(backend, fp, textured=False)
            untextured.append((_g_buffer(backend, fp, (k + 1) % 2), fp.prepass_raster_stats()))
            assert np.array_equal(untextured[k][0]["albedo"], r["albedo"]) and np.array_equal(untextured[k][0]["specular"], r["specular"])
        fp.destroy()
        fp = _pipeline(backend)
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        _set_textures(fp)
        biases, sampled = set(), 0
        for k in range(FRAMES):
            fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            general = backend.getGeneralKernelExecutions()
            got = _g_buffer(backend, fp, (k + 1) % 2)
            case, r, s = _expected(backend, fp)
            g = np.frombuffer(fp.submitted_globals(), np.float32)
            biases.add(float(g[79]))
            assert g[64:68].any(), "the TAA jitter is on"
            _assert_materials("%s frame %d" % ("fast" if fast else "exact", k), got, s["albedo"], s["specular"])
            for name in ("depth", "motion", "normal"):
                assert np.array_equal(got[name], untextured[k][0][name]), "%s of frame %d differs from the frame without textures" % (name, k)
            assert fp.prepass_raster_stats() == untextured[k][1] == (r["submitted"], r["clipped"], r["drawn"], r["rejects"])
            sampled += int((s["albedo"] != r["albedo"]).sum())
            if fast:
                assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
        print("prepass texture frame: mipBias of the frames %r, %d albedo texels differ from the constant words" % (sorted(biases), sampled))
        assert sampled > 500
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_textures_removed_dropped_kept_and_host_built(backend):
    i = _scene_inputs()
    fp = _pipeline(backend)
    try:
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        _set_textures(fp, host_built_first=True)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        case, r, s = _expected(backend, fp)
        host_built = _g_buffer(backend, fp, 1)
        _assert_materials("host-built chain", host_built, s["albedo"], s["specular"])
        assert (s["albedo"] != r["albedo"]).sum() > 200
        # texture_count 0: the constant words again
        fp.set_scene_textures([], [], [])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        case, r, _ = _expected(backend, fp, textured=False)
        _assert_materials("textures removed", _g_buffer(backend, fp, 0), r["albedo"], r["specular"])
        # set again, the chain of texture 0 supplied by the caller
        _set_textures(fp, host_built_first=False)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        case, r, s = _expected(backend, fp)
        supplied = _g_buffer(backend, fp, 1)
        _assert_materials("caller-supplied chain", supplied, s["albedo"], s["specular"])
        # plrf_set_scene_meshes drops them, the same scene given again included
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        case, r, _ = _expected(backend, fp, textured=False)
        _assert_materials("after plrf_set_scene_meshes", _g_buffer(backend, fp, 0), r["albedo"], r["specular"])
        # they survive a transform update and a resize
        _set_textures(fp)
        models = [m.copy() for m in i["models"]]
        models[1][12:15] += np.asarray(sc.mesh_scene()["cam"].right, np.float32) * np.float32(0.4)
        fp.set_scene_mesh_transforms(models)
        fp.set_resolution(70, 50)
        fp.apply_changes()
        cam = Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50)
        fp.frame(cam, 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        case, r, s = _expected(backend, fp, width=70, height=50)
        _assert_materials("after a transform update and a resize to 70 x 50", _g_buffer(backend, fp, 1, 70, 50), s["albedo"], s["specular"])
        assert (s["albedo"] != r["albedo"]).sum() > 100
    finally:
        fp.destroy()


def test_the_two_texture_sets_of_the_frame_test_hold_one_chain():
    """not gpu: what the frame test's two texture sets are - level 0 of texture 0 alone, and its chain by the rule"""
    i = _scene_inputs()
    assert np.array_equal(tref.build_chain(i["chains"][0][0][:256], 16, 16), i["chains"][0][0]) and i["chains"][0][0].size == 341


@pytest.mark.gpu
def test_gpu_host_built_and_supplied_chains_give_the_same_frame(backend):
    i = _scene_inputs()
    images = []
    for host_built in (True, False):
        fp = _pipeline(backend)
        try:
            fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
            _set_textures(fp, host_built_first=host_built, materials=[(0, 0), (0, 0), (0, 0)])
            fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
            images.append(_g_buffer(backend, fp, 1))
            if host_built:
                case, r, s = _expected(backend, fp, materials=[(0, 0), (0, 0), (0, 0)])
                _assert_materials("every draw samples the host-built chain", images[0], s["albedo"], s["specular"])
        finally:
            fp.destroy()
    for name in images[0]:
        assert np.array_equal(images[0][name], images[1][name]), name


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_change_nothing(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    i = _scene_inputs()
    fp = _pipeline(backend)
    try:
        def refused(call, code, *words):
            with pytest.raises(PlrError) as e:
                call()
            assert e.value.code == code, e.value
            assert all(w in str(e.value) for w in words), e.value

        chains, uvs, materials = list(i["chains"]), i["uvs"], i["materials"]
        refused(lambda: fp.set_scene_textures(chains, uvs, materials), INVALID_ARGUMENT, "no scene set")
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        _set_textures(fp)
        refused(lambda: fp.set_scene_textures(chains, uvs[:2], materials), INVALID_ARGUMENT, "mesh count 2", "mesh count 3")
        refused(lambda: fp.set_scene_textures(chains, uvs, materials + [(0, 0)]), INVALID_ARGUMENT, "draw count 4", "draw count 3")
        one = np.zeros(1, np.uint32)
        refused(lambda: fp.set_scene_textures([(one, 0, 4, 1)] + chains[1:], uvs, materials), INVALID_ARGUMENT, "texture size", "texture 0", "0 x 4")
        refused(lambda: fp.set_scene_textures(chains[:2] + [(one, 5, 16385, 1)], uvs, materials), INVALID_ARGUMENT, "texture size", "texture 2", "16385")
        refused(lambda: fp.set_scene_textures([chains[0], (chains[1][0], 8, 4, 5), chains[2]], uvs, materials), INVALID_ARGUMENT, "too many mips", "texture 1", "at most 4")
        refused(lambda: fp.set_scene_textures([chains[0], (np.zeros(0, np.uint32), 1, 1, 0), chains[2]], uvs, materials), INVALID_ARGUMENT, "null texels", "texture 1")
        refused(lambda: fp.set_scene_textures(chains, uvs, [(0, 1), (3, 2), (1, NONE)]), INVALID_ARGUMENT, "material texture index", "draw 1", "texture 3 of 3")
        def too_many():  # at the C boundary: sizes are refused before a texel is read, so one texel stands in for 2^28
            import ctypes as C
            from plainrenderer_amd.frame import PlrfSceneMaterial, PlrfSceneTexture
            pointer = one.ctypes.data_as(C.POINTER(C.c_uint32))
            t = (PlrfSceneTexture * 2)(PlrfSceneTexture(pointer, 16384, 16384, 1), PlrfSceneTexture(pointer, 1, 1, 1))
            fp._check(fp.lib.plrf_set_scene_textures(fp.handle, t, C.c_uint32(2), None, C.c_uint32(3), (PlrfSceneMaterial * 3)(), C.c_uint32(3)))
        refused(too_many, INVALID_ARGUMENT, "too many texels", "268435457")
        bad = [u.copy() for u in uvs]
        bad[2][7, 1] = np.nan
        refused(lambda: fp.set_scene_textures(chains, bad, materials), INVALID_ARGUMENT, "non-finite UV", "vertex 7 of mesh 2")
        # the textures set before the refusals are the ones the next frame samples
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        case, r, s = _expected(backend, fp)
        _assert_materials("after refused calls", _g_buffer(backend, fp, 1), s["albedo"], s["specular"])
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_textures(list(i["chains"]), i["uvs"], i["materials"])
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
