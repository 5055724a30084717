"""Alpha-tested cutouts in the frame pipeline (plrf_set_scene_alpha_cutoffs): 96 x 64, an opaque wall behind three double-sided cards with checker alphas, a moving
camera and TAA jitter.

Every frame's five G-buffer images and the four counters must equal tests/prepass_alpha_reference.py for the MainPassMatrices buffer downloaded from the
pipeline and the jitters and mipBias of the submitted global block. Removing the cutoffs and setting all of them to 0 give the textured frame bit for bit;
plrf_set_scene_meshes and plrf_set_scene_textures drop them; they survive a transform update, a resize and a settings update; every refusal names its cause and
leaves the next frame unchanged; a band pipeline refuses.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import prepass_alpha_cases as ac
import prepass_alpha_reference as aref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
import shadow_raster_cases as sc
import test_prepass_raster as tpr
from plainrenderer_amd.scene import Camera

W, H, RES = 96, 64, 128
FP_ARGS = dict(shadow_map_res=RES, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64)
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
FRAMES = 3
NONE = tref.NONE
CUTOFFS = [0, 128, 160, 100]

# a double-sided card in the XY plane, its UVs repeating twice
CARD = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), None, np.array([0, 1, 2, 0, 2, 3, 0, 2, 1, 0, 3, 2], np.uint32))
CARD_UVS = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.float32)
EYE, FORWARD = np.array([15.0, -7.0, -6.0]), np.array([0.0, 0.16, 1.0]) / np.linalg.norm([0.0, 0.16, 1.0])

_inputs = {}


def _model(distance, scale, dx, dy):
    m = np.eye(4)
    m[0, 0] = m[1, 1] = m[2, 2] = scale
    m[:3, 3] = EYE + FORWARD * distance + np.array([dx, dy, 0.0])
    return pc.glm(m)


def _cameras():
    return [Camera.look((15.0 + 0.03 * i, -7.0 + 0.01 * i, -6.0 + 0.05 * i), (0.002 * i, 0.16, 1.0), aspect=W / H) for i in range(FRAMES + 2)]


def _scene():
    """the wall and the three cards; built once, never modified"""
    if "scene" not in _inputs:
        models = [_model(14.0, 6.0, 0.0, 0.0), _model(10.0, 2.2, -1.0, 0.1), _model(8.0, 1.5, 1.2, -0.2), _model(6.0, 0.8, 0.3, 0.2)]
        chains = [(tc.chain(ac.checker(8, 8, 2, 61), 8, 8), 8, 8, 4), (tc.chain(ac.checker(16, 16, 2, 62, phase=1), 16, 16), 16, 16, 5), (tc.chain(ac.checker(4, 4, 1, 63), 4, 4), 4, 4, 3),
                  (tc.chain(tc.pattern(8, 8, 64), 8, 8), 8, 8, 4)]
        _inputs["scene"] = dict(meshes=[CARD], uvs=[CARD_UVS], mesh_of=[0, 0, 0, 0], models=models, chains=chains, materials=[(3, NONE), (0, 3), (1, NONE), (2, 3)])
    return _inputs["scene"]


def _synthetic():
    if "inp" not in _inputs:
        from plainrenderer_amd.frame import SyntheticInputs
        cams = _cameras()
        _inputs["inp"] = SyntheticInputs(sc.mesh_scene()["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45))
    return _inputs["inp"]


def _draws(models):
    return [(m, t, *pc.material(d)) for d, (m, t) in enumerate(zip(_scene()["mesh_of"], models))]


def _case(matrices, width, height, jitter_current=(0.0, 0.0), jitter_previous=(0.0, 0.0)):
    i = _scene()
    pos, nrm, idx, draws, _ = pc.merge_meshes(i["meshes"], [(m, pc.IDENTITY) for m in i["mesh_of"]])
    return pc.make_case(width, height, matrices, pos, idx, draws, nrm, jitter_current, jitter_previous)


def _textures_of(case, mip_bias):
    i = _scene()
    return tc.textured(case, np.concatenate(i["uvs"]), i["materials"], list(i["chains"]), mip_bias=mip_bias)[1]


def test_the_cutouts_of_the_frame_test_show():
    """not gpu: under the first camera's own matrices every card wins pixels, loses fragments, and the wall and a card behind show through the holes"""
    i = _scene()
    cam = _cameras()[1]
    vp = np.asarray(cam.view_projection(), np.float32).reshape(16)
    import prepass_raster_reference as ref
    case = _case(ref.main_pass_matrices(vp, vp, i["models"]), W, H)
    tex = _textures_of(case, 0.0)
    a = aref.render(case, tex, CUTOFFS)
    opaque = pc.rasterise(case)
    own, untested = aref.winner_draw(case, a["keys"]), aref.winner_draw(case, opaque["keys"])
    assert all((own == d).sum() > 40 for d in range(4)), [int((own == d).sum()) for d in range(4)]
    for d in (1, 2, 3):
        holes = (untested == d) & (own != d)
        assert holes.sum() > 30, "card %d loses fragments" % d
    assert ((untested == 3) & (own == 0)).sum() + ((untested == 2) & (own == 0)).sum() + ((untested == 1) & (own == 0)).sum() > 50, "the wall shows through"
    assert ((untested > 1) & (own >= 1) & (own < untested)).sum() > 10, "a card shows through a nearer one"


def _pipeline(be, **extra):
    from plainrenderer_amd.frame import FramePipeline
    fp = FramePipeline(be, W, H, **dict(FP_ARGS, **extra))
    copy.copy(_synthetic()).upload(fp)
    return fp


def _set_scene(fp, textures=True, cutoffs=None):
    i = _scene()
    fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
    if textures:
        fp.set_scene_textures(list(i["chains"]), i["uvs"], i["materials"])
    if cutoffs is not None:
        fp.set_scene_alpha_cutoffs(cutoffs)


def _expected(be, fp, cutoffs, textured=True, width=W, height=H):
    """the reference for the frame the pipeline just rendered, from ITS matrices, jitters and mipBias. cutoffs None: the frame without the test"""
    n = len(_scene()["mesh_of"])
    matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192 * n, dtype=np.float32).reshape(n, 48).copy()
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    case = _case(matrices, width, height, tuple(float(v) for v in g[64:66]), tuple(float(v) for v in g[66:68]))
    if not textured:
        return pc.rasterise(case)
    tex = _textures_of(case, float(g[79]))
    if cutoffs is None:
        r = pc.rasterise(case)
        s = tref.sample(case, tex, r["keys"])
        return dict(r, albedo=s["albedo"], specular=s["specular"])
    return aref.render(case, tex, cutoffs)


def _g_buffer(be, fp, target, width=W, height=H):
    names = dict(depth="depth%d" % target, motion="motion%d" % target, normal="normal", albedo="albedo", specular="specular")
    return {k: be.downloadImage(fp.image(v), 0, np.uint32).reshape(height, width).copy() for k, v in names.items()}


def _compare(label, be, fp, target, want, width=W, height=H):
    tpr.compare("alpha frame " + label, _g_buffer(be, fp, target, width, height), fp.prepass_raster_stats(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frames_with_cutoffs_equal_the_reference(backend, fast):
    cams = _cameras()
    backend.setMathMode(fast)
    fp = None
    try:
        fp = _pipeline(backend)
        _set_scene(fp, cutoffs=CUTOFFS)
        holes = 0
        for k in range(FRAMES):
            fp.frame(cams[k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            general = backend.getGeneralKernelExecutions()
            g = np.frombuffer(fp.submitted_globals(), np.float32)
            assert g[64:68].any(), "the TAA jitter is on"
            want = _expected(backend, fp, CUTOFFS)
            _compare("%s frame %d" % ("fast" if fast else "exact", k), backend, fp, (k + 1) % 2, want)
            holes += int((want["depth"] != _expected(backend, fp, None)["depth"]).sum())
            if fast:
                assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
        print("prepass alpha frame: %d pixels of %d frames see through a cutout" % (holes, FRAMES))
        assert holes > 300
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_cutoffs_removed_zeroed_dropped_and_kept(backend):
    cams = _cameras()
    i = _scene()
    fp = _pipeline(backend)
    try:
        _set_scene(fp, cutoffs=CUTOFFS)
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        _compare("with cutoffs", backend, fp, 1, _expected(backend, fp, CUTOFFS))
        # removed: the textured frame, bit for bit
        fp.set_scene_alpha_cutoffs([])
        fp.frame(cams[2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        _compare("cutoffs removed", backend, fp, 0, _expected(backend, fp, None))
        # all 0: the same
        fp.set_scene_alpha_cutoffs(CUTOFFS)
        fp.set_scene_alpha_cutoffs([0, 0, 0, 0])
        fp.frame(cams[1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        _compare("all cutoffs 0", backend, fp, 1, _expected(backend, fp, None))
        # plrf_set_scene_textures drops them, the same textures given again included
        fp.set_scene_alpha_cutoffs(CUTOFFS)
        fp.set_scene_textures(list(i["chains"]), i["uvs"], i["materials"])
        fp.frame(cams[2], 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        _compare("after plrf_set_scene_textures", backend, fp, 0, _expected(backend, fp, None))
        # plrf_set_scene_meshes drops them (and the textures)
        fp.set_scene_alpha_cutoffs(CUTOFFS)
        fp.set_scene_meshes(i["meshes"], _draws(i["models"]))
        fp.frame(cams[1], 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        _compare("after plrf_set_scene_meshes", backend, fp, 1, _expected(backend, fp, None, textured=False))
        fp.set_scene_textures(list(i["chains"]), i["uvs"], i["materials"])
        fp.frame(cams[2], 1.0 / 60.0, 0.5 + 5.0 / 60.0)
        _compare("textures again, no cutoffs", backend, fp, 0, _expected(backend, fp, None))
        # they survive a transform update, a resize and a settings update
        fp.set_scene_alpha_cutoffs(CUTOFFS)
        models = [m.copy() for m in i["models"]]
        models[2][12] += np.float32(0.4)
        fp.set_scene_mesh_transforms(models)
        fp.set_resolution(70, 50)
        fp.update_settings(bloom_strength=0.2)
        fp.apply_changes()
        cam = Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50)
        fp.frame(cam, 1.0 / 60.0, 0.5 + 6.0 / 60.0)
        want = _expected(backend, fp, CUTOFFS, width=70, height=50)
        _compare("after a transform update, a resize to 70 x 50 and a settings update", backend, fp, 1, want, 70, 50)
        assert (want["depth"] != _expected(backend, fp, None, width=70, height=50)["depth"]).sum() > 50
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_change_nothing(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    cams = _cameras()
    i = _scene()
    fp = _pipeline(backend)
    try:
        def refused(call, code, *words):
            with pytest.raises(PlrError) as e:
                call()
            assert e.value.code == code, e.value
            assert all(w in str(e.value) for w in words), e.value

        refused(lambda: fp.set_scene_alpha_cutoffs(CUTOFFS), INVALID_ARGUMENT, "no scene set")
        _set_scene(fp, textures=False)
        refused(lambda: fp.set_scene_alpha_cutoffs(CUTOFFS), INVALID_ARGUMENT, "no textures set")
        _set_scene(fp, cutoffs=CUTOFFS)
        refused(lambda: fp.set_scene_alpha_cutoffs(CUTOFFS[:3]), INVALID_ARGUMENT, "cutoff count 3", "draw count 4")
        refused(lambda: fp.set_scene_alpha_cutoffs(CUTOFFS + [0]), INVALID_ARGUMENT, "cutoff count 5", "draw count 4")
        refused(lambda: fp.set_scene_alpha_cutoffs([0, 0, 256, 0]), INVALID_ARGUMENT, "cutoff out of range", "draw 2", "256")
        refused(lambda: fp._check(fp.lib.plrf_set_scene_alpha_cutoffs(fp.handle, None, C.c_uint32(4))), INVALID_ARGUMENT, "cutoffs are null")
        # the cutoffs set before the refusals are the ones the next frame tests with
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        _compare("after refused calls", backend, fp, 1, _expected(backend, fp, CUTOFFS))
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_alpha_cutoffs(CUTOFFS)
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
