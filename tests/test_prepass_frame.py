"""Scene meshes in the frame pipeline (plrf_set_scene_meshes): 96 x 54, the meshes of the shadow tests' scene in front of its camera path.

A pipeline with scene meshes must write, every frame, the five G-buffer images tests/prepass_raster_reference.py gives for the MainPassMatrices buffer DOWNLOADED
from the pipeline and the jitters of the submitted global block; those matrices are separately held to the numpy product of the submitted viewProjection /
viewProjectionPrevious and the model matrices. A second pipeline without scene meshes that gets the reference's five images uploaded in front of every frame, on
the same camera path, must produce byte-identical colour, post-process and swapchain images, in both kernel sets. A scene replaced mid-run gives the new
reference in the next frame; a scene removed leaves the uploaded G-buffer alone; a resize needs no re-upload; with shadow casters and run_light_matrix the cascades
follow the depth the prepass made; the SDF debug view still records the prepass; every refusal names its cause and changes nothing.
"""
import copy

import numpy as np
import pytest

import prepass_raster_cases as pc
import prepass_raster_reference as ref
import shadow_raster_cases as sc
import shadow_raster_reference as shadow_ref
from plainrenderer_amd.scene import Camera

W, H, RES = 96, 54, 128
FP_ARGS = dict(shadow_map_res=RES, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64)
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
FRAMES = 4
G_BUFFER = ("depth", "motion", "normal", "albedo", "specular")

_inputs = {}


def _scene_inputs():
    """generated once for the module; never modified"""
    if not _inputs:
        from plainrenderer_amd.frame import SyntheticInputs
        s = sc.mesh_scene()
        cams = [Camera.look((15.0 + 0.03 * i, -7.0 + 0.01 * i, -6.0 + 0.05 * i), (0.002 * i, 0.16, 1.0), aspect=W / H) for i in range(FRAMES + 1)]
        inp = SyntheticInputs(s["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45))
        meshes = [pc.mesh_arrays(s["meshes"][0], False), pc.mesh_arrays(s["meshes"][1], True), pc.mesh_arrays(s["meshes"][2], True)]
        models = [np.asarray(t, np.float32).copy() for _, t in s["draws"]]
        right = np.asarray(s["cam"].right, np.float32)
        path = []  # per frame: the model matrices; draw 1 moves
        for k in range(FRAMES + 1):
            now = [m.copy() for m in models]
            now[1][12:15] += right * np.float32(0.2 * k)
            path.append(now)
        _inputs.update(inp=inp, cams=cams, meshes=meshes, mesh_of=[m for m, _ in s["draws"]], path=path)
    return _inputs


def _draws(models, mesh_of=None):
    mesh_of = mesh_of if mesh_of is not None else _scene_inputs()["mesh_of"]
    return [(m, t, *pc.material(d)) for d, (m, t) in enumerate(zip(mesh_of, models))]


def _pipeline(be, **extra):
    from plainrenderer_amd.frame import FramePipeline
    fp = FramePipeline(be, W, H, **dict(FP_ARGS, **extra))
    inp = copy.copy(_scene_inputs()["inp"])
    inp.upload(fp)
    return fp


def _jitters(fp):
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    return tuple(float(v) for v in g[64:66]), tuple(float(v) for v in g[66:68])


def _expected(be, fp, meshes, mesh_of, width=W, height=H):
    """the reference's result for the frame the pipeline just rendered, from ITS matrices and jitters"""
    n = len(mesh_of)
    matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192 * n, dtype=np.float32).reshape(n, 48).copy()
    pos, nrm, idx, draws, _ = pc.merge_meshes(meshes, [(m, pc.IDENTITY) for m in mesh_of])
    current, previous = _jitters(fp)
    return matrices, pc.rasterise(pc.make_case(width, height, matrices, pos, idx, draws, nrm, current, previous))


def _g_buffer(be, fp, target, width=W, height=H):
    names = dict(depth="depth%d" % target, motion="motion%d" % target, normal="normal", albedo="albedo", specular="specular")
    return {k: be.downloadImage(fp.image(names[k]), 0, np.uint32).reshape(height, width).copy() for k in G_BUFFER}


def _words(r):
    import test_prepass_raster as tpr
    return tpr.reference_words(r)


def _assert_g_buffer(label, got, r):
    want = _words(r)
    differing = {k: int((got[k] != want[k]).sum()) for k in G_BUFFER}
    print("prepass frame %-34s: texels that differ %r of %d, %d covered, counters %r" % (label, differing, got["depth"].size, int((r["keys"] != 0).sum()),
                                                                                          (r["submitted"], r["clipped"], r["drawn"], r["rejects"])))
    assert all(v == 0 for v in differing.values()), differing


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    scale = np.maximum(np.abs(a).max(), np.abs(b).max())  # an element is a sum of four products: its error scales with the largest of them
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / np.spacing(np.float32(scale)))


OUTPUTS = ("swapchain", "post0", "post1", "color0", "color1")


def _outputs(be, fp):
    return {n: be.downloadImage(fp.image(n), 0, np.uint8).copy() for n in OUTPUTS}


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frames_with_scene_meshes_equal_frames_with_the_reference_uploaded(backend, fast):
    i = _scene_inputs()
    backend.setMathMode(fast)
    fp = None
    try:
        fp = _pipeline(backend)
        assert fp.prepass_raster_stats() == (0, 0, 0, 0), "no frame yet"
        fp.set_scene_meshes(i["meshes"], _draws(i["path"][0]))
        expected, outputs, motion_seen = [], [], np.zeros(2, bool)
        for k in range(FRAMES):
            fp.set_scene_mesh_transforms(i["path"][k])
            fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            general = backend.getGeneralKernelExecutions()
            matrices, r = _expected(backend, fp, i["meshes"], i["mesh_of"])
            target = (k + 1) % 2  # the frame's current render target
            _assert_g_buffer("%s frame %d" % ("fast" if fast else "exact", k), _g_buffer(backend, fp, target), r)
            assert fp.prepass_raster_stats() == (r["submitted"], r["clipped"], r["drawn"], r["rejects"]) and r["drawn"] > 100
            if fast:
                assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
            # the matrices against the numpy product, from the submitted viewProjection / viewProjectionPrevious
            g = np.frombuffer(fp.submitted_globals(), np.float32)
            previous_models = i["path"][k - 1] if k else i["path"][0]
            want = ref.main_pass_matrices(g[0:16], g[16:32], i["path"][k], previous_models)
            assert np.array_equal(matrices[:, 0:16], want[:, 0:16]), "the model matrices are copied"
            assert _ulps(matrices[:, 16:32], want[:, 16:32]) <= 4 and _ulps(matrices[:, 32:48], want[:, 32:48]) <= 4, "mvp / mvpPrevious differ from viewProjection * model"
            motion_seen |= np.array([r["motion"][..., 0].any(), r["motion"][..., 1].any()])
            expected.append((target, r))
            outputs.append(_outputs(backend, fp))
        assert motion_seen.all(), "a moving camera and a moving draw give motion on both axes"
        fp.destroy()
        fp = None

        # the same frames without scene meshes, the reference's images uploaded in front of every frame
        fp = _pipeline(backend)
        for k in range(FRAMES):
            target, r = expected[k]
            words = _words(r)
            for name, image in (("depth", "depth%d" % target), ("motion", "motion%d" % target), ("normal", "normal"), ("albedo", "albedo"), ("specular", "specular")):
                backend.uploadImage(fp.image(image), words[name])
            fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            assert fp.prepass_raster_stats() == (0, 0, 0, 0)
            got = _outputs(backend, fp)
            for n in OUTPUTS:
                assert np.array_equal(got[n], outputs[k][n]), "%s of frame %d differs between the two pipelines" % (n, k)
        assert outputs[-1]["swapchain"].any() and not np.array_equal(outputs[-1]["swapchain"], outputs[0]["swapchain"])
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_scene_replaced_removed_and_resized(backend):
    i = _scene_inputs()
    fp = _pipeline(backend)
    try:
        fp.set_scene_meshes(i["meshes"], _draws(i["path"][0]))
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        _, first = _expected(backend, fp, i["meshes"], i["mesh_of"])
        _assert_g_buffer("first scene", _g_buffer(backend, fp, 1), first)
        # replaced by a larger scene (more draws, more triangles: the buffers grow), in other buffers' layout: the sphere twice and the box
        meshes2 = [i["meshes"][1], i["meshes"][2], i["meshes"][0], pc.mesh_arrays(sc.mesh_scene()["meshes"][1], False)]
        mesh_of2 = [0, 3, 1, 2, 0]
        models2 = [i["path"][2][1], i["path"][0][0], i["path"][0][2], i["path"][0][0], i["path"][0][1]]
        fp.set_scene_meshes(meshes2, _draws(models2, mesh_of2))
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        matrices, second = _expected(backend, fp, meshes2, mesh_of2)
        _assert_g_buffer("replaced scene", _g_buffer(backend, fp, 0), second)
        g = np.frombuffer(fp.submitted_globals(), np.float32)
        assert _ulps(matrices[:, 32:48], ref.main_pass_matrices(g[0:16], g[16:32], models2)[:, 32:48]) <= 4, "the first frame of a scene: the previous model matrix is the current one"
        assert second["submitted"] > first["submitted"] and fp.prepass_raster_stats()[0] == second["submitted"]
        # a resize with the scene set: no re-upload of the G-buffer, the next frame is a camera cut (previous model = current)
        models3 = [m.copy() for m in models2]
        models3[0][12:15] += np.asarray(sc.mesh_scene()["cam"].right, np.float32) * np.float32(0.5)  # draw 0 moves with the resize
        fp.set_scene_mesh_transforms(models3)
        fp.set_resolution(130, 70)
        fp.apply_changes()
        cam = Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=130 / 70)
        fp.frame(cam, 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        matrices, resized = _expected(backend, fp, meshes2, mesh_of2, 130, 70)
        _assert_g_buffer("after a resize to 130 x 70", _g_buffer(backend, fp, 1, 130, 70), resized)
        # the camera cut: mvpPrevious = viewProjectionPrevious * the CURRENT model matrices, although draw 0 moved since the last frame
        g = np.frombuffer(fp.submitted_globals(), np.float32)
        assert g[80:81].view(np.uint32)[0] == 1, "the resize made this frame a camera cut"
        assert _ulps(matrices[:, 32:48], ref.main_pass_matrices(g[0:16], g[16:32], models3)[:, 32:48]) <= 4
        assert _ulps(matrices[0, 32:48], ref.main_pass_matrices(g[0:16], g[16:32], models2)[0, 32:48]) > 1000, "the old model matrix would show"
        assert resized["drawn"] > 100
        # removed: the uploaded G-buffer is used again, nothing writes it
        fp.set_scene_meshes([], [])
        pattern = ((np.arange(130 * 70, dtype=np.uint64) * 40503 + 99) & 0xFFFFFFFF).astype(np.uint32).reshape(70, 130)
        for name in ("normal", "albedo", "specular", "depth0", "motion0"):
            backend.uploadImage(fp.image(name), pattern if name != "depth0" else (pattern & np.uint32(0x3EFFFFFF)))
        fp.frame(cam, 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        for name in ("normal", "albedo", "specular", "motion0"):
            assert np.array_equal(backend.downloadImage(fp.image(name), 0, np.uint32).reshape(70, 130), pattern), name
        assert np.array_equal(backend.downloadImage(fp.image("depth0"), 0, np.uint32).reshape(70, 130), pattern & np.uint32(0x3EFFFFFF))
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_cascades_follow_the_depth_the_prepass_made(backend):
    """scene meshes + shadow casters + run_light_matrix: lightMatrix.comp fits the cascades to the depth pyramid of the prepass' depth, and the shadow pass draws
    the casters under those matrices. With the scene pushed away from the camera the fitted matrices change"""
    i, s = _scene_inputs(), sc.mesh_scene()
    fp = _pipeline(backend, run_light_matrix=1)
    try:
        fp.set_scene_meshes(i["meshes"], _draws(i["path"][0]))
        fp.set_shadow_casters(s["meshes"], s["draws"])
        infos = []
        for k, models in enumerate((i["path"][0], None)):
            if models is None:
                forward = np.asarray(s["cam"].forward, np.float32)
                models = [m.copy() for m in i["path"][0]]
                for m in models:
                    m[12:15] += forward * np.float32(6.0)
                fp.set_scene_mesh_transforms(models)
            fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + k / 60.0)
            _, r = _expected(backend, fp, i["meshes"], i["mesh_of"])
            _assert_g_buffer("with casters, frame %d" % k, _g_buffer(backend, fp, (k + 1) % 2), r)
            info = backend.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
            for c in range(3):
                want = sc.rasterise(sc.mesh_case(shadow_ref.light_matrices(info)[c], RES))
                got = backend.downloadImage(fp.image("shadow%d" % c), 0, np.uint16).reshape(RES, RES)
                assert np.array_equal(got, want["map"]), "cascade %d in frame %d" % (c, k)
            infos.append(info)
        assert infos[0] != infos[1], "the cascade fit did not follow the prepass' depth"
        assert infos[0] != bytes(i["inp"].shadow_info), "the uploaded sunShadowInfo is still there"
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_sdf_debug_view_still_records_the_prepass(backend):
    i = _scene_inputs()
    fp = _pipeline(backend, sdf_debug_mode=1)
    try:
        fp.set_scene_meshes(i["meshes"], _draws(i["path"][0]))
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        _, r = _expected(backend, fp, i["meshes"], i["mesh_of"])
        _assert_g_buffer("sdf debug view", _g_buffer(backend, fp, 1), r)
        assert fp.prepass_raster_stats()[0] == r["submitted"] > 0
    finally:
        fp.destroy()


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

        good = _draws(i["path"][0])
        refused(lambda: fp.set_scene_meshes(i["meshes"], [(3, pc.IDENTITY, 0, 0)]), INVALID_ARGUMENT, "mesh index", "draw 0")
        pos, nrm, idx = i["meshes"][0]
        bad = idx.copy()
        bad[7] = pos.shape[0]
        refused(lambda: fp.set_scene_meshes([(pos, nrm, bad)], [(0, pc.IDENTITY, 0, 0)]), INVALID_ARGUMENT, "vertex index", "index 7")
        refused(lambda: fp.set_scene_meshes([(pos, nrm, idx[:-1])], [(0, pc.IDENTITY, 0, 0)]), INVALID_ARGUMENT, "triangle list")
        nan = pc.IDENTITY.copy()
        nan[9] = np.nan
        refused(lambda: fp.set_scene_meshes(i["meshes"], [good[0], (1, nan, 0, 0)]), INVALID_ARGUMENT, "non-finite", "element 9", "draw 1")
        # nothing was set by the refused calls: a frame records no prepass
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        assert fp.prepass_raster_stats() == (0, 0, 0, 0)
        fp.set_scene_meshes(i["meshes"], good)
        refused(lambda: fp.set_scene_mesh_transforms([pc.IDENTITY, pc.IDENTITY]), INVALID_ARGUMENT, "transform count", "2", "3")
        inf = pc.IDENTITY.copy()
        inf[12] = np.inf
        refused(lambda: fp.set_scene_mesh_transforms([pc.IDENTITY, pc.IDENTITY, inf]), INVALID_ARGUMENT, "non-finite", "element 12", "draw 2")
        refused(lambda: fp.set_scene_meshes(i["meshes"], [(3, pc.IDENTITY, 0, 0)]), INVALID_ARGUMENT, "mesh index")
        # the scene set before the refusals is the one the next frame draws
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        _, r = _expected(backend, fp, i["meshes"], i["mesh_of"])
        _assert_g_buffer("after refused calls", _g_buffer(backend, fp, 0), r)
        assert r["drawn"] > 100
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_meshes(i["meshes"], _draws(i["path"][0]))
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
