"""Normal maps in the frame pipeline (plrf_set_scene_normal_maps): 96 x 64, the three meshes of the texture frame test with the generators' tangents, a moving
camera and TAA jitter.

Every frame's shadingNormal must equal tests/prepass_normal_reference.py for the MainPassMatrices buffer downloaded from the pipeline and the jitters and mipBias of
the submitted global block; depth, motion, normal, albedo, specular and the counters must equal the same frames of a pipeline with textures but no normal maps.
The deferred shade reads shadingNormal and exactly it: a pipeline without a scene that gets the G-buffer uploaded with shadingNormal in the place of normal renders
the same bytes. The GI chain keeps normal. Normal maps are removed by draw_count 0, dropped by plrf_set_scene_meshes and plrf_set_scene_textures, kept across a
transform update, an alpha-cutoff call and a resize; host-derived bitangents equal the written rule; every refusal names its cause and leaves the next frame
unchanged; a band pipeline refuses.
"""
import numpy as np
import pytest

import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import prepass_texture_reference as tref
import shadow_raster_cases as sc
import test_prepass_texture_frame as ttf
from plainrenderer_amd.scene import Camera

W, H = ttf.W, ttf.H
FRAMES = 3
INVALID_ARGUMENT, UNSUPPORTED = ttf.INVALID_ARGUMENT, ttf.UNSUPPORTED
NONE = tref.NONE
OUTPUTS = ("swapchain", "post0", "post1", "color0", "color1")
GI_IMAGES = ("giFullResYSH", "giFullResCoCg", "giHistoryYSH0", "giHistoryCoCg0")

_inputs = {}


def _scene_inputs():
    """the texture frame test's inputs, and on top: the generators' tangents, bitangents by the written rule (the box, given without normals, from numpy's vertex
    normals), two steep normal textures behind the three material textures, one normal texture per draw. Generated once; never modified"""
    if not _inputs:
        from plainrenderer_amd import meshes
        i = dict(ttf._scene_inputs())
        raw = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_tangents=True), meshes.uv_sphere(1.25, segments=28, rings=14, with_tangents=True),
               meshes.torus(1.5, 0.5, segments=24, sides=12, with_tangents=True)]
        tangents = [np.asarray(m[-1], np.float32) for m in raw]
        normals = [pc.vertex_normals(m[0], m[1]) if n is None else n for m, (_, n, _) in zip(raw, i["meshes"])]
        bitangents = [nref.derive_bitangents(t, n) for t, n in zip(tangents, normals)]
        chains = list(i["chains"]) + [nc.steep(16, 16, 81), nc.steep(8, 8, 82)]
        i.update(tangents=tangents, bitangents=bitangents, chains=chains, normal_textures=[3, 4, 3])
        _inputs.update(i)
    return _inputs


def _pipeline(be, **extra):
    return ttf._pipeline(be, **extra)


def _set_scene(fp, normal_maps=True, decode=nref.DECODE_REFERENCE, derived=True):
    """scene, textures and (normal_maps) normal maps; derived: the sphere's and the torus' bitangents are left to the host"""
    i = _scene_inputs()
    fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
    fp.set_scene_textures(i["chains"], i["uvs"], i["materials"])
    if normal_maps:
        _set_normal_maps(fp, decode, derived)


def _set_normal_maps(fp, decode=nref.DECODE_REFERENCE, derived=True):
    i = _scene_inputs()
    fp.set_scene_normal_maps(i["tangents"], [i["bitangents"][0], None, None] if derived else i["bitangents"], i["normal_textures"], decode)


def _expected(be, fp, decode=nref.DECODE_REFERENCE, width=W, height=H):
    """(case, rasterise result, shadingNormal) for the frame the pipeline just rendered, from ITS matrices, jitters and mipBias"""
    i = _scene_inputs()
    n = len(i["mesh_of"])
    matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192 * n, dtype=np.float32).reshape(n, 48).copy()
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    pos, nrm, idx, draws, _ = pc.merge_meshes(i["meshes"], [(m, pc.IDENTITY) for m in i["mesh_of"]])
    case = pc.make_case(width, height, matrices, pos, idx, draws, nrm, tuple(float(v) for v in g[64:66]), tuple(float(v) for v in g[66:68]))
    r = pc.rasterise(case)
    tex = tc.textured(case, np.concatenate(i["uvs"]), i["materials"], list(i["chains"]), mip_bias=float(g[79]))[1]
    nm = dict(tangents=np.concatenate(i["tangents"]), bitangents=np.concatenate(i["bitangents"]), normal_materials=np.asarray(i["normal_textures"], np.uint32), decode=decode)
    return case, r, nref.shade(case, tex, nm, r["keys"], r["normal"])


def _g_buffer(be, fp, target, width=W, height=H, shading_normal=True):
    out = ttf._g_buffer(be, fp, target, width, height)
    if shading_normal:
        out["shadingNormal"] = be.downloadImage(fp.image("shadingNormal"), 0, np.uint32).reshape(height, width).copy()
    return out


def _outputs(be, fp, names=OUTPUTS):
    return {n: be.downloadImage(fp.image(n), 0, np.uint8).copy() for n in names}


def _assert_shading_normal(label, got, want):
    differing = int((got != want).sum())
    print("prepass normal frame %-44s: shadingNormal texels that differ %d of %d" % (label, differing, got.size))
    assert differing == 0


def _run(fp, k):
    fp.frame(_scene_inputs()["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frames_write_the_shading_normal_and_leave_the_rest_alone(backend, fast):
    from plainrenderer_amd.backend import PlrError
    backend.setMathMode(fast)
    fp = None
    try:
        fp = _pipeline(backend)
        _set_scene(fp, normal_maps=False)
        with pytest.raises(PlrError, match="shadingNormal.*does not exist yet"):
            fp.image("shadingNormal")
        plain = []
        for k in range(FRAMES):
            _run(fp, k)
            plain.append((_g_buffer(backend, fp, (k + 1) % 2, shading_normal=False), fp.prepass_raster_stats()))
        fp.destroy()
        fp = _pipeline(backend)
        _set_scene(fp)
        differing = 0
        for k in range(FRAMES):
            _run(fp, k)
            general = backend.getGeneralKernelExecutions()
            got = _g_buffer(backend, fp, (k + 1) % 2)
            case, r, sn = _expected(backend, fp)
            assert np.frombuffer(fp.submitted_globals(), np.float32)[64:68].any(), "the TAA jitter is on"
            _assert_shading_normal("%s frame %d" % ("fast" if fast else "exact", k), got["shadingNormal"], sn)
            for name in ("depth", "motion", "normal", "albedo", "specular"):
                assert np.array_equal(got[name], plain[k][0][name]), "%s of frame %d differs from the frame without normal maps" % (name, k)
            assert fp.prepass_raster_stats() == plain[k][1] == (r["submitted"], r["clipped"], r["drawn"], r["rejects"])
            differing += int((sn != r["normal"]).sum())
            if fast:
                assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
        assert differing > 500, "the normal maps show"
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_the_shade_reads_the_shading_normal_and_exactly_it(backend):
    i = _scene_inputs()
    fp = _pipeline(backend, indirect_lighting_tech=1)
    try:
        _set_scene(fp)
        recorded = []
        for k in range(FRAMES):
            _run(fp, k)
            recorded.append((_g_buffer(backend, fp, (k + 1) % 2), _outputs(backend, fp)))
        fp.destroy()
        # no scene: C's G-buffer uploaded in front of every frame, its shadingNormal as normal
        fp = _pipeline(backend, indirect_lighting_tech=1)
        for k in range(FRAMES):
            target, g = (k + 1) % 2, recorded[k][0]
            for name, image in (("depth", "depth%d" % target), ("motion", "motion%d" % target), ("shadingNormal", "normal"), ("albedo", "albedo"), ("specular", "specular")):
                backend.uploadImage(fp.image(image), g[name])
            _run(fp, k)
            got = _outputs(backend, fp)
            for n in OUTPUTS:
                assert np.array_equal(got[n], recorded[k][1][n]), "%s of frame %d differs between the two pipelines" % (n, k)
        fp.destroy()
        # and the normal maps show in the colour
        fp = _pipeline(backend, indirect_lighting_tech=1)
        _set_scene(fp, normal_maps=False)
        for k in range(FRAMES):
            _run(fp, k)
            name = "color%d" % ((k + 1) % 2)
            mine = backend.downloadImage(fp.image(name), 0, np.uint32).reshape(H, W)
            theirs = recorded[k][1][name].view(np.uint32).reshape(H, W)
            differing = int((mine != theirs).sum())
            print("prepass normal frame %d: %d colour texels differ from the frame without normal maps" % (k, differing))
            assert differing >= 100
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_the_gi_chain_does_not_read_the_shading_normal(backend):
    images = []
    for normal_maps in (False, True):
        fp = _pipeline(backend, indirect_lighting_tech=0)
        try:
            _set_scene(fp, normal_maps=normal_maps)
            _run(fp, 0)
            images.append(_outputs(backend, fp, GI_IMAGES))
        finally:
            fp.destroy()
    assert any(images[0][n].any() for n in GI_IMAGES), "the GI chain ran"
    for n in GI_IMAGES:
        assert np.array_equal(images[0][n], images[1][n]), "%s depends on normal maps" % n


@pytest.mark.gpu
def test_gpu_normal_maps_removed_dropped_kept_and_derived(backend):
    i = _scene_inputs()
    fp = None
    never = _pipeline(backend, indirect_lighting_tech=1)  # (one pipeline at a time: they share the backend's swapchain)
    try:
        # removed by draw_count 0, dropped by plrf_set_scene_textures, dropped by plrf_set_scene_meshes - each in front of a frame that `never`, a pipeline
        # that never called, renders too (the same other calls on both): as long as no frame ran with normal maps the two hold the same history, so every
        # output must be equal byte for byte. shadingNormal exists from the first call on and is not written by those frames
        steps = (("draw_count 0", lambda p, mine: p.set_scene_normal_maps(None, None, []) if mine else None),
                 ("plrf_set_scene_textures", lambda p, mine: p.set_scene_textures(i["chains"], i["uvs"], i["materials"])),
                 ("plrf_set_scene_meshes", lambda p, mine: _set_scene(p, normal_maps=False)))
        _set_scene(never, normal_maps=False)
        theirs = []
        for k, (label, step) in enumerate(steps):
            step(never, False)
            _run(never, k)
            theirs.append(_outputs(backend, never))
        never.destroy()
        never = None
        fp = _pipeline(backend, indirect_lighting_tech=1)
        _set_scene(fp)
        for k, (label, step) in enumerate(steps):
            if k:
                _set_normal_maps(fp)
            step(fp, True)
            _run(fp, k)
            mine = _outputs(backend, fp)
            for n in OUTPUTS:
                assert np.array_equal(mine[n], theirs[k][n]), "%s after %s differs from a pipeline that never called" % (n, label)
            assert not backend.downloadImage(fp.image("shadingNormal"), 0, np.uint32).any(), "%s: shadingNormal was written" % label
        assert mine["swapchain"].any()
        # set again behind the drops, and kept across a transform update, an alpha-cutoff call and a resize
        _set_normal_maps(fp)
        models = [m.copy() for m in i["models"]]
        models[1][12:15] += np.asarray(sc.mesh_scene()["cam"].right, np.float32) * np.float32(0.4)
        fp.set_scene_mesh_transforms(models)
        fp.set_scene_alpha_cutoffs([0, 0, 0])
        fp.set_resolution(70, 50)
        fp.apply_changes()
        fp.frame(Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50), 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        case, r, sn = _expected(backend, fp, width=70, height=50)
        _assert_shading_normal("after a transform update, a cutoff call and a resize", _g_buffer(backend, fp, 0, 70, 50)["shadingNormal"], sn)  # (the pipeline's fourth frame)
        assert (sn != r["normal"]).sum() > 100
    finally:
        for p in (fp, never):
            if p is not None:
                p.destroy()


@pytest.mark.gpu
def test_gpu_host_derived_bitangents_equal_the_written_rule(backend):
    """host-derived bitangents against the same bitangents computed in numpy by the written rule and passed in: two pipelines, one frame each, unit decode"""
    first = []
    for derived in (True, False):
        p = _pipeline(backend)
        try:
            _set_scene(p, decode=nref.DECODE_UNIT, derived=derived)
            _run(p, 0)
            first.append(_g_buffer(backend, p, 1)["shadingNormal"])
            if derived:
                case, r, sn = _expected(backend, p, nref.DECODE_UNIT)
                _assert_shading_normal("unit decode, host-derived bitangents", first[0], sn)
        finally:
            p.destroy()
    assert np.array_equal(first[0], first[1]), "derived and passed-in bitangents give different images"


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

        t, b, n = i["tangents"], i["bitangents"], i["normal_textures"]
        refused(lambda: fp.set_scene_normal_maps(t, b, n), INVALID_ARGUMENT, "no scene set")
        fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
        refused(lambda: fp.set_scene_normal_maps(t, b, n), INVALID_ARGUMENT, "no textures set")
        fp.set_scene_textures(i["chains"], i["uvs"], i["materials"])
        _set_normal_maps(fp)
        _run(fp, 0)
        before = _g_buffer(backend, fp, 1)
        refused(lambda: fp.set_scene_normal_maps(t[:2], b[:2], n), INVALID_ARGUMENT, "mesh count 2", "mesh count 3")
        refused(lambda: fp.set_scene_normal_maps(t, b, n + [0]), INVALID_ARGUMENT, "draw count 4", "draw count 3")
        refused(lambda: fp.set_scene_normal_maps(t, b, [3, 5, NONE]), INVALID_ARGUMENT, "normal texture index", "draw 1", "texture 5 of 5")
        bad = [a.copy() for a in t]
        bad[2][7, 1] = np.nan
        refused(lambda: fp.set_scene_normal_maps(bad, b, n), INVALID_ARGUMENT, "non-finite tangent", "vertex 7 of mesh 2")
        bad = [a.copy() for a in b]
        bad[1][3, 0] = np.inf
        refused(lambda: fp.set_scene_normal_maps(t, bad, n), INVALID_ARGUMENT, "non-finite bitangent", "vertex 3 of mesh 1")
        refused(lambda: fp.set_scene_normal_maps(t, b, n, 3), INVALID_ARGUMENT, "decode is 3")
        refused(lambda: fp.set_scene_normal_maps(t, b, n, 0), INVALID_ARGUMENT, "decode is 0")
        refused(lambda: fp.set_scene_normal_maps(t, None, n), INVALID_ARGUMENT, "mesh 0 was given without normals")

        def null_textures():  # at the C boundary: NULL normal_textures with a non-zero count
            import ctypes as C
            fp._check(fp.lib.plrf_set_scene_normal_maps(fp.handle, None, None, C.c_uint32(3), None, C.c_uint32(3), C.c_uint32(1)))
        refused(null_textures, INVALID_ARGUMENT, "normal_textures are null")
        # the normal maps set before the refusals are the ones the next frame uses, and that frame is the one a pipeline renders that made no refused call
        _run(fp, 1)
        case, r, sn = _expected(backend, fp)
        after = _g_buffer(backend, fp, 0)
        _assert_shading_normal("after refused calls", after["shadingNormal"], sn)
        mine = _outputs(backend, fp)
        fp.destroy()
        fp = None  # (one pipeline at a time: they share the backend's swapchain)
        twin = _pipeline(backend)
        try:
            _set_scene(twin)
            _run(twin, 0)
            first = _g_buffer(backend, twin, 1)
            _run(twin, 1)
            second, outputs = _g_buffer(backend, twin, 0), _outputs(backend, twin)
        finally:
            twin.destroy()
        for name in before:
            assert np.array_equal(before[name], first[name]) and np.array_equal(after[name], second[name]), name
        for n in OUTPUTS:
            assert np.array_equal(mine[n], outputs[n]), "%s differs from the frame of a pipeline without refused calls" % n
    finally:
        if fp is not None:
            fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **ttf.FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_normal_maps(i["tangents"], i["bitangents"], i["normal_textures"])
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
