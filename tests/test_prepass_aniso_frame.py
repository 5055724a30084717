"""Anisotropic filtering in the frame pipeline (plrf_set_scene_anisotropy): 96 x 64, the synthetic inputs of the texture frame test, and as the scene one large
ground quad below its moving camera with a 64 x 64 striped albedo and a 32 x 32 random-texel normal map, TAA jitter on.

Over three frames with set_scene_anisotropy(8) the six prepass images must be bit-identical to tests/prepass_aniso_reference.py run on the pipeline's own
matrices, jitters and mipBias, and the final colour must differ from the isotropic pipeline's on the floor. 0, 1 and never-called are byte-identical, final
colour included. The setting survives a resize, a set_scene_textures_formatted and a set_scene_meshes followed by new textures; a value set before any scene exists
takes effect once textures arrive; 17 is refused by name and changes nothing; a band pipeline refuses.
"""
import numpy as np
import pytest

import prepass_aniso_cases as an
import prepass_aniso_reference as aniso
import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import prepass_texture_cases as tc
import test_prepass_normal_frame as tnf
import test_prepass_raster as tpr
import test_prepass_texture_frame as ttf
from plainrenderer_amd.scene import Camera

W, H, FRAMES = ttf.W, ttf.H, 3
NONE = ttf.NONE
FLOOR_Y = -5.5  # the camera flies at y = -7 and looks 9 degrees towards +y
POSITIONS = np.array([[-25.0, FLOOR_Y, -11.0], [55.0, FLOOR_Y, -11.0], [55.0, FLOOR_Y, 194.0], [-25.0, FLOOR_Y, 194.0]], np.float32)
NORMALS = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (4, 1))  # towards the sun of the synthetic inputs (direction (0.35, -0.8, 0.45)): the floor is lit
INDICES = np.array([0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3], np.uint32)  # both windings: one faces the camera
UVS = (POSITIONS[:, [0, 2]] / np.float32(1.5)).astype(np.float32)
TANGENTS = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (4, 1))
BITANGENTS = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (4, 1))



def _stripes():
    """64 x 64, stripes four texels wide across u and constant along v, with the full chain: the floor's footprint is long along v and short along u, so the
    isotropic level (the long axis') blurs the stripes to their mean where the anisotropic level (the short axis') still resolves them - a difference the final
    colour shows, which filtered random texels (grey either way) do not"""
    x = np.arange(64, dtype=np.uint32)[None, :].repeat(64, axis=0)
    level0 = np.where((x >> np.uint32(2)) & np.uint32(1), np.uint32(0xFF10E0F0), np.uint32(0xFFF02010)).reshape(-1)
    return tc.chain(level0, 64, 64), 64, 64, 7


TEXTURES = [_stripes(), an.random_chain(32, 42)]
MATERIALS = [(0, NONE)]
NORMAL_TEXTURES = [1]
G_BUFFER = ("depth", "motion", "normal", "albedo", "specular", "shadingNormal")


def _set_scene(fp, textures=True, normal_maps=True):
    fp.set_scene_meshes([(POSITIONS, NORMALS, INDICES)], [(0, pc.IDENTITY, *pc.material(0))])
    if textures:
        fp.set_scene_textures(TEXTURES, [UVS], MATERIALS)
        if normal_maps:
            fp.set_scene_normal_maps([TANGENTS], [BITANGENTS], NORMAL_TEXTURES, nref.DECODE_UNIT)


def _expected(be, fp, A, width=W, height=H, normal_maps=True):
    """the six images of the frame the pipeline just rendered, as words, from ITS matrices, jitters and mipBias"""
    matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192, dtype=np.float32).reshape(1, 48).copy()
    g = np.frombuffer(fp.submitted_globals(), np.float32)
    case = pc.make_case(width, height, matrices, POSITIONS, INDICES, [[0, 12, 0, 0, *pc.material(0)]], NORMALS, tuple(float(v) for v in g[64:66]), tuple(float(v) for v in g[66:68]))
    tex = tc.textured(case, UVS, MATERIALS, TEXTURES, mip_bias=float(g[79]))[1]
    if A >= 2:
        base = aniso.base_images(case, tex, None, A, diagnostics=True)
    else:
        base = nc.base_images(case, tex, None)
    want = dict(tpr.reference_words(base))
    if normal_maps:
        nm = nc.normal_inputs(case, TANGENTS, BITANGENTS, NORMAL_TEXTURES, nref.DECODE_UNIT)
        want["shadingNormal"] = aniso.shade(case, tex, nm, base["keys"], base["normal"], A) if A >= 2 else nref.shade(case, tex, nm, base["keys"], base["normal"])
    return want, base


def _assert_g_buffer(label, got, want):
    differing = {name: int((got[name] != want[name]).sum()) for name in want}
    print("prepass aniso frame %-44s: texels that differ %r of %d" % (label, differing, got["depth"].size))
    assert not any(differing.values()), differing


def _frames(be, fp, count=FRAMES):
    i = ttf._scene_inputs()
    out = []
    for k in range(count):
        fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
        out.append((tnf._g_buffer(be, fp, (k + 1) % 2), tnf._outputs(be, fp)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_anisotropic_frames_are_the_references_and_show_in_the_final_colour(backend, fast):
    backend.setMathMode(fast)
    fp = None
    try:
        i = ttf._scene_inputs()
        fp = ttf._pipeline(backend)
        _set_scene(fp)
        fp.set_scene_anisotropy(8)
        anisotropic = []
        for k in range(FRAMES):
            fp.frame(i["cams"][k + 1], 1.0 / 60.0, 0.5 + k / 60.0)
            general = backend.getGeneralKernelExecutions()
            got = tnf._g_buffer(backend, fp, (k + 1) % 2)
            if fast:
                assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
            assert np.frombuffer(fp.submitted_globals(), np.float32)[64:68].any(), "the TAA jitter is on"
            want, base = _expected(backend, fp, 8)
            _assert_g_buffer("%s frame %d" % ("fast" if fast else "exact", k), got, want)
            N = base["diagnostics"]["albedo"]["N"]
            assert (base["keys"] != 0).sum() > W * H // 3 and np.unique(N[N > 0]).size >= 5, "the floor fills the lower frame with many probe counts"
            anisotropic.append((got, tnf._outputs(backend, fp), base["keys"] != 0))
        fp.destroy()
        fp = ttf._pipeline(backend)
        _set_scene(fp)
        for k, (got, outputs) in enumerate(_frames(backend, fp)):
            floor = anisotropic[k][2]
            assert np.array_equal(got["depth"], anisotropic[k][0]["depth"]) and (got["albedo"] != anisotropic[k][0]["albedo"])[floor].sum() > floor.sum() // 2
            print("prepass aniso frame %d: bytes of the outputs that differ from the isotropic pipeline's %r" % (k, {n: int((outputs[n] != anisotropic[k][1][n]).sum()) for n in outputs}))
            # the final colour: the frame's lit colour target and the post-process target behind it, per pixel of the floor; the 8-bit swapchain behind the
            # tonemapper moves in a few dozen bytes only under the synthetic inputs' exposure (printed above), so it is only asked to move at all
            target = (k + 1) % 2
            on_floor = lambda name: int((outputs[name] != anisotropic[k][1][name]).reshape(H, W, -1).any(axis=2)[floor].sum())
            for name, pixels in (("color%d" % target, on_floor("color%d" % target)), ("post0 | post1", max(on_floor("post0"), on_floor("post1")))):
                assert pixels > floor.sum() // 10, "%s differs from the isotropic pipeline's on %d of the floor's %d pixels" % (name, pixels, floor.sum())
            assert (outputs["swapchain"] != anisotropic[k][1]["swapchain"]).any()
    finally:
        if fp is not None:
            fp.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_off_values_are_byte_identical_to_a_pipeline_never_told(backend):
    recorded = []
    for value in (None, 0, 1):
        fp = ttf._pipeline(backend)
        try:
            _set_scene(fp)
            if value is not None:
                fp.set_scene_anisotropy(value)
            recorded.append(_frames(backend, fp))
        finally:
            fp.destroy()
    for other in recorded[1:]:
        for (g0, o0), (g1, o1) in zip(recorded[0], other):
            for name in g0:
                assert g0[name].tobytes() == g1[name].tobytes(), name
            for name in o0:
                assert o0[name].tobytes() == o1[name].tobytes(), name


@pytest.mark.gpu
def test_gpu_the_setting_survives_and_waits_for_textures(backend):
    i = ttf._scene_inputs()
    fp = ttf._pipeline(backend)
    try:
        # set before any scene exists: nothing to sample yet, the frame is the untextured one
        fp.set_scene_anisotropy(8)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        _set_scene(fp, textures=False)
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        assert np.unique(ttf._g_buffer(backend, fp, 0)["albedo"]).size <= 2, "no textures: the draw's constant word, or sky"
        # textures arrive: it takes effect
        _set_scene(fp)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        want, base = _expected(backend, fp, 8)
        _assert_g_buffer("set before the scene", tnf._g_buffer(backend, fp, 1), want)
        isotropic, _ = _expected(backend, fp, 0)
        assert (want["albedo"] != isotropic["albedo"]).sum() > 500
        # a formatted store of RGBA8 entries (code 2) replaces the store and drops the normal maps; the setting stays
        fp.set_scene_textures_formatted([(*t, 2) for t in TEXTURES], [UVS], MATERIALS)
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        want, _ = _expected(backend, fp, 8, normal_maps=False)
        _assert_g_buffer("after set_scene_textures_formatted", ttf._g_buffer(backend, fp, 0), want)
        # set_scene_meshes drops the textures; new ones are sampled anisotropically again
        _set_scene(fp, textures=False)
        fp.set_scene_textures(TEXTURES, [UVS], MATERIALS)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        want, _ = _expected(backend, fp, 8, normal_maps=False)
        _assert_g_buffer("after set_scene_meshes and new textures", ttf._g_buffer(backend, fp, 1), want)
        # a resize
        fp.set_resolution(70, 50)
        fp.apply_changes()
        cam = Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50)
        fp.frame(cam, 1.0 / 60.0, 0.5 + 5.0 / 60.0)
        want, _ = _expected(backend, fp, 8, 70, 50, normal_maps=False)
        _assert_g_buffer("after a resize to 70 x 50", ttf._g_buffer(backend, fp, 1, 70, 50), {name: want[name] for name in ("normal", "albedo", "specular")})  # (the resize restarts the depth and motion targets' turn)
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_refusals_name_their_cause_and_change_nothing(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    i = ttf._scene_inputs()
    fp = ttf._pipeline(backend)
    try:
        _set_scene(fp)
        fp.set_scene_anisotropy(4)
        with pytest.raises(PlrError) as e:
            fp.set_scene_anisotropy(17)
        assert e.value.code == ttf.INVALID_ARGUMENT and "17" in str(e.value) and "16" in str(e.value), e.value
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        want, _ = _expected(backend, fp, 4)
        _assert_g_buffer("after a refused call: still 4", tnf._g_buffer(backend, fp, 1), want)
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **ttf.FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_scene_anisotropy(8)
        assert e.value.code == ttf.UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
