"""Alpha-tested cutout casters in the frame pipeline (plrf_set_shadow_caster_cutouts): 96 x 54, shadow_map_res 128, run_light_matrix = 1, the caster scene of
tests/shadow_alpha_cases.py with its large cards (box, sphere, torus, two small and five large two-sided cards; two textures - one given with its chain, one with level 0 alone so that the host builds it).

After a frame every cascade map must be bit-identical to tests/shadow_alpha_reference.py evaluated with the light matrices DOWNLOADED from sunShadowInfo, and
differ from the map without cutouts. texture_count 0 and a fresh plrf_set_shadow_casters restore the opaque maps; cutouts survive new transforms, a live
resize and a settings update; every refusal returns its code, names its cause and leaves the next frame as it was; a pipeline that never makes the call gives
the bytes of a second pipeline with the same casters - the opaque reference's.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import shadow_alpha_cases as ac
import shadow_alpha_reference as aref
import shadow_raster_cases as sc
import shadow_raster_reference as ref
from plainrenderer_amd.scene import Camera

W, H, RES = 96, 54, 128
FP_ARGS = dict(shadow_map_res=RES, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64, run_light_matrix=1)
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
NO_TEXTURE = 0xFFFFFFFF

_inputs = {}


def _scene_inputs():
    """generated once for the module; never modified"""
    if not _inputs:
        from plainrenderer_amd.frame import SyntheticInputs
        s = sc.mesh_scene()
        casters = ac.frame_scene()
        cams = [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=W / H) for i in range(3)]
        inp = SyntheticInputs(s["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45))
        patterns = [((np.arange(RES * RES, dtype=np.uint64) * (40503 + 2 * i) + 77 * i) & 0xFFFF).astype(np.uint16).reshape(RES, RES) for i in range(4)]
        moved = [(m, t.copy()) for m, t in casters["draws"]]
        for _, t in moved:
            t[12:15] += np.asarray(s["cam"].right, np.float32) * np.float32(0.75)
        (chain0, w0, h0, mips0), (chain1, w1, h1, _) = casters["textures"]
        given = [(chain0, w0, h0, mips0), (chain1[:w1 * h1], w1, h1, 0)]  # the second: level 0 alone, the host builds the chain
        _inputs.update(inp=inp, cams=cams, patterns=patterns, moved=moved, textures=given, uvs=[m[2] for m in casters["meshes"]],
                       meshes=[(m[0], m[1]) for m in casters["meshes"]], draws=casters["draws"], cutouts=casters["cutouts"])
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


def _set(fp, cutouts=True):
    i = _scene_inputs()
    fp.set_shadow_casters(i["meshes"], i["draws"])
    if cutouts:
        fp.set_shadow_caster_cutouts(i["textures"], i["uvs"], i["cutouts"])


def _maps(be, fp):
    return [be.downloadImage(fp.image("shadow%d" % i), 0, np.uint16).reshape(RES, RES).copy() for i in range(4)]


_reference_cache = {}


def _expected(be, fp, tested, draws="first"):
    """[reference result per cascade] under the light matrices the last frame fitted; tested False: the opaque reference"""
    info = be.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()
    out = []
    for c in range(3):
        key = (bytes(info[16 + 64 * c:16 + 64 * (c + 1)]), tested, draws)
        if key not in _reference_cache:
            case, tex = ac.caster_case(ref.light_matrices(info)[c], RES, draws=None if draws == "first" else _scene_inputs()["moved"], scene=ac.frame_scene())
            _reference_cache[key] = aref.rasterise(case, tex) if tested else sc.rasterise(case)
        out.append(_reference_cache[key])
    return out


def _compare(what, be, fp, want):
    i = _scene_inputs()
    maps = _maps(be, fp)
    for c in range(3):
        r = want[c]
        differing = int((maps[c] != r["map"]).sum())
        print("shadow cutout frame, %s, cascade %d: %d of %d texels differ, %d texels covered, counters %r" % (what, c, differing, RES * RES, int((r["map"] > 0).sum()), fp.shadow_raster_stats(c)))
        assert differing == 0, (what, c)
        assert fp.shadow_raster_stats(c) == (r["submitted"], r["drawn"], r["rejects"]), (what, c)
    assert np.array_equal(maps[3], i["patterns"][3]), "shadow3 lies above the cascade count and was written"
    return maps


def test_the_cutouts_of_the_frame_test_show():
    """not gpu: under the light matrices the CPU fits to the smoke camera, close to those the frame downloads, every cascade's tested map differs from its opaque
    one and tested fragments both pass and fail; the texture given with level 0 alone has the chain the reference's builder gives"""
    s, i = sc.mesh_scene(), _scene_inputs()
    for c in range(3):
        case, tex = ac.caster_case(ref.light_matrices(s["info"])[c], RES, scene=ac.frame_scene())
        a, o = aref.rasterise(case, tex), sc.rasterise(case)
        assert int((a["map"] != o["map"]).sum()) > 20 and 0 < a["passed"] < a["tested"], c
        assert (a["submitted"], a["drawn"], a["rejects"]) == (o["submitted"], o["drawn"], o["rejects"])
    assert i["textures"][1][3] == 0 and i["textures"][1][0].size == 32 * 16 and i["textures"][0][3] == 7


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_frames_with_cutouts_equal_the_reference(backend, fast):
    i = _scene_inputs()
    backend.setMathMode(fast)
    fp = plain = None
    try:
        fp = _pipeline(backend)
        _set(fp)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        general = backend.getGeneralKernelExecutions()
        tested, opaque = _expected(backend, fp, True), _expected(backend, fp, False)
        maps = _compare("cutouts %s" % ("fast" if fast else "exact"), backend, fp, tested)
        assert sum(r["drawn"] for r in tested) > 0 and all(0 < r["passed"] < r["tested"] for r in tested), "the casters lie in no cascade, or nothing is tested"
        fp.destroy()
        fp = None
        # a second pipeline that never makes the call: the opaque pass' bytes
        plain = _pipeline(backend)
        _set(plain, cutouts=False)
        plain.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        without = _compare("no cutouts %s" % ("fast" if fast else "exact"), backend, plain, _expected(backend, plain, False))
        for c in range(3):
            assert int((maps[c] != opaque[c]["map"]).sum()) > 20, "cascade %d: the cutouts do not show" % c
            assert int((maps[c] != without[c]).sum()) > 20
        if fast:
            assert general[0] == 0, "the fast-set frame ran general kernels: %r" % (general,)
    finally:
        for p in (fp, plain):
            if p is not None:
                p.destroy()
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_cutouts_removed_zeroed_dropped_and_kept(backend):
    i = _scene_inputs()
    fp = _pipeline(backend)
    try:
        _set(fp)
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        _compare("with cutouts", backend, fp, _expected(backend, fp, True))
        # texture_count 0 removes them: the opaque maps, bit for bit
        fp.set_shadow_caster_cutouts([], [], [])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 1.0 / 60.0)
        _compare("cutouts removed", backend, fp, _expected(backend, fp, False))
        # all cutoffs 0: the same
        fp.set_shadow_caster_cutouts(i["textures"], i["uvs"], [(t, 0) for t, _ in i["cutouts"]])
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5 + 2.0 / 60.0)
        _compare("all cutoffs 0", backend, fp, _expected(backend, fp, False))
        # a fresh plrf_set_shadow_casters drops them, the same casters given again included
        fp.set_shadow_caster_cutouts(i["textures"], i["uvs"], i["cutouts"])
        fp.set_shadow_casters(i["meshes"], i["draws"])
        fp.frame(i["cams"][2], 1.0 / 60.0, 0.5 + 3.0 / 60.0)
        _compare("after plrf_set_shadow_casters", backend, fp, _expected(backend, fp, False))
        # they survive a transform update, a resize and a settings update
        fp.set_shadow_caster_cutouts(i["textures"], i["uvs"], i["cutouts"])
        fp.set_shadow_caster_transforms([t for _, t in i["moved"]])
        fp.set_resolution(70, 50)
        fp.update_settings(bloom_strength=0.2)
        fp.apply_changes()
        fp.frame(Camera.look((15.06, -6.98, -5.9), (0.004, 0.16, 1.0), aspect=70 / 50), 1.0 / 60.0, 0.5 + 4.0 / 60.0)
        want, solid = _expected(backend, fp, True, draws="moved"), _expected(backend, fp, False, draws="moved")
        _compare("after a transform update, a resize to 70 x 50 and a settings update", backend, fp, want)
        assert sum(int((want[c]["map"] != solid[c]["map"]).sum()) for c in range(3)) > 50
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

        textures, uvs, cutouts = i["textures"], i["uvs"], i["cutouts"]
        refused(lambda: fp.set_shadow_caster_cutouts(textures, uvs, cutouts), INVALID_ARGUMENT, "no casters set")
        _set(fp)
        refused(lambda: fp.set_shadow_caster_cutouts(textures, uvs[:3], cutouts), INVALID_ARGUMENT, "mesh count 3", "mesh count 4")
        refused(lambda: fp.set_shadow_caster_cutouts(textures, uvs, cutouts[:4]), INVALID_ARGUMENT, "draw count 4", "draw count 10")
        level0 = textures[1][0]
        refused(lambda: fp.set_shadow_caster_cutouts([textures[0], (level0, 0, 16, 0)], uvs, cutouts), INVALID_ARGUMENT, "texture size out of range", "texture 1")
        refused(lambda: fp.set_shadow_caster_cutouts([textures[0], (level0, 16385, 1, 0)], uvs, cutouts), INVALID_ARGUMENT, "texture size out of range", "16385")
        refused(lambda: fp.set_shadow_caster_cutouts([textures[0], (level0, 32, 16, 7)], uvs, cutouts), INVALID_ARGUMENT, "too many mips", "texture 1")
        refused(lambda: fp.set_shadow_caster_cutouts([textures[0], (np.zeros(0, np.uint32), 32, 16, 0)], uvs, cutouts), INVALID_ARGUMENT, "null texels", "texture 1")
        refused(lambda: fp.set_shadow_caster_cutouts(textures, uvs, cutouts[:9] + [(2, 128)]), INVALID_ARGUMENT, "texture index out of range", "draw 9", "texture 2 of 2")
        refused(lambda: fp.set_shadow_caster_cutouts(textures, uvs, cutouts[:9] + [(1, 256)]), INVALID_ARGUMENT, "cutoff out of range", "draw 9", "256")
        # (refused before a texel is read: the full chain of 16384 x 16384 alone has more than 2^28 texels)
        from plainrenderer_amd.frame import PlrfSceneTexture, PlrfShadowCutout
        one = np.zeros(1, np.uint32)
        huge = (PlrfSceneTexture * 1)(PlrfSceneTexture(one.ctypes.data_as(C.POINTER(C.c_uint32)), 16384, 16384, 0))
        opaque = (PlrfShadowCutout * 10)(*[PlrfShadowCutout(NO_TEXTURE, 0)] * 10)
        refused(lambda: fp._check(fp.lib.plrf_set_shadow_caster_cutouts(fp.handle, huge, C.c_uint32(1), None, C.c_uint32(4), opaque, C.c_uint32(10))),
                INVALID_ARGUMENT, "too many texels")
        bad = [u.copy() for u in uvs]
        bad[2][5, 1] = np.inf
        refused(lambda: fp.set_shadow_caster_cutouts(textures, bad, cutouts), INVALID_ARGUMENT, "non-finite UV", "vertex 5 of mesh 2")
        # the cutouts set before the refusals are the ones the next frame tests with
        fp.frame(i["cams"][1], 1.0 / 60.0, 0.5)
        _compare("after refused calls", backend, fp, _expected(backend, fp, True))
    finally:
        fp.destroy()
    band = FramePipeline(backend, W, H, band_row_begin=0, band_row_end=H, **FP_ARGS)
    try:
        with pytest.raises(PlrError) as e:
            band.set_shadow_caster_cutouts(i["textures"], i["uvs"], i["cutouts"])
        assert e.value.code == UNSUPPORTED and "band" in str(e.value)
    finally:
        band.destroy()
