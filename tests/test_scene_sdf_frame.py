"""SDF instances from the scene in the frame pipeline (plrf_set_scene_sdf), at 256 x 128 and 320 x 192: a floor (no SDF) and two boxes of 2 x 2 x 2 m and
9 x 1 x 3 m whose meshes are baked by the call (volumes of 16^3 and 64 x 16 x 16), the cube with a textured albedo, run_gi on, six frames, the exact kernel set
(one test repeats the comparison in the fast set).

A and B: pipeline A uses plrf_set_scene_sdf; pipeline B gets the same volumes from the host bake through plrf_add_sdf_volume_dds and, in front of every frame, an
instance buffer packed by tests/scene_sdf_reference.py and uploaded with plrf_set_sdf_scene. The GI images, the colour buffer, the resolved colour and the tonemapped
output must be equal byte for byte on every frame (the texture indices in the instance buffers may differ). From frame 3 on the cube moves
(plrf_set_scene_mesh_transforms): A still equals B, sdfInstances read back after frame 3 holds the reference's record for the new matrix, and A's traced GI of
frame 4 differs from the same run without the move - the guard against comparing two empty traces.
Further: the stats do not grow under repeated calls, removal leaves no instance, plrf_set_scene_meshes removes the scene SDF, plrf_set_sdf_scene is refused while it
is set and accepted afterwards, every refusal names its cause and changes nothing; the SDF debug view shows the scene's instances; a pipeline that never calls
the new entry points records the passes it recorded before; a 2-band partition with band_raster = 1 and whole-image halos equals the unpartitioned frame.
"""
import copy
import struct

import numpy as np
import pytest

import prepass_raster_cases as pc
import prepass_texture_cases as tc
import scene_sdf_reference as ref

SIZES = [(256, 128), (320, 192)]
FP_ARGS = dict(shadow_map_res=128, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64)
FRAMES, MOVE_AT = 6, 3
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
NONE = ref.NONE
F32 = np.float32
GI_IMAGES = ("giYSH0", "giCoCg0", "giHistoryYSH0", "giHistoryCoCg0", "giFullResYSH", "giFullResCoCg")

_cache = {}


def _translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return pc.glm(m)


def _scene():
    """generated once for the module; never modified. y points down: the floor's top is at y = -4, three metres below the camera, the boxes stand on it"""
    if "scene" not in _cache:
        from plainrenderer_amd import meshes
        raw = [meshes.box((14.0, 0.25, 14.0), subdiv=2), meshes.box((1.0, 1.0, 1.0), subdiv=2, with_uvs=True), meshes.box((4.5, 0.5, 1.5), subdiv=2)]
        ms = [pc.mesh_arrays(m, False) for m in raw]
        models = [_translation(15.0, -3.75, 8.0), _translation(12.5, -5.0, 6.0), _translation(18.0, -4.5, 12.0)]
        moved = [m.copy() for m in models]
        moved[1] = _translation(14.0, -5.0, 7.5)
        boxes = [None] + [(m[0].min(axis=0).astype(F32), m[0].max(axis=0).astype(F32)) for m in ms[1:]]
        texture = (tc.chain(tc.pattern(16, 16, 31), 16, 16), 16, 16, 5)
        materials = [(NONE, NONE), (0, NONE), (NONE, NONE)]
        words = [pc.material(d)[0] for d in range(3)]
        albedos = [ref.mean_albedo([words[0]])[:3], ref.mean_albedo(texture[0][:256])[:3], ref.mean_albedo([words[2]])[:3]]
        _cache["scene"] = dict(meshes=ms, models=models, moved=moved, boxes=boxes, texture=texture, uvs=[None, np.asarray(raw[1][2], F32), None], materials=materials,
                               albedos=albedos)
    return _cache["scene"]


def _cams(w, h, n=FRAMES):
    from plainrenderer_amd.scene import Camera
    return [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=w / h) for i in range(n + 1)]


def _inputs(w, h):
    if (w, h) not in _cache:
        from plainrenderer_amd import synth
        from plainrenderer_amd.frame import SyntheticInputs
        cams = _cams(w, h)
        _cache[(w, h)] = SyntheticInputs(synth.SynthScene(grid=4, cell=8.0, seed_id=600), cams[1], cams[0], w, h, sdf_res=16, shadow_res=128, froxel_depth=8,
                                         sun_direction=(0.35, -0.8, 0.45))
    return _cache[(w, h)]


def _draws(models):
    return [(d, m, *pc.material(d)) for d, m in enumerate(models)]


def _pipeline(be, w, h, scene=True, **extra):
    from plainrenderer_amd.frame import FramePipeline
    fp = FramePipeline(be, w, h, **dict(FP_ARGS, **extra))
    copy.copy(_inputs(w, h)).upload(fp)
    if scene:
        _set_scene(fp)
    return fp


def _set_scene(fp):
    s = _scene()
    fp.set_scene_meshes(s["meshes"], _draws(s["models"]))
    fp.set_scene_textures([s["texture"]], s["uvs"], s["materials"])


def _baked_volumes():
    """the host bake of the two boxes, as the asset pipeline runs it: [(width, height, depth), uint16 voxels]"""
    if "volumes" not in _cache:
        from plainrenderer_amd import sdf_bake
        s = _scene()
        out = []
        for (pos, _, idx), (mn, mx) in zip(s["meshes"][1:], s["boxes"][1:]):
            res = sdf_bake.sdf_texture_description(mn, mx)
            out.append((res, sdf_bake.compute_sdf(pos, idx, mn, mx, res)))
        assert [r for r, _ in out] == [(16, 16, 16), (64, 16, 16)]
        _cache["volumes"] = out
    return _cache["volumes"]


def _add_volumes_from_dds(fp, tmp_path):
    from plainrenderer_amd import image_io
    from plainrenderer_amd.backend import ImageDescription, ImageFormat, ImageType, ImageUsageFlags, MipCount
    indices = []
    for k, (res, voxels) in enumerate(_baked_volumes()):
        path = tmp_path / ("volume%d.dds" % k)
        image_io.write_dds_file(path, ImageDescription(width=res[0], height=res[1], depth=res[2], type=ImageType.Type3D, format=ImageFormat.R16_sFloat,
                                                       usageFlags=int(ImageUsageFlags.Sampled), mipCount=MipCount.One, manualMipCount=1), voxels)
        index, size = fp.add_sdf_volume_dds(path)
        assert size == res
        indices.append(index)
    return indices


def _packed(models, texture_indices):
    s = _scene()
    return ref.pack_scene(np.stack(models), [0, 1, 2], s["boxes"], [NONE] + list(texture_indices), s["albedos"])


def _download(be, fp, frame, w, h, names=GI_IMAGES):
    cur = (frame + 1) % 2
    out = {n: be.downloadImage(fp.image(n), 0, np.uint8).copy() for n in names}
    out["color"] = be.downloadImage(fp.image("color%d" % cur), 0, np.uint8).copy()
    out["post"] = be.downloadImage(fp.image("post1"), 0, np.uint8).copy()
    out["swapchain"] = be.downloadImage(fp.image("swapchain"), 0, np.uint8).copy()
    return out


def _run(be, w, h, how, tmp_path=None, move=True, frames=FRAMES, names=GI_IMAGES):
    """how: 'scene' (plrf_set_scene_sdf) or 'upload' (volumes from DDS files, instances packed by the reference in front of every frame)"""
    from plainrenderer_amd.frame import SDF_BAKE, NO_TEXTURE
    s = _scene()
    cams = _cams(w, h)
    fp = _pipeline(be, w, h)
    try:
        if how == "scene":
            fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
        else:
            indices = _add_volumes_from_dds(fp, tmp_path)
        out, models = [], s["models"]
        for f in range(frames):
            if move and f == MOVE_AT:
                models = s["moved"]
                fp.set_scene_mesh_transforms(models)
            if how == "upload":
                fp.set_sdf_scene(*_packed(models, indices))
            fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
            images = _download(be, fp, f, w, h, names)
            images["instances"] = be.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes()
            images["bbs"] = be.downloadStorageBuffer(fp.storage_buffer("sdfWorldBBs"), 32 * 2).tobytes()
            out.append(images)
        return out
    finally:
        fp.destroy()


def _without_texture_indices(instances):
    b = bytearray(instances)
    for i in range(2):
        b[16 + 96 * i + 12:16 + 96 * i + 16] = bytes(4)
    return bytes(b)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=["256x128", "320x192"])
def test_gpu_scene_sdf_frames_equal_frames_of_uploaded_instances(backend, tmp_path, w, h):
    backend.setMathMode(False)
    a = _run(backend, w, h, "scene")
    b = _run(backend, w, h, "upload", tmp_path)
    for f in range(FRAMES):
        differing = [n for n in a[f] if n not in ("instances", "bbs") and not np.array_equal(a[f][n], b[f][n])]
        print("scene sdf frame %dx%d frame %d: outputs that differ between the scene SDF and the uploaded instances: %r" % (w, h, f, differing))
        assert not differing
        assert a[f]["bbs"] == b[f]["bbs"] and _without_texture_indices(a[f]["instances"]) == _without_texture_indices(b[f]["instances"])
    # the instance buffer after the move holds the new inverse: the reference's record for the moved matrix, and another one than before
    s = _scene()
    indices = [struct.unpack_from("<I", a[MOVE_AT]["instances"], 16 + 96 * i + 12)[0] for i in range(2)]
    assert a[MOVE_AT]["instances"] == _packed(s["moved"], indices)[0] and a[MOVE_AT - 1]["instances"] == _packed(s["models"], indices)[0]
    assert a[MOVE_AT]["instances"][16 + 32:16 + 96] != a[MOVE_AT - 1]["instances"][16 + 32:16 + 96], "the cube's worldToLocal changed"
    assert a[MOVE_AT]["instances"][16 + 96:] == a[MOVE_AT - 1]["instances"][16 + 96:], "the slab did not move"
    # the guard: the trace sees the instances - the same run without the move gives another traced GI on frame 4
    still = _run(backend, w, h, "scene", move=False, frames=MOVE_AT + 2, names=("giYSH0", "giCoCg0"))
    assert np.array_equal(still[MOVE_AT - 1]["giYSH0"], a[MOVE_AT - 1]["giYSH0"]), "up to the move the two runs are one"
    changed = int((still[MOVE_AT + 1]["giYSH0"].view(np.uint64) != a[MOVE_AT + 1]["giYSH0"].view(np.uint64)).sum())
    print("scene sdf frame %dx%d: traced GI texels of frame %d that the move changed: %d" % (w, h, MOVE_AT + 1, changed))
    assert changed > 50


@pytest.mark.gpu
def test_gpu_the_fast_kernel_set_agrees_too(backend, tmp_path):
    w, h = SIZES[0]
    backend.setMathMode(True)
    try:
        names = ("giHistoryYSH0", "giHistoryCoCg0")
        a = _run(backend, w, h, "scene", names=names)
        b = _run(backend, w, h, "upload", tmp_path, names=names)
    finally:
        backend.setMathMode(False)
    for f in range(FRAMES):
        differing = [n for n in a[f] if n not in ("instances", "bbs") and not np.array_equal(a[f][n], b[f][n])]
        assert not differing, (f, differing)
        assert a[f]["bbs"] == b[f]["bbs"] and _without_texture_indices(a[f]["instances"]) == _without_texture_indices(b[f]["instances"])


@pytest.mark.gpu
def test_gpu_stats_removal_and_refusals(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import NO_TEXTURE, SDF_BAKE, FramePipeline
    w, h = SIZES[0]
    s, cams = _scene(), _cams(w, h)
    backend.setMathMode(False)

    def refused(call, code, *words):
        with pytest.raises(PlrError) as e:
            call()
        assert e.value.code == code, e.value
        assert all(word in str(e.value) for word in words), e.value

    fp = _pipeline(backend, w, h, scene=False)
    try:
        assert fp.scene_sdf_stats() == (0, 0, 0)
        refused(lambda: fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE]), INVALID_ARGUMENT, "no scene set")
        nothing = (bytes(16), bytes(32))  # an upload of no instance
        _set_scene(fp)
        refused(lambda: fp.set_scene_sdf([SDF_BAKE, SDF_BAKE]), INVALID_ARGUMENT, "mesh count 2", "mesh count 3")
        singular = [m.copy() for m in s["models"]]
        singular[2][5] = 0.0
        fp.set_scene_mesh_transforms(singular)  # no scene SDF yet: the prepass takes a flat slab
        refused(lambda: fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE]), INVALID_ARGUMENT, "singular model matrix", "draw 2")
        assert fp.scene_sdf_stats() == (0, 0, 0)
        fp.set_scene_mesh_transforms(s["models"])
        fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
        first = fp.scene_sdf_stats()
        assert first == (2, 2, 2 * (16 * 16 * 16 + 64 * 16 * 16))
        for _ in range(3):
            fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
            assert fp.scene_sdf_stats() == first, "repeated calls re-use the images of the volumes they replace"
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        instances = backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes()
        # refusals while the scene SDF is set: each names its cause, none changes anything
        refused(lambda: fp.set_sdf_scene(*nothing), UNSUPPORTED, "scene SDF")
        refused(lambda: fp.set_scene_mesh_transforms(singular), INVALID_ARGUMENT, "singular model matrix", "draw 2", "zero")
        refused(lambda: fp.set_scene_sdf_mean_albedo(np.zeros((2, 3), F32)), INVALID_ARGUMENT, "draw count 2", "draw count 3")
        refused(lambda: fp.set_scene_sdf_mean_albedo([[0.5, np.inf, 0.5]] * 3), INVALID_ARGUMENT, "non-finite mean albedo", "draw 0")
        assert fp.scene_sdf_stats() == first
        # a frame with the same camera and time on a pipeline in the same state gives the same instances: nothing was changed by the refused calls
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        assert backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes() == instances
        # an override replaces the derived mean albedo of its draw alone
        fp.set_scene_sdf_mean_albedo([[np.nan, 0, 0], [0.25, 0.5, 0.75], [np.nan, 1, 1]])
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        overridden = backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes()
        assert overridden[16 + 16:16 + 28] == np.array([0.25, 0.5, 0.75], F32).tobytes() and overridden[16 + 96:] == instances[16 + 96:] and overridden[16 + 32:16 + 96] == instances[16 + 32:16 + 96]
        fp.set_scene_sdf_mean_albedo(None)
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        assert backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes() == instances
        # removal: no instance, no volume; the upload is accepted again
        fp.set_scene_sdf(None)
        assert fp.scene_sdf_stats() == (0, 0, 0)
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        assert backend.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16)[:4].tobytes() == bytes(4), "the instance count is 0 until the caller uploads again"
        fp.set_sdf_scene(*nothing)
        # set again (the released images are re-used), then plrf_set_scene_meshes removes it
        fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
        assert fp.scene_sdf_stats() == first
        fp.set_scene_meshes(s["meshes"], _draws(s["models"]))
        assert fp.scene_sdf_stats() == (0, 0, 0)
        fp.set_sdf_scene(*nothing)
        fp.frame(cams[2], 1.0 / 60.0, 0.5)
    finally:
        fp.destroy()
    few = FramePipeline(backend, w, h, **dict(FP_ARGS, max_sdf_instances=1))  # (no frame is rendered: nothing is uploaded)
    try:
        _set_scene(few)
        refused(lambda: few.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE]), INVALID_ARGUMENT, "too many SDF instances", "2 draws", "is 1")
        few.set_scene_sdf([NO_TEXTURE, NO_TEXTURE, SDF_BAKE])
        assert few.scene_sdf_stats() == (1, 1, 2 * 64 * 16 * 16)
    finally:
        few.destroy()
    band = FramePipeline(backend, w, h, band_row_begin=0, band_row_end=h, **FP_ARGS)
    try:
        refused(lambda: band.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE]), UNSUPPORTED, "band")
        refused(lambda: band.set_scene_sdf(None), UNSUPPORTED, "band")
    finally:
        band.destroy()


def _pass_names(be, fp, cam, time):
    be.setPassTiming(True)
    try:
        fp.frame(cam, 1.0 / 60.0, time)
        be.waitForGPUIdle()
        return [name for name, _ in be.getRenderpassTimings()]
    finally:
        be.setPassTiming(False)


@pytest.mark.gpu
def test_gpu_the_pass_list_changes_only_with_the_call(backend):
    from plainrenderer_amd.frame import NO_TEXTURE, SDF_BAKE
    w, h = SIZES[0]
    cams = _cams(w, h)
    backend.setMathMode(False)
    new = ("SDF instance update", "Scene mean albedo")
    fp = _pipeline(backend, w, h)
    try:
        plain = [_pass_names(backend, fp, cams[1 + k], 0.5 + k / 60.0) for k in range(2)]
        assert plain[0] and not any(n.startswith(new) for names in plain for n in names), "a pipeline that never calls the new entry points records neither pass"
        fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
        first, second = (_pass_names(backend, fp, cams[1 + k], 0.5 + k / 60.0) for k in range(2))
        without = lambda names: [n for n in names if not n.startswith(new)]
        assert without(first) == plain[1] and without(second) == plain[1], "every other pass is recorded as before, in the same order"
        assert [n for n in first if n.startswith(new)] == ["Scene mean albedo (mark)", "Scene mean albedo", "SDF instance update"] or \
            [n for n in first if n.startswith(new)] == ["Scene mean albedo", "Scene mean albedo (mark)", "SDF instance update"], first
        assert [n for n in second if n.startswith(new)] == ["SDF instance update"], "the mean albedos are reduced once, not per frame"
        at = first.index("SDF instance update")
        assert first[at + 1] == "SDF camera frustum culling", first
        fp.set_scene_textures([_scene()["texture"]], _scene()["uvs"], _scene()["materials"])
        third = _pass_names(backend, fp, cams[3], 0.5 + 2 / 60.0)
        assert any(n == "Scene mean albedo" for n in third), "a new texture store is reduced again"
        fp.set_scene_sdf(None)
        assert _pass_names(backend, fp, cams[4], 0.5 + 3 / 60.0) == plain[1]
    finally:
        fp.destroy()


@pytest.mark.gpu
def test_gpu_the_debug_view_shows_the_scene_s_instances(backend, tmp_path):
    from plainrenderer_amd.frame import NO_TEXTURE, SDF_BAKE
    w, h = SIZES[0]
    cams = _cams(w, h)
    backend.setMathMode(False)
    views = {}
    for how in ("scene", "upload", "none"):
        fp = _pipeline(backend, w, h, sdf_debug_mode=1)
        try:
            if how == "scene":
                fp.set_scene_sdf([NO_TEXTURE, SDF_BAKE, SDF_BAKE])
            elif how == "upload":
                fp.set_sdf_scene(*_packed(_scene()["models"], _add_volumes_from_dds(fp, tmp_path)))
            else:
                fp.set_sdf_scene(bytes(16), bytes(32))
            for f in range(2):
                fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
            views[how] = backend.downloadImage(fp.image("swapchain"), 0, np.uint32).copy()
        finally:
            fp.destroy()
    assert np.array_equal(views["scene"], views["upload"])
    shown = int((views["scene"] != views["none"]).sum())
    print("scene sdf debug view: %d of %d pixels show an instance" % (shown, w * h))
    assert shown > 200


@pytest.mark.gpu
def test_gpu_two_bands_with_a_scene_sdf_equal_the_unpartitioned_frame():
    """the scene of tests/test_band_raster.py (textures, a cutout, a draw that moves in front of the second frame) with its box and its sphere baked, the torus
    without an SDF; its sessions, its in-process transport and its comparison"""
    import test_band_raster as tbr
    import test_bands as tb
    from plainrenderer_amd import tiling
    from plainrenderer_amd.frame import NO_TEXTURE, SDF_BAKE
    W, H = tb.W, tb.H
    rects = tiling.band_rects(W, H, 2)
    big = max(W, H)

    def setup(fp, be):
        tbr._set_scene(fp, normal_maps=False, casters=False)
        fp.set_scene_sdf([SDF_BAKE, SDF_BAKE, NO_TEXTURE])
        assert fp.scene_sdf_stats() == (2, 2, 2 * 2 * 16 ** 3)

    def before_frame(fp, be, f):
        if f == 1:
            tbr._move(fp)

    def after(fp, be):
        return be.downloadStorageBuffer(fp.storage_buffer("sdfInstances"), 16 + 96 * 2).tobytes()

    full = tbr._alone(W, H, setup=setup, before_frame=before_frame, after=after)
    halos = dict(band_gi_halo=big, band_gi_history_halo=big, band_post_halo=big, band_taa_history_halo=big, band_raster=1)
    ranks = tbr._partition(W, H, rects, settings=halos, setup=setup, before_frame=before_frame, after=after)
    bad = tbr._mismatches(lambda i: full, lambda i: ranks[i], rects, ("hist", "light"))
    assert not bad, bad
    for i in range(len(rects)):
        assert _without_texture_indices(ranks[i]["after"]) == _without_texture_indices(full["after"]), "every rank packs every instance"
    assert struct.unpack_from("<I", full["after"], 0)[0] == 2
