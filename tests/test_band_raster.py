"""Scene meshes and shadow casters in partitioned pipelines (plrf_settings.band_raster): the depth prepass restricted to each rank's raster window, the shadow
cascades rasterised in full by every rank. As tests/test_bands.py: one backend per rank on one GPU, each on its own thread, the native exchange over its
in-process transport, the exact kernel set, three frames with the slowly moving camera of test_bands._cams().

1. Whole-image halos: 2 bands and 2 x 2 tiles with band_raster = 1 against the unpartitioned pipeline, all given the same scene - the three meshes of the texture
   frame test with textures, one cutout draw, normal maps, and the caster scene of the shadow cutout test with its cutouts; run_light_matrix = 1; one draw moves in
   front of the second frame. post, colour, swapchain, histogram, light and sunShadowInfo must be byte-identical over every owned rectangle, and the raster stats
   must be the unpartitioned pipeline's.
2. Bounded halos (band_gi_halo 8, band_gi_history_halo 4): the window is sufficient. Run A: the partition with band_raster = 0, fed in front of every frame the
   G-buffer images downloaded from an unpartitioned scene pipeline; run B: the same partition with band_raster = 1 and the scene. In both every G-buffer image of
   both parities is filled with a poison word before the first frame (A's uploads then overwrite whole images, B's prepass only its window). A and B must agree
   byte for byte over every owned rectangle, and in B every texel outside the window and its wrap strips (plrf_raster_wrap_strips_for: the tiles at the opposite
   frame edge that the temporal GI filter's repeat-addressed read of last frame's motion reaches; with the window alone this comparison found 2 - 6 differing
   colour words per frame in the bottom-left tile) must still be the poison after the last frame: no pass reads the G-buffer outside them. (The scene of this test has textures and the cutout but no normal maps and no casters: run A has no scene, so its shade and its GI chain
   read one `normal` image, and the shadow maps are not windowed.)
   The shading normal has a test of its own: run B's partition with normal maps, twice, with every G-buffer image and shadingNormal filled with two different
   words. The outputs must not depend on the word, and outside window and strips shadingNormal keeps it.
3. band_raster = 1 on an unpartitioned pipeline renders the frames it renders without it.
4. The new entry points are exported.
"""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

import test_bands as tb
import test_prepass_normal_frame as tnf
import test_prepass_texture_frame as ttf
import test_shadow_alpha_frame as tsf
from plainrenderer_amd import tiling

N_FRAMES = tb.N_FRAMES
POISON = 0xDEADBEEF
TILE = 64
COMPARED = ("post", "color", "swap")
G_BUFFER = ("depth0", "depth1", "motion0", "motion1", "normal", "albedo", "specular")
CUTOFFS = [0, 128, 0]  # the sphere (its albedo texture's alpha is a pattern) is the cutout draw


def _cams(width, height):
    from plainrenderer_amd.scene import Camera
    return [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=width / height) for i in range(N_FRAMES + 1)]


_inputs_cache = {}


def _inputs(width, height):
    if (width, height) not in _inputs_cache:
        from plainrenderer_amd.frame import SyntheticInputs
        import shadow_raster_cases as sc
        cams = _cams(width, height)
        _inputs_cache[(width, height)] = SyntheticInputs(sc.mesh_scene()["synth"], cams[1], cams[0], width, height, sdf_res=16, shadow_res=128, froxel_depth=8,
                                                         sun_direction=(0.35, -0.8, 0.45))
    return _inputs_cache[(width, height)]


def _materials():
    """the texture frame test's materials with an albedo texture on the sphere, so that its cutoff tests a sampled alpha"""
    return [(0, 1), (0, 2), (1, ttf.NONE)]


def _set_scene(fp, normal_maps, casters):
    i = tnf._scene_inputs()
    fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
    fp.set_scene_textures(i["chains"], i["uvs"], _materials())
    fp.set_scene_alpha_cutoffs(CUTOFFS)
    if normal_maps:
        fp.set_scene_normal_maps(i["tangents"], [i["bitangents"][0], None, None], i["normal_textures"])
    if casters:
        c = tsf._scene_inputs()
        fp.set_shadow_casters(c["meshes"], c["draws"])
        fp.set_shadow_caster_cutouts(c["textures"], c["uvs"], c["cutouts"])


def _move(fp):
    i = tnf._scene_inputs()
    import shadow_raster_cases as sc
    models = [m.copy() for m in i["models"]]
    models[1][12:15] += np.asarray(sc.mesh_scene()["cam"].right, np.float32) * np.float32(0.4)
    fp.set_scene_mesh_transforms(models)


def _session(width, height, out, key, rect=None, rank=0, world=1, group=None, rects=None, settings=None, setup=None, before_frame=None, after=None):
    """one backend + pipeline on the calling thread, N_FRAMES frames; rect: the owned rectangle of a partitioned pipeline. setup(fp, be), before_frame(fp, be, f)
    and after(fp, be) -> anything are the run's hooks; out[key] = dict(frames, stats, window, after) or the exception"""
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import FramePipeline
    try:
        be = RenderBackend(width, height, device=0)
        be.setMathMode(False)  # the exact kernel set
        kw = dict(tb.FP_ARGS, **(settings or {}))
        if rect is not None:
            x0, y0, x1, y1 = rect
            kw.update(band_row_begin=y0, band_row_end=y1)
            if (x0, x1) != (0, width):
                kw.update(band_col_begin=x0, band_col_end=x1)
        fp = FramePipeline(be, width, height, **kw)
        copy.copy(_inputs(width, height)).upload(fp)
        if setup:
            setup(fp, be)
        if rect is not None:
            fp.attach_local_rects(group, rank, world, width, height, rects)
        cams = _cams(width, height)
        frames, stats = [], []
        for f in range(N_FRAMES):
            if before_frame:
                before_frame(fp, be, f)
            fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
            cur = (f + 1) % 2
            frames.append(dict(post=be.downloadImage(fp.image("post1"), 0, np.uint32).reshape(height, width).copy(),
                               color=be.downloadImage(fp.image("color%d" % cur), 0, np.uint32).reshape(height, width).copy(),
                               swap=be.downloadImage(fp.image("swapchain"), 0, np.uint32).reshape(height, width).copy(),
                               hist=be.downloadStorageBuffer(fp.storage_buffer("histogram"), 512, dtype=np.uint32).copy(),
                               light=be.downloadStorageBuffer(fp.storage_buffer("light"), 20, dtype=np.uint8).tobytes(),
                               shadow=be.downloadStorageBuffer(fp.storage_buffer("sunShadowInfo"), 304, dtype=np.uint8).tobytes()))
            stats.append(fp.prepass_raster_stats())
        res = dict(frames=frames, stats=stats, window=fp.raster_window(), after=after(fp, be) if after else None)
        fp.destroy()
        be.shutdown()
        out[key] = res
    except BaseException as e:  # surface failures of worker threads (and unblock the others)
        out[key] = e
        if group is not None:
            group.abort()
        raise


def _alone(width, height, **how):
    out = {}
    t = threading.Thread(target=_session, args=(width, height, out, "full"), kwargs=how)
    t.start()
    t.join(timeout=600)
    assert "full" in out, "the unpartitioned pipeline did not finish"
    if isinstance(out["full"], BaseException):
        raise out["full"]
    return out["full"]


def _partition(width, height, rects, per_rank=None, **how):
    """per_rank(rank) -> more keyword arguments of that rank's session"""
    from plainrenderer_amd.frame import LocalExchangeGroup
    n = len(rects)
    group = LocalExchangeGroup(n)
    out = {}
    threads = [threading.Thread(target=_session, args=(width, height, out, i),
                                kwargs=dict(how, rect=rects[i], rank=i, world=n, group=group, rects=rects, **(per_rank(i) if per_rank else {}))) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    group.destroy()
    for i in range(n):
        assert i in out, "rank %d did not finish" % i
        if isinstance(out[i], BaseException):
            raise out[i]
    return out


def _mismatches(a_of_rank, b_of_rank, rects, what):
    """{(frame, rank, output): differing words} over every owned rectangle; a_of_rank(i), b_of_rank(i): the two runs' results for rank i"""
    bad = {}
    for i, (x0, y0, x1, y1) in enumerate(rects):
        for f in range(N_FRAMES):
            fa, fb = a_of_rank(i)["frames"][f], b_of_rank(i)["frames"][f]
            for k in COMPARED:
                d = fa[k][y0:y1, x0:x1] != fb[k][y0:y1, x0:x1]
                if d.any():  # how many words, and where the first ones are (frame coordinates x, y)
                    bad[(f, i, k)] = (int(d.sum()), [(int(x) + x0, int(y) + y0) for y, x in np.argwhere(d)[:6]])
            for k in what:
                if not np.array_equal(fa[k], fb[k]):
                    bad[(f, i, k)] = "differs"
    return bad


def _window_for(width, height, rect, **fields):
    from plainrenderer_amd import backend
    from plainrenderer_amd.frame import PlrfSettings
    lib = backend._load()
    s = PlrfSettings()
    assert lib.plrf_default_settings(C.byref(s), C.c_uint32(width), C.c_uint32(height)) == 0
    x0, y0, x1, y1 = rect
    s.band_row_begin, s.band_row_end = y0, y1
    if (x0, x1) != (0, width):
        s.band_col_begin, s.band_col_end = x0, x1
    for k, v in fields.items():
        setattr(s, k, v)
    out = (C.c_uint32 * 4)()
    assert lib.plrf_raster_window_for(C.byref(s), out) == 0
    strips, count = (C.c_uint32 * 12)(), C.c_uint32()
    assert lib.plrf_raster_wrap_strips_for(C.byref(s), strips, C.byref(count)) == 0
    _strips[(width, height, tuple(rect))] = [tuple(int(v) for v in strips[4 * k:4 * k + 4]) for k in range(count.value)]
    return tuple(int(v) for v in out)


_strips = {}


def _expected_strips(window, gx, gy):
    """worked out here: the far tile column over the window's rows, the far tile row over its columns, the far corner - where the window touches a frame edge
    without spanning the frame in that direction"""
    x0, y0, x1, y1 = window
    far_x = None if (x0 == 0 and x1 == gx) else gx - 1 if x0 == 0 else 0 if x1 == gx else None
    far_y = None if (y0 == 0 and y1 == gy) else gy - 1 if y0 == 0 else 0 if y1 == gy else None
    out = []
    if far_x is not None:
        out.append((far_x, y0, far_x + 1, y1))
    if far_y is not None:
        out.append((x0, far_y, x1, far_y + 1))
    if far_x is not None and far_y is not None:
        out.append((far_x, far_y, far_x + 1, far_y + 1))
    return out


# ------------------------------------------------------------------ 1. whole-image halos
@pytest.mark.gpu
@pytest.mark.parametrize("grid", [(1, 2), (2, 2)], ids=["2_bands", "2x2_tiles"])
def test_gpu_partitions_that_rasterise_reproduce_the_unpartitioned_scene_frame(grid):
    W, H = tb.W, tb.H
    rects = tiling.band_rects(W, H, grid[1]) if grid[0] == 1 else tiling.tile_rects(W, H, *grid)
    big = max(W, H)

    def setup(fp, be):
        _set_scene(fp, normal_maps=True, casters=True)

    def before_frame(fp, be, f):
        if f == 1:
            _move(fp)

    full = _alone(W, H, settings=dict(run_light_matrix=1), setup=setup, before_frame=before_frame)
    assert full["stats"][0][2] > 0, "the scene is drawn"
    assert full["window"] == (0, 0, (W + TILE - 1) // TILE, (H + TILE - 1) // TILE)
    halos = dict(band_gi_halo=big, band_gi_history_halo=big, band_post_halo=big, band_taa_history_halo=big, band_raster=1, run_light_matrix=1)
    ranks = _partition(W, H, rects, settings=halos, setup=setup, before_frame=before_frame)
    bad = _mismatches(lambda i: full, lambda i: ranks[i], rects, ("hist", "light", "shadow"))
    assert not bad, bad
    for i in range(len(rects)):
        assert ranks[i]["stats"] == full["stats"], "rank %d: raster stats %r, unpartitioned %r" % (i, ranks[i]["stats"], full["stats"])
        assert ranks[i]["window"] == full["window"], "whole-image halos: the window is the whole frame"


# ------------------------------------------------------------------ 2. bounded halos: the window is sufficient
SMALL_HALOS = dict(band_gi_halo=8, band_gi_history_halo=4)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,grid", [(256, 384, (1, 2)), (384, 384, (2, 2))], ids=["2_bands", "2x2_tiles"])
def test_gpu_no_pass_reads_the_g_buffer_outside_the_raster_window(width, height, grid):
    rects = tiling.band_rects(width, height, grid[1]) if grid[0] == 1 else tiling.tile_rects(width, height, *grid)
    gx, gy = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    windows = [_window_for(width, height, r, **SMALL_HALOS) for r in rects]
    for w, r in zip(windows, rects):  # (here, on the CPU) every rank's window leaves at least one tile row or column of the frame out, its wrap strips included
        assert (w[2] - w[0] < gx) or (w[3] - w[1] < gy), "the window %r is the whole %d x %d grid: take a larger frame" % (w, gx, gy)
        rows, cols = set(range(w[1], w[3])), set(range(w[0], w[2]))
        for sx0, sy0, sx1, sy1 in _strips[(width, height, tuple(r))]:
            if (sx0, sx1) == (w[0], w[2]):
                rows |= set(range(sy0, sy1))
            if (sy0, sy1) == (w[1], w[3]):
                cols |= set(range(sx0, sx1))
        assert len(rows) < gy or len(cols) < gx, "window %r and its strips leave no tile row or column out: take a larger frame" % (w,)
    poison = np.full(width * height, POISON, np.uint32)

    def scene(fp, be):
        _set_scene(fp, normal_maps=False, casters=False)

    # the unpartitioned scene pipeline: its G-buffer after every frame
    recorded = []

    def keep(fp, be, f):
        if f > 0:
            recorded.append(_download_g_buffer(fp, be, f - 1, width, height))

    def keep_last(fp, be):
        recorded.append(_download_g_buffer(fp, be, N_FRAMES - 1, width, height))

    _alone(width, height, setup=scene, before_frame=keep, after=keep_last)
    assert len(recorded) == N_FRAMES and all((g["depth"] != 0).any() for g in recorded)

    def fill_poison(fp, be):
        for name in G_BUFFER:
            be.uploadImage(fp.image(name), poison)

    def feed(fp, be, f):
        target = (f + 1) % 2
        for name, image in (("depth", "depth%d" % target), ("motion", "motion%d" % target), ("normal", "normal"), ("albedo", "albedo"), ("specular", "specular")):
            be.uploadImage(fp.image(image), recorded[f][name])

    def poisoned_scene(fp, be):
        scene(fp, be)
        fill_poison(fp, be)

    def g_buffer_after(fp, be):
        return {name: be.downloadImage(fp.image(name), 0, np.uint32).reshape(height, width).copy() for name in G_BUFFER}

    a = _partition(width, height, rects, settings=dict(SMALL_HALOS, band_raster=0), setup=fill_poison, before_frame=feed)
    b = _partition(width, height, rects, settings=dict(SMALL_HALOS, band_raster=1), setup=poisoned_scene, after=g_buffer_after)
    bad = _mismatches(lambda i: a[i], lambda i: b[i], rects, ("hist", "light", "shadow"))
    assert not bad, "the raster window is too small for what a pass reads: %r" % (bad,)
    for i, (x0, y0, x1, y1) in enumerate(windows):
        assert b[i]["window"] == (x0, y0, x1, y1)
        outside = np.ones((height, width), bool)
        outside[y0 * TILE:y1 * TILE, x0 * TILE:x1 * TILE] = False
        strips = _strips[(width, height, tuple(rects[i]))]
        assert strips == _expected_strips(windows[i], gx, gy), "rank %d: wrap strips %r" % (i, strips)
        for sx0, sy0, sx1, sy1 in strips:  # the tiles at the opposite frame edge that the temporal GI filter's repeat-addressed motion read reaches
            outside[sy0 * TILE:sy1 * TILE, sx0 * TILE:sx1 * TILE] = False
        assert outside.any(), "window and strips leave tiles out"
        for name, words in b[i]["after"].items():
            touched = int((words[outside] != POISON).sum())
            assert touched == 0, "rank %d: %d texels of %s outside the window %r were written" % (i, touched, name, windows[i])
            inside_written = int((words[~outside] != POISON).sum())
            assert inside_written > 0, "rank %d: %s inside the window was never written" % (i, name)
        # inside the window the current frame's images are the unpartitioned pipeline's
        last = (N_FRAMES) % 2
        for name, image in (("depth", "depth%d" % last), ("motion", "motion%d" % last), ("normal", "normal"), ("albedo", "albedo"), ("specular", "specular")):
            assert np.array_equal(b[i]["after"][image][~outside], recorded[N_FRAMES - 1][name][~outside]), "rank %d: %s inside the window differs from the unpartitioned pipeline's" % (i, name)
        assert b[i]["stats"][-1][2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("width,height,grid", [(256, 384, (1, 2)), (384, 384, (2, 2))], ids=["2_bands", "2x2_tiles"])
def test_gpu_no_pass_reads_the_shading_normal_outside_the_raster_window(width, height, grid):
    """the bounded-halo partition with band_raster = 1 and the scene WITH normal maps: every G-buffer image, shadingNormal included, is filled with one word
    before the first frame - 0xDEADBEEF in one run, 0x12345678 in the other. No pass reads a texel outside window and strips if and only if the word does not
    show: the two runs' outputs must be equal byte for byte over every owned rectangle, and afterwards every texel of shadingNormal (and of the other images)
    outside window and strips is still the run's word, while shadingNormal inside the window was written"""
    rects = tiling.band_rects(width, height, grid[1]) if grid[0] == 1 else tiling.tile_rects(width, height, *grid)
    windows = [_window_for(width, height, r, **SMALL_HALOS) for r in rects]
    images = G_BUFFER + ("shadingNormal",)

    def run(word):
        fill = np.full(width * height, word, np.uint32)

        def setup(fp, be):
            _set_scene(fp, normal_maps=True, casters=False)  # (creates shadingNormal)
            for name in images:
                be.uploadImage(fp.image(name), fill)

        def after(fp, be):
            return {name: be.downloadImage(fp.image(name), 0, np.uint32).reshape(height, width).copy() for name in images}
        return _partition(width, height, rects, settings=dict(SMALL_HALOS, band_raster=1), setup=setup, after=after)

    words = (POISON, 0x12345678)
    runs = [run(word) for word in words]
    bad = _mismatches(lambda i: runs[0][i], lambda i: runs[1][i], rects, ("hist", "light", "shadow"))
    assert not bad, "a pass reads the G-buffer outside the raster window and its strips: %r" % (bad,)
    for word, ranks in zip(words, runs):
        for i, (x0, y0, x1, y1) in enumerate(windows):
            outside = np.ones((height, width), bool)
            outside[y0 * TILE:y1 * TILE, x0 * TILE:x1 * TILE] = False
            for sx0, sy0, sx1, sy1 in _strips[(width, height, tuple(rects[i]))]:
                outside[sy0 * TILE:sy1 * TILE, sx0 * TILE:sx1 * TILE] = False
            assert outside.any()
            for name, texels in ranks[i]["after"].items():
                touched = int((texels[outside] != word).sum())
                assert touched == 0, "rank %d: %d texels of %s outside the window %r were written" % (i, touched, name, windows[i])
            inside = ~outside
            assert (ranks[i]["after"]["shadingNormal"][inside] != word).all(), "rank %d: shadingNormal inside the window and strips is written everywhere" % i
    inside_equal = [np.array_equal(runs[0][i]["after"]["shadingNormal"][y0 * TILE:y1 * TILE, x0 * TILE:x1 * TILE],
                                   runs[1][i]["after"]["shadingNormal"][y0 * TILE:y1 * TILE, x0 * TILE:x1 * TILE]) for i, (x0, y0, x1, y1) in enumerate(windows)]
    assert all(inside_equal)
    assert any((runs[0][i]["after"]["shadingNormal"] != runs[0][i]["after"]["normal"]).any() for i in range(len(rects))), "the normal maps show"


def _download_g_buffer(fp, be, f, width, height):
    target = (f + 1) % 2
    names = dict(depth="depth%d" % target, motion="motion%d" % target, normal="normal", albedo="albedo", specular="specular")
    return {k: be.downloadImage(fp.image(v), 0, np.uint32).reshape(height, width).copy() for k, v in names.items()}


# ------------------------------------------------------------------ 3. the flag on an unpartitioned pipeline
@pytest.mark.gpu
def test_gpu_band_raster_on_an_unpartitioned_pipeline_changes_nothing():
    W, H = tb.W, tb.H

    def setup(fp, be):
        _set_scene(fp, normal_maps=True, casters=True)

    runs = [_alone(W, H, settings=dict(band_raster=flag), setup=setup) for flag in (0, 1)]
    for f in range(N_FRAMES):
        for k in COMPARED + ("hist",):
            assert np.array_equal(runs[0]["frames"][f][k], runs[1]["frames"][f][k]), "%s of frame %d depends on band_raster" % (k, f)
        assert runs[0]["frames"][f]["light"] == runs[1]["frames"][f]["light"] and runs[0]["frames"][f]["shadow"] == runs[1]["frames"][f]["shadow"]
    assert runs[0]["stats"] == runs[1]["stats"] and runs[0]["stats"][0][2] > 0


@pytest.mark.gpu
def test_gpu_without_band_raster_a_partition_still_refuses_and_with_it_keeps_its_size(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import FramePipeline
    i = tnf._scene_inputs()
    for flag in (0, 1):
        fp = FramePipeline(backend, ttf.W, ttf.H, band_row_begin=0, band_row_end=ttf.H, band_raster=flag, **ttf.FP_ARGS)
        try:
            if flag:
                fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
            else:
                with pytest.raises(PlrError, match="setSceneMeshes: a band / tile pipeline cannot rasterise scene meshes") as e:
                    fp.set_scene_meshes(i["meshes"], ttf._draws(i["models"]))
                assert e.value.code == ttf.UNSUPPORTED
            with pytest.raises(PlrError, match="setResolution: a band / tile pipeline cannot change size") as e:
                fp.set_resolution(64, 64)
            assert e.value.code == ttf.UNSUPPORTED
        finally:
            fp.destroy()


# ------------------------------------------------------------------ 4. exports
def test_the_two_window_functions_are_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    assert hasattr(lib, "plrf_raster_window_for") and hasattr(lib, "plrf_get_raster_window") and hasattr(lib, "plrf_raster_wrap_strips_for")
