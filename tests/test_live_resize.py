"""Live resolution and settings changes of the frame pipeline (plr_frame.h plrf_set_resolution / plrf_update_settings): a resize before the first frame equals
creation at that size, mid-run resizes and settings changes continue against an oracle mirror that was changed the same way, the fast kernel set keeps running
across shrinking and growing frames, a minimized pipeline renders nothing, and the changes the pipeline refuses leave it untouched."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest

import passes
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.scene import Camera
from test_hiz_bloom_taa import packed_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT_RES = 32
PLR_ERR_INVALID_ARGUMENT, PLR_ERR_UNSUPPORTED = -1, -6
CAMERA_CUT_OFFSET = 320  # GlobalShaderInfo::cameraCut (frame_pipeline.h)
OPTS = dict(shadow_map_res=256, brdf_lut_res=LUT_RES, froxel_depth=16, max_sdf_instances=64)


def test_live_change_entry_points_are_exported():
    """the C-ABI of the live changes is declared and exported (no GPU: loading the library does not initialise one)"""
    from plainrenderer_amd import backend
    header = open(os.path.join(ROOT, "include", "plr_frame.h")).read()
    lib = ctypes.CDLL(backend.LIB_PATH)
    for name in ("plrf_set_resolution", "plrf_update_settings", "plrf_apply_changes"):
        assert name + "(" in header, name
        assert hasattr(lib, name), name
    plr_header = open(os.path.join(ROOT, "include", "plr.h")).read()
    for name in ("plr_recreate_image", "plr_resize_storage_buffer"):
        assert name + "(" in plr_header and hasattr(lib, name), name


def _camera(f, w, h):
    return Camera.look((15.0 + 0.03 * f, -7.0, -6.0 + 0.05 * f), (0.0, 0.16, 1.0), aspect=w / h)


class Scene:
    """the synthetic inputs of one scene at every size asked for; what does not follow the screen (SDF volumes and scene, shadow maps, LUTs, noise) is the first
    upload's, as the pipeline keeps it across a resize"""

    def __init__(self, seed):
        self.scene = synth.SynthScene(grid=4, cell=8.0, seed_id=seed)
        self.base = None
        self.cache = {}

    def inputs(self, w, h):
        if (w, h) not in self.cache:
            inp = synth_inputs(self.scene, w, h)
            if self.base is not None:
                for a in ("instance_bytes", "bb_bytes", "volumes", "noise", "sky", "transmission", "sun", "shadow_info", "shadow_maps", "vol_settings",
                          "volume_indices", "instance_bytes_patched"):
                    setattr(inp, a, getattr(self.base, a))
            self.cache[(w, h)] = inp
        return self.cache[(w, h)]

    def upload_all(self, fp):
        inp = self.inputs(fp.width, fp.height)
        inp.upload(fp)
        if self.base is None:
            self.base = inp
        return inp

    def upload_screen(self, fp):
        """what follows the screen: the G-buffer and the froxel volume"""
        inp = self.inputs(fp.width, fp.height)
        be, gb = fp.be, inp.gb
        for i in (0, 1):
            be.uploadImage(fp.image("depth%d" % i), gb["depth"])
            be.uploadImage(fp.image("motion%d" % i), gb["motion"])
        for n in ("normal", "albedo", "specular"):
            be.uploadImage(fp.image(n), gb[n])
        be.uploadImage(fp.image("volumetricIntegrationVolume"), inp.froxel)
        return inp


def synth_inputs(scene, w, h):
    from plainrenderer_amd.frame import SyntheticInputs
    return SyntheticInputs(scene, _camera(1, w, h), _camera(0, w, h), w, h, sdf_res=16, shadow_res=256, froxel_depth=16, sun_direction=(0.35, -0.8, 0.45))


def _frame(fp, f):
    fp.frame(_camera(f + 1, max(fp.width, 1), max(fp.height, 1)), 1.0 / 60.0, 0.5 + f / 60.0)


def _oracle_frame(fp, ora):
    be = fp.be
    frustum = be.downloadUniformBuffer(fp.uniform_buffer("sdfCameraFrustum"), 192).tobytes()
    influence = float(be.downloadUniformBuffer(fp.uniform_buffer("sdfInfluenceRange"), 4, dtype=np.float32)[0])
    ora.frame(fp.submitted_globals(), fp.resolve_weights(), frustum, influence)


def _camera_cut(fp):
    return struct.unpack_from("<I", fp.submitted_globals(), CAMERA_CUT_OFFSET)[0]


def _new_oracle(fp, inp, old=None, keep_images=False):
    """the mirror after a change: built at the pipeline's size and settings, carrying what the pipeline carries (light, frame counter, render target index, LUT);
    keep_images: also the colour targets and TAA history (a trace-resolution change re-creates the GI images only)"""
    from oracle_frame import OracleFrame
    ora = OracleFrame(inp, fp.width, fp.height, LUT_RES, fp.settings)
    if old is not None:
        ora.light, ora.cpu_frame, ora.rt_index, ora.brdf_lut = old.light, old.cpu_frame, old.rt_index, old.brdf_lut
        if keep_images:
            ora.color, ora.post1, ora.taa_hist = old.color, old.post1, old.taa_hist
    return ora


def _check_exact(fp, ora, what):
    """tests/test_full_frame.py's statement"""
    be, W, H = fp.be, fp.width, fp.height
    light = be.downloadStorageBuffer(fp.storage_buffer("light"), 20, dtype=np.float32)
    assert np.array_equal(light.view(np.uint32), np.frombuffer(ora.light, np.uint32)), "light buffer, " + what
    hist = be.downloadStorageBuffer(fp.storage_buffer("histogram"), 512, dtype=np.uint32)
    import pass_parity
    assert np.array_equal(hist, ora.hist), "histogram, " + what
    if pass_parity.histogram_counts_every_pixel(W, H, hist.size) and ora.hist.sum() > 0:  # (the first frame after a resize bins a zero-filled colour target)
        assert int(hist.sum()) == W * H, "histogram total, " + what
    tiles = be.downloadStorageBuffer(fp.storage_buffer("sdfCulledTiles"), ora.tiles.nbytes, dtype=np.uint32).reshape(-1, passes.TILE_UINTS)
    assert np.array_equal(tiles[:, 0], ora.tiles.reshape(-1, passes.TILE_UINTS)[:, 0]), "culled tiles, " + what
    if ora.half:
        ysh = be.downloadImage(fp.image("giFullResYSH"), 0, np.uint16)
        assert np.array_equal(pixfmt.unpack_half(ysh), pixfmt.unpack_half(ora.full_y)), "GI upscale, " + what
    else:
        ysh = be.downloadImage(fp.image("giHistoryYSH0"), 0, np.uint16)
        assert np.array_equal(pixfmt.unpack_half(ysh), pixfmt.unpack_half(ora.hist_y[0])), "GI history, " + what
    cur = ora.rt_index
    assert packed_close(be.downloadImage(fp.image("color%d" % cur), 0, np.uint32), ora.color[cur], 0.0), "shaded colour, " + what
    assert packed_close(be.downloadImage(fp.image("post1"), 0, np.uint32), ora.post1, 0.0), "TAA+bloom output, " + what
    sw = be.downloadImage(fp.image("swapchain"), 0, np.uint8).reshape(H, W, 4).astype(int)
    d = np.abs(sw - ora.swapchain.astype(int))
    assert d.max() <= 1 and (d != 0).mean() < 0.02, "tonemapped swapchain, " + what


def _check_fast(fp, ora, what):
    """pass_parity.check_frame_end_to_end's tolerance for a fast frame against the oracle: colour and swapchain statistics, no general kernel; the histogram
    bins the same number of pixels as the oracle's (its every-pixel rule is stated for the sizes of the parity tests, and the first frame after a resize bins
    a zero-filled colour target)"""
    import parity
    import pass_parity
    be, W, H = fp.be, fp.width, fp.height
    post, swap = be.downloadImage(fp.image("post1"), 0, np.uint32), be.downloadImage(fp.image("swapchain"), 0, np.uint8)
    hist = be.downloadStorageBuffer(fp.storage_buffer("histogram"), 512, dtype=np.uint32)
    pass_parity.fast_only(be, what)
    d = parity.r11g11b10_code_diff(post, ora.post1)
    sw = np.abs(swap.astype(int).reshape(-1) - ora.swapchain.astype(int).reshape(-1))
    lit, ref = pixfmt.unpack_r11g11b10(post), pixfmt.unpack_r11g11b10(ora.post1)
    pass_parity.report("frame", within_one_code=float((d <= 1).all(axis=1).mean()), swapchain_max_lsb=int(sw.max()), histogram_total=int(hist.sum()), size="%dx%d" % (W, H))
    assert np.isfinite(lit).all()
    assert (~(d <= 1).all(axis=1)).sum() <= pass_parity.count_cap(5e-3, W * H), what
    assert (~(d <= 4).all(axis=1)).sum() <= pass_parity.count_cap(5e-4, W * H), what
    assert (sw > 1).sum() <= pass_parity.count_cap(1e-4, sw.size), what
    assert float(np.abs(lit - ref).mean() / ref.mean()) <= 2e-3, what
    assert int(hist.sum()) == int(ora.hist.sum()), "histogram total, " + what


def _outputs(fp):
    """every output image of the frame; in the fast set an intermediate a fused launch kept in registers (pass fusion level 2) cannot be read: None"""
    from plainrenderer_amd.backend import PlrError
    be = fp.be
    out = {}
    for n in ("swapchain", "post1", "color0", "color1", "giHistoryYSH0", "giHistoryYSH1", "giHistoryCoCg0", "giHistoryCoCg1", "giFullResYSH", "giFullResCoCg"):
        try:
            out[n] = be.downloadImage(fp.image(n), 0, np.uint8).copy()
        except PlrError as e:
            if be.getMathMode() != 1 or "was not written in the last frame" not in str(e):
                raise
            out[n] = None
    out["light"] = be.downloadStorageBuffer(fp.storage_buffer("light"), 20).copy()
    out["histogram"] = be.downloadStorageBuffer(fp.storage_buffer("histogram"), 512).copy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True])
def test_gpu_resize_before_first_frame_equals_creation_at_that_size(backend, fast):
    from plainrenderer_amd.frame import FramePipeline
    results = []
    try:
        backend.setMathMode(fast)
        for resized in (True, False):
            sc = Scene(700)
            fp = FramePipeline(backend, 256, 144, **OPTS) if resized else FramePipeline(backend, 322, 182, **OPTS)
            if resized:
                fp.set_resolution(322, 182)
                fp.apply_changes()
                assert backend.getImageDescription(fp.image("color0")).width == 322
            sc.upload_all(fp)
            frames = []
            for f in range(4):
                _frame(fp, f)
                frames.append(_outputs(fp))
                if fast:
                    import pass_parity
                    pass_parity.fast_only(backend, "frame %d" % f)
            results.append(frames)
            fp.destroy()
    finally:
        backend.setMathMode(False)
    for f in range(4):
        assert results[0][f]["swapchain"] is not None and results[0][f]["post1"] is not None
        for name, a in results[0][f].items():
            b = results[1][f][name]
            assert (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b)), "%s, frame %d" % (name, f)


def _run_sizes(backend, fp, sc, ora, sizes, check, f0=0):
    """frames at each (w, h, n) in turn: a resize, the G-buffer of the new size, n frames beside a fresh mirror; -> next frame number"""
    f = f0
    for w, h, n in sizes:
        if (w, h) != (fp.width, fp.height):
            fp.set_resolution(w, h)
            fp.apply_changes()
            ora[0] = _new_oracle(fp, sc.upload_screen(fp), ora[0])
            cut_expected = True
        else:
            cut_expected = False
        for k in range(n):
            _frame(fp, f)
            assert _camera_cut(fp) == (1 if cut_expected and k == 0 else 0), "camera cut, %d x %d frame %d" % (w, h, k)
            _oracle_frame(fp, ora[0])
            check(fp, ora[0], "%d x %d, frame %d after the resize" % (w, h, k))
            f += 1
    return f


@pytest.mark.gpu
def test_gpu_mid_run_resize_matches_oracle(backend):
    from plainrenderer_amd.frame import FramePipeline
    sc = Scene(701)
    fp = FramePipeline(backend, 256, 144, **OPTS)
    ora = [_new_oracle(fp, sc.upload_all(fp))]
    shadow_before = backend.downloadImage(fp.image("shadow2"), 0, np.uint8).copy()
    _run_sizes(backend, fp, sc, ora, [(256, 144, 3), (323, 183, 3), (256, 144, 2)], _check_exact)
    assert fp.cpu_frame_index() == 8
    assert np.array_equal(backend.downloadImage(fp.image("shadow2"), 0, np.uint8), shadow_before), "a shadow map does not follow the screen"
    fp.destroy()


@pytest.mark.gpu
def test_gpu_fast_set_across_shrink_and_grow(backend):
    from plainrenderer_amd.frame import FramePipeline
    sc = Scene(702)
    try:
        backend.setMathMode(True)
        fp = FramePipeline(backend, 256, 144, **OPTS)
        ora = [_new_oracle(fp, sc.upload_all(fp))]
        f = _run_sizes(backend, fp, sc, ora, [(256, 144, 3), (323, 183, 3), (256, 144, 2), (1000, 563, 2)], _check_fast)
        allocated = None
        for i in range(20):  # one frame each: freed allocations come back at the other size
            w, h = (323, 183) if i % 2 == 0 else (256, 144)
            f = _run_sizes(backend, fp, sc, ora, [(w, h, 1)], _check_fast, f)
            if i == 1:
                allocated = backend.getMemoryStats()[0]
        assert backend.getMemoryStats()[0] <= allocated, "allocated bytes grow with every resize cycle"
        fp.destroy()
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_minimized_renders_nothing(backend):
    from plainrenderer_amd.frame import FramePipeline
    sc = Scene(703)
    fp = FramePipeline(backend, 256, 144, **OPTS)
    ora = _new_oracle(fp, sc.upload_all(fp))
    for f in range(2):
        _frame(fp, f)
        _oracle_frame(fp, ora)
    _check_exact(fp, ora, "before minimizing")
    index, swap = fp.cpu_frame_index(), backend.downloadImage(fp.image("swapchain"), 0, np.uint8).copy()
    fp.set_resolution(0, 144)
    for f in range(2, 4):
        _frame(fp, f)
        assert fp.cpu_frame_index() == index
        assert np.array_equal(backend.downloadImage(fp.image("swapchain"), 0, np.uint8), swap)
    fp.set_resolution(256, 144)
    for f in range(4, 6):
        _frame(fp, f)
        assert _camera_cut(fp) == (1 if f == 4 else 0)
        _oracle_frame(fp, ora)
        _check_exact(fp, ora, "frame %d after the restore" % (f - 4))
    fp.destroy()


@pytest.mark.gpu
def test_gpu_live_settings_match_oracle(backend):
    from plainrenderer_amd.frame import FramePipeline
    sc = Scene(704)
    fp = FramePipeline(backend, 256, 144, **OPTS)
    ora = _new_oracle(fp, sc.upload_all(fp))
    f = 0

    def run(n, what, cut_first=False):
        nonlocal f
        for k in range(n):
            _frame(fp, f)
            assert _camera_cut(fp) == (1 if cut_first and k == 0 else 0), what
            _oracle_frame(fp, ora)
            _check_exact(fp, ora, "%s, frame %d" % (what, k))
            f += 1

    run(2, "initial settings")
    for change in (dict(taa_history_sampling_tech=1), dict(taa_use_clipping=0), dict(bloom_strength=0.2)):
        fp.update_settings(**change)
        ora.s = fp.settings
        run(2, str(change))
    lut_before = backend.downloadImage(fp.image("brdfLut"), 0, np.uint16).copy()
    fp.update_settings(diffuse_brdf=0)
    ora.s, ora.brdf_lut = fp.settings, None
    run(2, "diffuse_brdf 0")
    lut = backend.downloadImage(fp.image("brdfLut"), 0, np.uint16).copy()
    assert not np.array_equal(lut, lut_before), "the BRDF LUT was not re-baked"
    fp.update_settings(sdf_half_res_trace=0)
    fp.apply_changes()
    d = backend.getImageDescription(fp.image("giHistoryYSH0"))
    assert (d.width, d.height) == (256, 144), "GI images at full resolution"
    ora = _new_oracle(fp, sc.inputs(256, 144), ora, keep_images=True)
    run(2, "sdf_half_res_trace 0", cut_first=True)
    fp.destroy()
    # (after fp's last frame: pipelines of one backend share its global uniform buffer binding, the last one created owns it)
    twin = FramePipeline(backend, 256, 144, diffuse_brdf=0, **OPTS)
    sc.upload_all(twin)
    _frame(twin, 0)
    assert np.array_equal(backend.downloadImage(twin.image("brdfLut"), 0, np.uint16), lut), "BRDF LUT of a pipeline created with diffuse_brdf 0"
    twin.destroy()


@pytest.mark.gpu
def test_gpu_refused_changes_leave_the_pipeline_untouched(backend):
    from plainrenderer_amd.frame import FramePipeline
    from plainrenderer_amd.backend import PlrError
    outs = []
    for refuse in (True, False):  # the pipeline and its untouched twin, one after the other (pipelines of one backend share its global uniform buffer binding)
        sc = Scene(705)
        fp = FramePipeline(backend, 256, 144, **OPTS)
        sc.upload_all(fp)
        _frame(fp, 0)
        if refuse:
            for change, code in ((dict(shadow_map_res=512), PLR_ERR_UNSUPPORTED), (dict(band_row_end=64), PLR_ERR_UNSUPPORTED),
                                 (dict(width=320), PLR_ERR_INVALID_ARGUMENT)):
                with pytest.raises(PlrError) as e:
                    fp.update_settings(**change)
                assert e.value.code == code, change
            assert fp.settings.shadow_map_res == 256 and fp.settings.width == 256
        _frame(fp, 1)
        outs.append(_outputs(fp))
        fp.destroy()
    for name, a in outs[0].items():
        assert np.array_equal(a, outs[1][name]), name
    for band in (dict(band_row_begin=0, band_row_end=64), dict(band_row_begin=0, band_row_end=64, band_col_begin=0, band_col_end=128)):
        bp = FramePipeline(backend, 256, 144, **OPTS, **band)
        with pytest.raises(PlrError) as e:
            bp.set_resolution(320, 180)
        assert e.value.code == PLR_ERR_UNSUPPORTED, band
        with pytest.raises(PlrError) as e:
            bp.update_settings(bloom_strength=0.2)
        assert e.value.code == PLR_ERR_UNSUPPORTED, band
        bp.destroy()
