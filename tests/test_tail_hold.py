"""The asynchronous frame tail under every serial placement (include/plr.h plr_set_async_tail_hold; DESIGN.md "Host-side hold of the tail").

The tail of frame N (bloom chain, apply, tonemap: 12 executions) may run anywhere between its place in frame N and the next join; the hazard tracking of the backend
(hazardWithTail, tailPending, the fill checks of flushFills, the rotating copies of the global uniform buffer) claims the bytes do not depend on where. The hold knob
makes the members of that set of schedules that are fully serial reachable from the host, without any timing: position -1 launches a held tail only when something
forces it, position k in front of the k-th launch-stream operation behind it. Every test here runs frames with no host access in between (a download joins, and a
join flushes), downloads once at the end and demands the bytes of the same frames with plr_set_async_tail(0). The statistics of the getter say how many launch-stream
operations went ahead of each held tail: a placement that cannot show that proves nothing, so each test asserts them.

All at 256 x 144 (the pass list does not depend on the frame size), the fast kernel set, fusion level 2, half-resolution trace, unless a case says otherwise.
"""
import copy
import threading

import numpy as np
import pytest

from plainrenderer_amd import synth
from plainrenderer_amd.scene import Camera

W, H, N_FRAMES = 256, 144, 6
OFF, FORCED = -2, -1
INVALID_ARGUMENT, UNSUPPORTED = -1, -6
TAIL_EXECUTIONS = 12  # 5 downsamples + 5 upsamples + apply + tonemap
FP_ARGS = dict(shadow_map_res=128, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64, sdf_half_res_trace=1)
IMAGES = ["swapchain", "post1", "color0", "color1", "taaHistory0", "taaHistory1", "giHistoryYSH0", "giHistoryCoCg0"]
BUFFERS = [("histogram", 512), ("light", 20)]
WHAT = IMAGES + [name for name, _ in BUFFERS]
N_CHUNKS = 6  # the placements k = c, c + N_CHUNKS, ... <= M are case c

_cache = {}


def _cams(n, w=W, h=H):
    return [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=w / h) for i in range(n + 1)]


def _inputs(w=W, h=H):
    """generated once per size for the module; never modified (upload() gets a copy)"""
    if ("inputs", w, h) not in _cache:
        from plainrenderer_amd.frame import SyntheticInputs
        cams = _cams(1, w, h)
        _cache[("inputs", w, h)] = SyntheticInputs(synth.SynthScene(grid=4, cell=8.0, seed_id=512), cams[1], cams[0], w, h, sdf_res=16, shadow_res=128, froxel_depth=8,
                                                   sun_direction=(0.35, -0.8, 0.45))
    return _cache[("inputs", w, h)]


def _handles(fp):
    return [fp.image(name) for name in IMAGES], [fp.storage_buffer(name) for name, _ in BUFFERS]


def _download(be, handles):
    images, buffers = handles
    return [be.downloadImage(im, 0, np.uint8).copy() for im in images] + [be.downloadStorageBuffer(b, size).copy() for b, (_, size) in zip(buffers, BUFFERS)]


def _run(be, position, frames=N_FRAMES, w=W, h=H, fast=True, fusion=2, settings=None, inputs=None, cams=None, setup=None, events=None, tail=TAIL_EXECUTIONS, general_free=True):
    """`frames` frames back to back, one download at the end -> (arrays in the order of WHAT, statistics after every frame, statistics after the download).
    position None: the tail in order (plr_set_async_tail(0)), otherwise the hold position. setup(fp): before the first frame; events: {f: fn(be, fp) -> fp or None}
    run in front of frame f"""
    from plainrenderer_amd.frame import FramePipeline
    cams = cams or _cams(frames, w, h)
    be.setMathMode(fast)
    be.setPassFusion(fusion)
    fp = None
    try:
        fp = FramePipeline(be, w, h, **dict(FP_ARGS, **(settings or {})))
        copy.copy(inputs or _inputs(w, h)).upload(fp)
        if setup:
            setup(fp)
        be.setAsyncTail(position is not None)
        be.setAsyncTailHold(OFF if position is None else position)  # (clears the statistics)
        handles, snaps = _handles(fp), []
        for f in range(frames):
            if events and f in events:
                fp = events[f](be, fp) or fp
                handles = _handles(fp) if fp.handle else handles
            if fp.handle:
                fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
                enabled, n_async = be.getAsyncTail()
                assert n_async == (tail if enabled else 0) or (tail is None and enabled and n_async > 0), "executions of frame %d on the tail stream: %d" % (f, n_async)
                if fast and general_free:
                    general, which = be.getGeneralKernelExecutions()
                    assert general == 0, which
            snaps.append(be.getAsyncTailHold()[1])
        out = _download(be, handles)
        final = be.getAsyncTailHold()[1]
        assert final["held_now"] == 0 and (final["general_executions"] == 0 or not general_free), final
        return out, snaps, final
    finally:
        be.setAsyncTailHold(OFF)
        be.setAsyncTail(True)
        be.setPassFusion(2)
        be.setMathMode(False)
        if fp is not None and fp.handle:
            fp.destroy()


def _flushes(s):
    return s["flushes_join"] + s["flushes_position"] + s["flushes_next_tail"] + s["flushes_host"]


def _assert_equal(got, expected, label):
    for a, b, name in zip(got, expected, WHAT):
        assert a.shape == b.shape, (label, name)
        d = a != b
        assert not d.any(), "%s: %s differs from the in-order frames in %d bytes (first at byte %d)" % (label, name, int(d.sum()), int(np.argmax(d)))


def _in_order(be):
    if "in order" not in _cache:
        out, snaps, final = _run(be, None)
        assert all(v == 0 for s in snaps + [final] for v in s.values()), "the knob is off: no statistics"
        assert all(len(np.unique(a)) > 1 for a in out) and len(np.unique(out[1])) > 16, "the outputs are not constant"
        _cache["in order"] = out
    return _cache["in order"]


def _forced(be):
    """the position -1 run: (arrays, per frame f >= 1 the launch-stream operations that went ahead of frame f - 1's tail, M)"""
    if "forced" not in _cache:
        out, snaps, final = _run(be, FORCED)
        for f, s in enumerate(snaps):
            assert s["held_runs"] == f + 1 and s["held_executions"] == TAIL_EXECUTIONS * (f + 1) and s["held_now"] == 1, (f, s)
            assert _flushes(s) == f and s["flushes_position"] == 0 and s["flushes_host"] == 0, (f, s)
        assert final["flushes_join"] == snaps[-1]["flushes_join"] + 1, "the download's join launches the last held tail"
        ahead = [None] + [s["last_ahead"] for s in snaps[1:]]
        m = snaps[-1]["frame_operations"]
        print("tail hold -1: launch-stream operations per frame %r, ahead of the held tail per frame %r, statistics %r" % ([s["frame_operations"] for s in snaps], ahead[1:], final))
        assert snaps[-2]["frame_operations"] == m, "a steady-state frame"
        _cache["forced"] = (out, ahead, m)
    return _cache["forced"]


def test_tail_hold_refuses_bad_values():
    """needs no GPU: a position below -2 is an invalid argument whether or not a backend exists, and the Python setter takes integers only"""
    import ctypes as C
    from plainrenderer_amd import RenderBackend, backend
    lib = backend._load()
    for bad in (-3, -100, -2147483648):
        assert lib.plr_set_async_tail_hold(C.c_int(bad)) == INVALID_ARGUMENT
        assert b"plr_set_async_tail_hold" in lib.plr_last_error()
    for bad in (1.5, "1", None, True):
        with pytest.raises(TypeError):
            RenderBackend.setAsyncTailHold(object.__new__(RenderBackend), bad)
    assert (RenderBackend.TAIL_HOLD_OFF, RenderBackend.TAIL_HOLD_FORCED) == (OFF, FORCED)


@pytest.mark.gpu
def test_gpu_knob_off_keeps_no_statistics_and_early_parts_are_refused(backend):
    from plainrenderer_amd.backend import PlrError
    assert backend.getAsyncTailHold()[0] == OFF, "off by default"
    out, snaps, final = _run(backend, OFF, frames=2)  # the asynchronous tail as shipped
    assert all(v == 0 for s in snaps + [final] for v in s.values()), (snaps, final)
    with pytest.raises(PlrError) as e:
        backend.setAsyncTailHold(-3)
    assert "plr error %d" % INVALID_ARGUMENT in str(e.value)
    assert backend.getAsyncTailHold()[0] == OFF
    try:
        backend.setEarlyParts(1)
        with pytest.raises(PlrError, match="plr_set_early_parts"):
            backend.setAsyncTailHold(FORCED)
        backend.setEarlyParts(0)
        backend.setAsyncTailHold(3)
        assert backend.getAsyncTailHold()[0] == 3
        with pytest.raises(PlrError, match="plr_set_async_tail_hold"):
            backend.setEarlyParts(1)
        assert backend.getEarlyParts()[0] == 0
    finally:
        backend.setEarlyParts(0)
        backend.setAsyncTailHold(OFF)


@pytest.mark.gpu
def test_gpu_tail_launched_only_when_forced_equals_in_order(backend):
    """position -1. Measured on MI355X: a steady-state frame of this pipeline is M = 7 launch-stream operations (the first frame 9), and the join that launches the
    held tail of frame f - 1 is forced in front of operation 6 of frame f, the TAA resolve: 6 of the 7 went ahead of it, in every frame."""
    expected = _in_order(backend)
    out, ahead, m = _forced(backend)
    assert max(ahead[1:]) >= 1, "no frame's tail ran behind a launch of the next frame: %r" % (ahead,)
    assert all(a <= m for a in ahead[1:])
    _assert_equal(out, expected, "position -1")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_gpu_every_placement_of_the_tail_equals_in_order(backend, chunk):
    """k = 0 .. M, M = the launch-stream operations of a steady-state frame: the tail of frame f - 1 is launched in front of operation k of frame f, so exactly k
    operations went ahead of it - until k reaches the operation whose hazard with the tail forces the join, from where on every k is the -1 schedule (asserted)."""
    expected = _in_order(backend)
    _, ahead, m = _forced(backend)
    assert m >= 4, "a frame of %d launch-stream operations" % m
    for k in range(chunk, m + 1, N_CHUNKS):
        out, snaps, final = _run(backend, k)
        for f in range(1, N_FRAMES):
            s = snaps[f]
            assert s["held_runs"] == f + 1 and _flushes(s) == f and s["held_now"] == 1, (k, f, s)
            assert s["last_ahead"] == min(k, ahead[f]), "position %d, frame %d: %d operations went ahead (forced join behind %d)" % (k, f, s["last_ahead"], ahead[f])
        assert snaps[-1]["flushes_position"] == sum(1 for f in range(1, N_FRAMES) if k < ahead[f]), (k, snaps[-1], ahead)
        assert snaps[-1]["flushes_host"] == 0
        _assert_equal(out, expected, "position %d" % k)


def _scene_case():
    """the scene path: depth prepass raster, sun shadow raster, draw culling of both, noise generated in the first frame - per-frame fills and storage buffers"""
    import shadow_raster_cases as sc
    import test_draw_culling_frame as tdc
    from plainrenderer_amd.frame import SyntheticInputs
    if "scene" not in _cache:
        cams = tdc._cameras(W, H, 4)
        _cache["scene"] = (SyntheticInputs(sc.mesh_scene()["synth"], cams[1], cams[0], W, H, sdf_res=16, shadow_res=tdc.RES, froxel_depth=8, sun_direction=(0.35, -0.8, 0.45)), cams)
    inputs, cams = _cache["scene"]

    def setup(fp):
        fp.set_draw_culling(3)
        tdc._set_scene(fp)
        fp.generate_noise(0x5EED)
    return dict(inputs=inputs, cams=cams, setup=setup, settings=dict(shadow_map_res=tdc.RES, run_light_matrix=1))


RECORDINGS = {
    "fusion_0": lambda: dict(fusion=0, general_free=False),  # (histogramReset and histogramCombineTiles have fast kernels only inside the fused frame front)
    "fusion_1": lambda: dict(fusion=1),
    "exact_set": lambda: dict(fast=False),
    "producers": lambda: dict(settings=dict(run_volumetrics=1, run_sky_luts=1, run_light_matrix=1)),
    "scene": _scene_case,
    "separate_supersampling": lambda: dict(settings=dict(taa_use_separate_supersampling=1)),
    "odd_size": lambda: dict(w=323, h=183),
}


@pytest.mark.gpu
@pytest.mark.parametrize("recording", sorted(RECORDINGS))
def test_gpu_other_recordings_of_the_frame_equal_in_order(backend, recording):
    """three frames (two held tails that the next frame overtakes) of other pass lists, at position -1 and at the last placement in front of the forced join"""
    how = dict(RECORDINGS[recording](), frames=3)
    expected, _, _ = _run(backend, None, **how)
    out, snaps, _ = _run(backend, FORCED, **how)
    ahead = [s["last_ahead"] for s in snaps[1:]]
    print("tail hold, recording %s: operations per frame %r, ahead of the held tail %r" % (recording, [s["frame_operations"] for s in snaps], ahead))
    assert all(s["held_runs"] == f + 1 and _flushes(s) == f for f, s in enumerate(snaps)), snaps
    assert min(ahead) >= 1, "the next frame put nothing in front of a held tail: %r" % (ahead,)
    _assert_equal(out, expected, "%s, position -1" % recording)
    k = ahead[-1] - 1
    out, snaps, _ = _run(backend, k, **how)
    assert snaps[-1]["last_ahead"] == k and snaps[-1]["flushes_position"] >= 1, (k, snaps[-1])
    _assert_equal(out, expected, "%s, position %d" % (recording, k))


def _held(be):
    return be.getAsyncTailHold()[1]["held_now"]


def _resize(be, fp, held=True):
    assert _held(be) == int(held)
    fp.set_resolution(322, 182)
    fp.apply_changes()
    assert _held(be) == 0, "the resize joins the tail: the held run is launched in front of it"
    copy.copy(_inputs(322, 182)).upload(fp)


def _tail_off(be, fp, held=True):
    if held:  # (the in-order run has the tail off from the start)
        assert _held(be) == 1
        be.setAsyncTail(False)
        assert _held(be) == 0, "switching the tail off joins it"


def _destroy(be, fp, held=True):
    assert _held(be) == int(held)
    fp.destroy()  # frames 3 and 4 render nothing; a held tail is launched by the download's join, on images that outlive the pipeline
    assert _held(be) == int(held)


CHANGES = {"resize": (_resize, 5), "tail_off": (_tail_off, 3), "destroy": (_destroy, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize("change", sorted(CHANGES))
def test_gpu_changes_between_frames_launch_the_held_tail(backend, change):
    """three frames, the change while frame 2's tail is held, two more frames: the held tail is launched, not lost"""
    fn, held_runs = CHANGES[change]
    cams = _cams(5)
    expected, _, _ = _run(backend, None, frames=5, cams=cams, events={3: lambda be, fp: fn(be, fp, False)})
    out, snaps, final = _run(backend, FORCED, frames=5, cams=cams, events={3: fn})
    assert snaps[2]["held_now"] == 1 and snaps[2]["last_ahead"] >= 1, snaps[2]
    assert final["held_runs"] == held_runs and _flushes(final) == held_runs and final["flushes_position"] == 0, final
    _assert_equal(out, expected, change)


def _band_session(position, rank, rects, group, out):
    from plainrenderer_amd import RenderBackend
    try:
        be = RenderBackend(W, H, device=0)
        x0, y0, x1, y1 = rects[rank]
        big = max(W, H)
        settings = dict(band_row_begin=y0, band_row_end=y1, band_gi_halo=big, band_gi_history_halo=big, band_post_halo=big, band_taa_history_halo=big)
        res = _run(be, position, frames=3, settings=settings, setup=lambda fp: fp.attach_local_rects(group, rank, len(rects), W, H, rects), tail=None, general_free=False)
        be.shutdown()
        out[rank] = res
    except BaseException as e:  # surface failures of worker threads (and unblock the other)
        out[rank] = e
        group.abort()
        raise


def _bands(position):
    from plainrenderer_amd import tiling
    from plainrenderer_amd.frame import LocalExchangeGroup
    rects = tiling.band_rects(W, H, 2)
    group = LocalExchangeGroup(2)
    out = {}
    threads = [threading.Thread(target=_band_session, args=(position, r, rects, group, out)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    group.destroy()
    for r in range(2):
        assert r in out, "rank %d did not finish" % r
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


@pytest.mark.gpu
def test_gpu_two_bands_with_held_tails_equal_in_order():
    """two bands over the in-process transport, one backend per rank: exchange callbacks recorded with their resource list are where a join is skipped on purpose"""
    _inputs()  # (generated before the threads start)
    expected, held = _bands(None), _bands(FORCED)
    for r in range(2):
        out, snaps, final = held[r]
        ahead = [s["last_ahead"] for s in snaps[1:]]
        print("tail hold, band %d: operations per frame %r, ahead of the held tail %r" % (r, [s["frame_operations"] for s in snaps], ahead))
        assert final["held_runs"] == 3 and min(ahead) >= 1, (r, final, ahead)
        _assert_equal(out, expected[r][0], "band %d, position -1" % r)
