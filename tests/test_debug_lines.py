"""The "debugGeometry.comp" pass through the C-ABI pass record against tests/debug_lines_reference.py, in both math modes: every word of the colour image, of the
depth image and of the counters must be bit-identical.

Cases: tests/debug_lines_cases.py at 70 x 37 (ragged, odd pitch) and 256 x 144 - x-major and y-major segments of 1, 63, 64, 65, 128 and 129 steps (the chunk
boundaries), a diagonal across the frame, segments partly and wholly off each side, zero length, a line hidden behind nearer geometry, one at bit-equal depth,
lines over depth 0, two crossing lines at bit-equal zf, 300 segments through one pixel with distinct and with equal depths, 1, 63, 64, 65 and 1000 segments, boxes
of draws and SDF instances, a NaN in a matrix and a transformIndex out of range, a culled draw array, and a perspective view. Then several executions in a row of
one pass - so that they share its scratch - with different segments and frame sizes: a key left behind would show. Then each launcher refusal.
The images are pre-filled (the pass writes winners only), and the inputs are compared with what was uploaded afterwards.
"""
import struct

import numpy as np
import pytest

import debug_lines_cases as dc
from passes import global_binding
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

F = ImageFormat
DRAW, BOUNDS, TRANSFORMS, SDF_BOXES, LINES, STATS = 0, 1, 2, 3, 4, 5
COLOR, DEPTH = 0, 1
SOURCES = {DRAW: "draws", BOUNDS: "bounds", TRANSFORMS: "transforms", SDF_BOXES: "sdf_boxes", LINES: "lines"}


def _global(view_projection):
    return np.asarray(view_projection, np.float32).reshape(16).tobytes() + bytes(340 - 64)


def _counts(c):
    return (len(c["draws"]) if "draws" in c else 0, len(c["sdf_boxes"]) if "sdf_boxes" in c else 0, len(c["lines"]) if "lines" in c else 0, 1 if c.get("draws_culled") else 0)


def gpu_draw(be, cases, push=None, sizes=None, read_only=(), alias=None, omit=(), formats=None, depth_size=None, dispatch=(1, 1, 1)):
    """runs the pass once per case, all in one frame on one pass (one scratch) -> [(color, depth, stats 8 uint32, inputs unchanged)]. All cases share a viewProjection"""
    sizes, formats = sizes or {}, formats or {}
    global_binding(be).set(_global(cases[0]["view_projection"]))
    p = be.createComputePass("debugGeometry.comp", [], "Debug geometry test")
    be.newFrame()
    made = []
    for c in cases:
        assert np.array_equal(c["view_projection"], cases[0]["view_projection"])
        w, h = c["width"], c["height"]
        images = {COLOR: be.createImage(image_desc_2d(w, h, formats.get(COLOR, F.R11G11B10_uFloat)), c["color"]),
                  DEPTH: be.createImage(image_desc_2d(*(depth_size or (w, h)), formats.get(DEPTH, F.Depth32)), c["depth"] if depth_size is None else np.zeros(depth_size[::-1], np.float32))}
        inputs = {b: np.ascontiguousarray(c[name]).tobytes() for b, name in SOURCES.items() if name in c and len(c[name])}
        buffers = {b: be.createStorageBuffer(sizes.get(b, len(data)), data[:sizes.get(b, len(data))]) for b, data in inputs.items()}
        n = sizes.get(STATS, 32)
        buffers[STATS] = be.createStorageBuffer(n, b"\xa5" * n)
        if alias:
            buffers[alias[0]] = buffers[alias[1]]
        for b in omit:
            buffers.pop(b, None)
        be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
            storageImages=[ImageResource(images[b], 0, b) for b in (COLOR, DEPTH) if ("image", b) not in omit],
            storageBuffers=[StorageBufferResource(hd, (b != STATS) != (b in read_only), b) for b, hd in sorted(buffers.items())]),
            push if push is not None else struct.pack("<4I", *_counts(c)), dispatch))
        made.append((c, images, buffers, inputs))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = []
    for c, images, buffers, inputs in made:
        w, h = c["width"], c["height"]
        color = be.downloadImage(images[COLOR], 0, np.uint32).reshape(h, w).copy()
        depth = be.downloadImage(images[DEPTH], 0, np.float32).reshape(h, w).copy()
        stats = be.downloadStorageBuffer(buffers[STATS], 32, dtype=np.uint32).copy()
        unchanged = all(be.downloadStorageBuffer(buffers[b], len(data), dtype=np.uint8).tobytes() == data for b, data in inputs.items())
        out.append((color, depth, stats, unchanged))
    return out


def _compare(what, got, want):
    color, depth, stats, unchanged = got
    rcolor, rdepth, rstats = want[0], want[1], want[2]
    differing = int((color != rcolor).sum()), int((depth.view(np.uint32) != rdepth.view(np.uint32)).sum())
    counters = dict(zip(dc.ref.STAT_NAMES, stats[:6].tolist()))
    print("debug lines %-60s colour words differing %d, depth words differing %d, counters %r (reference %r)" % (what, differing[0], differing[1], counters, rstats))
    assert differing == (0, 0), "%s: %d colour and %d depth words differ from the reference" % (what, *differing)
    assert counters == rstats and stats[6] == 0 and stats[7] == 0, what
    assert unchanged, "%s: the pass modified an input" % what


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("size", dc.SIZES, ids=["%dx%d" % s for s in dc.SIZES])
def test_gpu_debug_lines_are_bit_identical_to_the_reference(backend, size, fast):
    backend.setMathMode(fast)
    try:
        for name, c in dc.named_cases(*size):
            got = gpu_draw(backend, [c])[0]
            general = backend.getGeneralKernelExecutions()
            _compare("%dx%d %-5s %s" % (*size, "fast" if fast else "exact", name), got, dc.reference(*size, name))
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


@pytest.mark.gpu
def test_gpu_executions_in_a_row_leave_no_key_behind(backend):
    """one pass, one scratch: different segments over the same pixels, then a larger frame (the keys grow over the last execution's records), a smaller one again, an
    execution without a segment, and the first once more"""
    small, large = dict(dc.named_cases(70, 37)), dict(dc.named_cases(256, 144))
    order = [(70, 37, "300 through one pixel, equal depths"), (70, 37, "diagonal"), (256, 144, "1000 segments"), (70, 37, "steps"), (256, 144, "crossing at equal depth"),
             (70, 37, "300 through one pixel, equal depths")]
    cases = [(small if w == 70 else large)[name] for w, h, name in order]
    empty = dc.case(70, 37)
    results = gpu_draw(backend, cases[:3] + [empty] + cases[3:])
    color, depth, stats, _ = results.pop(3)
    assert np.array_equal(color, empty["color"]) and np.array_equal(depth, empty["depth"]) and not stats.any(), "an execution without a segment clears the counters and writes nothing"
    for (w, h, name), got in zip(order, results):
        _compare("in a row: %dx%d %s" % (w, h, name), got, dc.reference(w, h, name))


@pytest.mark.gpu
def test_gpu_launcher_refuses_what_it_cannot_run(backend):
    """fails loudly: a missing, mis-formatted or mis-sized image, a missing or short buffer, a read-only or aliased stats buffer, a malformed push record"""
    from plainrenderer_amd.backend import PlrError
    boxes, lines = dict(dc.named_cases(70, 37))["boxes"], dict(dc.named_cases(70, 37))["63 segments"]
    refusals = [("missing storage image at binding 0", dict(omit=(("image", COLOR),))), ("missing storage image at binding 1", dict(omit=(("image", DEPTH),))),
                ("colour.*expects R11G11B10", dict(formats={COLOR: F.RGBA8})), ("depth.*expects Depth32", dict(formats={DEPTH: F.R11G11B10_uFloat})),
                ("one size", dict(depth_size=(70, 36))),
                ("draws", dict(sizes={DRAW: 24 * 5 - 4})), ("bounds", dict(sizes={BOUNDS: 24 * 5 - 4})), ("transforms", dict(omit=(TRANSFORMS,))),
                ("sdfBoxes", dict(sizes={SDF_BOXES: 63})), ("lines", dict(sizes={LINES: 32})), ("stats", dict(sizes={STATS: 28})), ("missing storage buffer at binding 5", dict(omit=(STATS,))),
                ("read-only", dict(read_only=(STATS,))), ("also bound as an input", dict(alias=(STATS, LINES))),
                ("push constants", dict(push=struct.pack("<3I", 5, 2, 1))), ("drawsCulled", dict(push=struct.pack("<4I", 5, 2, 1, 2))),
                ("draws", dict(push=struct.pack("<4I", 6, 2, 1, 0))), ("segments", dict(push=struct.pack("<4I", 0xFFFFFFFF, 0xFFFFFFFF, 1, 0))),
                ("dispatch", dict(dispatch=(2, 1, 1)))]
    for match, how in refusals:
        with pytest.raises(PlrError, match=match):
            gpu_draw(backend, [boxes], **how)
    with pytest.raises(PlrError, match="lines"):
        gpu_draw(backend, [lines], push=struct.pack("<4I", 0, 0, 64, 0))
    # and it still runs afterwards
    _compare("after the refusals", gpu_draw(backend, [boxes])[0], dc.reference(70, 37, "boxes"))
