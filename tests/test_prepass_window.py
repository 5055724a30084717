"""The tile window of the "depthPrepassRaster.comp" pass (the 44-byte pass record: words 0 - 6 as before, words 7 - 10 {windowTileX0, windowTileY0, windowTileX1,
windowTileY1}, half-open, in 64 x 64 tiles) through the C-ABI, in both math modes.

The windowed execution is the unwindowed one restricted to the pixels of the window's tiles: inside the window every image (shadingNormal included where the
case has a normal map) has the bits of the unwindowed GPU execution AND of the numpy reference; outside, every word is still the poison the images were filled
with; the four counters are the unwindowed execution's; a window of the whole grid is the unwindowed execution. Every execution runs twice and gives the same bits.

Frames: 192 x 128 (3 x 2 tiles) and 200 x 150 (4 x 3 tiles, ragged right and bottom). Windows: one interior tile (the frame's second column, second row - on
the 3 x 2 grid that row is the last), one full tile column, the ragged corner tile (the last tile of the last row), the whole grid. Cases: existing ones, taken
from the case modules and stretched over the frame (their geometry is given in NDC, so the same draws cover every tile): the mesh scene without textures, the
stacked cutouts of prepass_alpha_cases, the BC5-normal-mapped quads of prepass_bc_cases, the anisotropic floor of prepass_aniso_cases and the crowd of 250
triangles of prepass_crowd_cases (alpha-tested; 250 records in one tile at its own size, some forty per tile here).

The launcher refuses, by name: an empty window, an inverted one, one that reaches past the tile grid, and a push-constant size that is none of 8, 12, 16, 20, 24,
28 and 44.
"""
import struct

import numpy as np
import pytest

import prepass_alpha_cases as ac
import prepass_aniso_cases as an
import prepass_bc_cases as bc
import prepass_bc_reference as bref
import prepass_crowd_cases as cc
import prepass_normal_cases as nc
import prepass_normal_reference as nref
import prepass_raster_cases as pc
import test_prepass_normal as tpn
import test_prepass_raster as tpr
import test_prepass_texture as tpt
from plainrenderer_amd.backend import PlrError
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

POISON = 0xDEADBEEF  # as depth a negative float, as RGBA8 an alpha of 0xDE: nothing the pass stores
FRAMES = ((192, 128), (200, 150))
TILE = 64


def grid_of(size):
    return (size[0] + TILE - 1) // TILE, (size[1] + TILE - 1) // TILE


def windows_of(size):
    gx, gy = grid_of(size)
    return dict(interior_tile=(1, 1, 2, 2), tile_column=(1, 0, 2, gy), ragged_corner=(gx - 1, gy - 1, gx, gy), whole_grid=(0, 0, gx, gy))


def _plain(size):
    scene = pc.mesh_scene()
    return pc.perspective_case(size[0], size[1], scene["meshes"], scene["draws"], pc.camera(aspect=size[0] / size[1])), None, None, None, 0


def _stretched(run, size):
    case = dict(run[0], width=size[0], height=size[1])
    return (case,) + tuple(run[1:])


def _alpha(size):
    (case, tex, cutoffs), = ac.CASES["stacked"]()
    return _stretched((case, tex, None, cutoffs, 0), size)


def _bc_normal(size):
    case, tex, nm, cutoffs = bc.CASES["normal_bc5"]()[0]
    return _stretched((case, tex, nm, cutoffs, 0), size)


def _aniso(size):
    return _stretched(an.CASES["floor"]()[0], size)


def _crowd(size):
    r = cc.CASES["one_wave"]()
    return _stretched((r["case"], r["tex"], None, r["cutoffs"], 0), size)


RUNS = dict(plain=_plain, alpha_tested=_alpha, bc_normal_mapped=_bc_normal, anisotropic=_aniso, crowd=_crowd)
_cache = {}


def reference(name, size):
    """(run, the reference's five images as words + counters, shadingNormal or None), computed once per (case, frame); callers must not modify it"""
    if (name, size) not in _cache:
        run = RUNS[name](size)
        case, tex, nm, cutoffs, A = run
        sn = None
        if tex is None:
            base = pc.rasterise(case)
        elif A >= 2:
            base, sn, _ = an.compute(case, tex, nm, cutoffs, A, diagnostics=False)
        else:
            decoded = bref.decode_store(tex) if "formats" in tex else tex
            base = nc.base_images(case, decoded, cutoffs)
            if nm is not None:
                sn = nref.shade(case, decoded, nm, base["keys"], base["normal"])
        _cache[(name, size)] = (run, dict(tpr.reference_words(base), shadingNormal=sn), tpr.counters(base))
    return _cache[(name, size)]


def push_of(run, window=None, words=7):
    case, tex, nm, cutoffs, A = run
    draws, triangles = tpn.counts_of(case)
    seven = struct.pack("<7I", draws, triangles, 0 if tex is None else tex["texture_count"], 0 if cutoffs is None else 1, 0 if nm is None else nm["decode"],
                        1 if tex is not None and "formats" in tex else 0, A)
    return seven[:4 * words] if window is None else seven + struct.pack("<4I", *window)


def gpu_run(be, run, push):
    """one execution with the test's own buffers and images full of POISON -> (the images as uint32 h x w, shadingNormal included where bound, counters)"""
    import passes
    case, tex, nm, cutoffs, A = run
    w, h = case["width"], case["height"]
    draws, triangles = tpn.counts_of(case)
    passes.global_binding(be).set(tpr.globals_with_jitter(case) if tex is None else tpt.globals_of(case, tex))
    arrays = {0: case["transforms"], 1: case["positions"], 2: case["normals"], 3: case["indices"], 4: case["draws"], 5: None}
    if tex is not None:
        arrays.update({6: tex["uvs"], 7: tex["materials"], 8: tex["textures"], 9: tex["texels"]})
        if "formats" in tex:
            arrays[14] = np.asarray(tex["formats"], np.uint32)
    if cutoffs is not None:
        arrays[tpn.ALPHA_CUTOFFS] = np.asarray(cutoffs, np.uint32)
    if nm is not None:
        arrays.update({tpn.TANGENTS: nm["tangents"], tpn.BITANGENTS: nm["bitangents"], tpn.NORMAL_MATERIALS: nm["normal_materials"]})
    buffers = {}
    for binding, a in arrays.items():
        b = b"\xa5" * tpr.scratch_bytes(triangles) if a is None else np.ascontiguousarray(a).tobytes()
        buffers[binding] = be.createStorageBuffer(max(len(b), 4), b if b else b"\0" * 4)
    names = tpr.IMAGES + (("shadingNormal",) if nm is not None else ())
    formats = tpr.FORMATS + ((ImageFormat.RGBA8,) if nm is not None else ())
    poison = np.full(w * h, POISON, np.uint32)
    images = [be.createImage(image_desc_2d(w, h, fmt), poison) for fmt in formats]
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, binding != 5, binding) for binding, b in buffers.items()]), push, (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(names, images)}
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


def twice(be, run, push, label):
    first, counted = gpu_run(be, run, push)
    again, counted_again = gpu_run(be, run, push)
    for name in first:
        assert first[name].tobytes() == again[name].tobytes(), "%s: %s differs between two executions" % (label, name)
    assert counted == counted_again, "%s: the counters differ between two executions" % label
    return first, counted


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("size", FRAMES, ids=["%dx%d" % s for s in FRAMES])
@pytest.mark.parametrize("name", list(RUNS))
def test_gpu_a_windowed_execution_is_the_unwindowed_one_inside_and_stores_nothing_outside(backend, name, size, fast):
    run, want, want_counted = reference(name, size)
    assert want_counted[2] > 0, "the case draws something"
    backend.setMathMode(fast)
    try:
        label = "window %s %dx%d %s" % (name, size[0], size[1], "fast" if fast else "exact")
        whole, whole_counted = twice(backend, run, push_of(run), label + ", no window")
        general = backend.getGeneralKernelExecutions()
        if fast:
            assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
        for image, words in whole.items():
            differing = int((words != want[image]).sum())
            print("%s: %s texels of the unwindowed execution that differ from the reference %d" % (label, image, differing))
            assert differing == 0, "%s, no window: %s differs from the reference in %d texels" % (label, image, differing)
        assert whole_counted == want_counted
        for window_name, (x0, y0, x1, y1) in windows_of(size).items():
            out, counted = twice(backend, run, push_of(run, (x0, y0, x1, y1)), "%s, %s" % (label, window_name))
            inside = np.zeros((size[1], size[0]), bool)
            inside[y0 * TILE:y1 * TILE, x0 * TILE:x1 * TILE] = True
            for image, words in out.items():
                wrong_gpu, wrong_ref = int((words[inside] != whole[image][inside]).sum()), int((words[inside] != want[image][inside]).sum())
                touched = int((words[~inside] != POISON).sum())
                print("%s, %s %r: %s inside: %d differ from the unwindowed execution, %d from the reference; outside: %d of %d words are not the poison"
                      % (label, window_name, (x0, y0, x1, y1), image, wrong_gpu, wrong_ref, touched, int((~inside).sum())))
                assert wrong_gpu == 0 and wrong_ref == 0, "%s, %s: %s differs inside the window" % (label, window_name, image)
                assert touched == 0, "%s, %s: %s was stored to outside the window, first at %r" % (label, window_name, image, tuple(np.argwhere((words != POISON) & ~inside)[0]))
            assert counted == whole_counted, "%s, %s: the counters %r depend on the window (unwindowed %r)" % (label, window_name, counted, whole_counted)
            if window_name == "whole_grid":
                for image, words in out.items():
                    assert words.tobytes() == whole[image].tobytes(), "%s: the whole-grid window's %s differs from the unwindowed execution's" % (label, image)
    finally:
        backend.setMathMode(False)


def _refused(backend, push, match):
    run, _, _ = reference("plain", FRAMES[1])
    with pytest.raises(PlrError, match=match):
        gpu_run(backend, run, push)


@pytest.mark.gpu
def test_gpu_an_empty_window_is_refused(backend):
    run, _, _ = reference("plain", FRAMES[1])
    _refused(backend, push_of(run, (1, 1, 1, 2)), "tile window \\{1, 1, 1, 2\\} is empty or inverted")
    _refused(backend, push_of(run, (0, 2, 4, 2)), "tile window \\{0, 2, 4, 2\\} is empty or inverted")


@pytest.mark.gpu
def test_gpu_an_inverted_window_is_refused(backend):
    run, _, _ = reference("plain", FRAMES[1])
    _refused(backend, push_of(run, (3, 0, 1, 2)), "tile window \\{3, 0, 1, 2\\} is empty or inverted")
    _refused(backend, push_of(run, (0, 2, 1, 1)), "tile window \\{0, 2, 1, 1\\} is empty or inverted")


@pytest.mark.gpu
def test_gpu_a_window_past_the_tile_grid_is_refused(backend):
    """200 x 150 is 4 x 3 tiles"""
    run, _, _ = reference("plain", FRAMES[1])
    _refused(backend, push_of(run, (0, 0, 5, 3)), "reaches past the tile grid of the bound images, 4 x 3 tiles")
    _refused(backend, push_of(run, (3, 2, 4, 4)), "reaches past the tile grid of the bound images, 4 x 3 tiles")
    _refused(backend, push_of(run, (0, 0, 0xFFFFFFFF, 1)), "reaches past the tile grid")


@pytest.mark.gpu
def test_gpu_a_push_constant_size_that_is_not_defined_is_refused(backend):
    """between the defined sizes, a window cut short, and past the end; a size that is no multiple of 4"""
    run, _, _ = reference("plain", FRAMES[1])
    full = push_of(run, (0, 0, 4, 3))
    for size in (10, 32, 36, 40, 42, 48):
        _refused(backend, (full + bytes(8))[:size], "push constants are %d bytes, the record has 8, 12, 16, 20, 24, 28 or 44" % size)
