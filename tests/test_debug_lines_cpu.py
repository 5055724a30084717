"""tests/debug_lines_reference.py - the line contract of "debugGeometry.comp" - against the contract's own properties, without a GPU; and that the library exports
the calls. What the reference is held to here is what tests/test_debug_lines.py then holds the kernels to through it."""
import ctypes

import numpy as np
import pytest

import debug_lines_cases as dc
import debug_lines_reference as ref

F32 = np.float32
W, H = 256, 144


def _sub(v):
    return int(round(v * 256))


def _fragments(x0, y0, x1, y1, z0=0.5, z1=0.75, w=W, h=H):
    """fragments of a segment given in pixels (on the sub-pixel grid)"""
    return ref.cover(_sub(x0), _sub(y0), F32(z0), _sub(x1), _sub(y1), F32(z1), w, h)


SEGMENTS = [(3.25, 1.5, 40.0, 9.0), (3.25, 9.0, 40.0, 1.5), (7.0, 2.0, 9.5, 60.0), (9.5, 2.0, 7.0, 60.0), (10.0, 10.0, 30.0, 30.0), (10.0, 30.0, 30.0, 10.0),
            (-20.5, 3.0, 50.0, -4.0), (0.3, 0.2, 255.9, 143.7), (100.0, 5.5, 101.0, 5.5), (5.0, 20.0, 5.2, 90.0)]


@pytest.mark.parametrize("seg", SEGMENTS)
def test_reversing_the_ends_gives_identical_pixels_and_depth_bits(seg):
    x0, y0, x1, y1 = seg
    a, b = _fragments(x0, y0, x1, y1, 0.3, 0.9), _fragments(x1, y1, x0, y0, 0.9, 0.3)
    assert a["drawn"] and a["xs"].size > 0
    assert np.array_equal(a["xs"], b["xs"]) and np.array_equal(a["ys"], b["ys"])
    assert np.array_equal(a["zf"].view(np.uint32), b["zf"].view(np.uint32))


@pytest.mark.parametrize("seg", SEGMENTS)
def test_one_fragment_per_major_step_and_the_pixels_are_8_connected(seg):
    f = _fragments(*seg)
    major, minor = (f["xs"], f["ys"]) if f["x_major"] else (f["ys"], f["xs"])
    assert np.array_equal(np.diff(major), np.ones(major.size - 1, np.int64)), "one pixel per major step, ascending"
    assert np.abs(np.diff(minor)).max(initial=0) <= 1, "8-connected"
    assert major.size <= f["steps"]


def test_a_shared_polyline_vertex_is_covered_once():
    """two segments that continue each other along one major axis share no pixel, whether the vertex lies on a pixel centre - where the half-open rule decides -
    or off it, in either direction of travel; and together they cover every major step between their outer ends"""
    for vx, vy in ((20.5, 11.5), (20.25, 11.75), (20.0, 11.0)):
        for (ax, ay), (bx, by), x_major in (((3.0, 8.0), (40.0, 15.0), True), ((40.0, 15.0), (3.0, 8.0), True), ((18.0, 2.0), (23.0, 30.0), False), ((23.0, 30.0), (18.0, 2.0), False)):
            first, second = _fragments(ax, ay, vx, vy), _fragments(vx, vy, bx, by)
            assert first["x_major"] == second["x_major"] == x_major
            pixels = list(zip(first["xs"].tolist(), first["ys"].tolist())) + list(zip(second["xs"].tolist(), second["ys"].tolist()))
            assert len(set(pixels)) == len(pixels), "vertex %r of %r - %r: a pixel is covered twice" % ((vx, vy), (ax, ay), (bx, by))
            major = sorted(p[0] if x_major else p[1] for p in pixels)
            assert major == list(range(major[0], major[-1] + 1)), "and no major step is left out"


def test_a_segment_that_crosses_no_pixel_centre_along_its_major_axis_covers_nothing():
    for seg in ((10.6, 5.0, 11.4, 5.3), (10.5 + 1 / 256, 5.0, 11.5, 5.3), (7.2, 3.55, 7.3, 4.45), (12.5, 7.5, 12.5, 7.5)):
        f = _fragments(*seg)
        assert not f["drawn"] and f["xs"].size == 0, seg
    # the half-open rule: a centre at U0 is covered, one at U1 is not
    assert _fragments(10.5, 5.0, 11.5, 5.0)["xs"].tolist() == [10]
    assert _fragments(11.5, 5.0, 10.5, 5.0)["xs"].tolist() == [10]


def test_equal_extents_are_x_major():
    for seg in ((10.0, 10.0, 30.0, 30.0), (10.0, 30.0, 30.0, 10.0), (30.0, 30.0, 10.0, 10.0)):
        f = _fragments(*seg)
        assert f["x_major"] and f["steps"] == 20 and np.array_equal(np.diff(f["xs"]), np.ones(19, np.int64))
    assert not _fragments(10.0, 10.0, 30.0, 30.0 + 1 / 256)["x_major"]


def test_negative_slopes_and_a_minor_coordinate_below_zero_use_the_floor_division():
    # V falls from 1.25 to -0.75 over four columns: at the centres 0.5 .. 3.5 it is 1.0, 0.5, 0.0, -0.5: j = 1, 0, 0, -1; truncation would keep the last at 0
    f = _fragments(0.0, 1.25, 4.0, -0.75)
    assert f["steps"] == 4 and f["xs"].tolist() == [0, 1, 2] and f["ys"].tolist() == [1, 0, 0]
    # wholly above the image but within a pixel of it: -0.25 truncates to row 0, floors to row -1
    f = _fragments(2.0, -0.25, 9.0, -0.25)
    assert f["drawn"] and f["xs"].size == 0
    # against exact rational arithmetic on a steep and a shallow negative slope
    from fractions import Fraction
    for x0, y0, x1, y1 in ((1.3, 40.7, 200.9, -3.2), (-7.6, 2.1, 3.3, 120.4)):
        f = _fragments(x0, y0, x1, y1)
        X0, Y0, X1, Y1 = _sub(x0), _sub(y0), _sub(x1), _sub(y1)
        for x, y in zip(f["xs"].tolist(), f["ys"].tolist()):
            if f["x_major"]:
                exact = Fraction(Y0) + Fraction(256 * x + 128 - X0) * Fraction(Y1 - Y0, X1 - X0)
                assert y == int(np.floor(exact / 256))
            else:
                exact = Fraction(X0) + Fraction(256 * y + 128 - Y0) * Fraction(X1 - X0, Y1 - Y0)
                assert x == int(np.floor(exact / 256))


def test_depth_is_interpolated_in_fp64_and_rounded_once():
    f = _fragments(3.25, 1.5, 40.0, 9.0, 0.3, 0.9)
    U0, U1 = _sub(3.25), _sub(40.0)
    t = (256 * f["xs"] + 128 - U0).astype(np.float64) / float(U1 - U0)
    want = (np.float64(F32(0.3)) + t * (np.float64(F32(0.9)) - np.float64(F32(0.3)))).astype(F32)
    assert np.array_equal(f["zf"].view(np.uint32), want.view(np.uint32)) and (np.diff(f["zf"]) > 0).all()


def test_the_clip_cuts_rejects_and_keeps():
    w, h = 70, 37
    inside = dc.px(w, h, 5.0, 5.0, 0.5, 20.0, 8.0, 0.9)
    r = ref.clip_and_snap(inside[0:3], inside[3:6], dc.IDENTITY, w, h)
    assert not r["rejected"] and not r["clipped"] and (r["X0"], r["Y0"], r["X1"], r["Y1"]) == (5 * 256, 5 * 256, 20 * 256, 8 * 256)
    # through the near plane (z = 1 under the identity): cut there, half way along
    through = dc.px(w, h, 5.0, 5.0, 0.5, 20.0, 8.0, 1.5)
    r = ref.clip_and_snap(through[0:3], through[3:6], dc.IDENTITY, w, h)
    assert not r["rejected"] and r["clipped"] and abs(r["X1"] - int(12.5 * 256)) <= 1 and abs(float(r["z1"]) - 1.0) < 1e-6 and r["X0"] == 5 * 256
    # the same segment given the other way round is cut at the same point
    back = ref.clip_and_snap(through[3:6], through[0:3], dc.IDENTITY, w, h)
    assert (back["X0"], back["Y0"]) == (r["X1"], r["Y1"]) and np.float32(back["z0"]).view(np.uint32) == np.float32(r["z1"]).view(np.uint32)
    # wholly in front of the near plane under the identity; wholly behind the camera under a perspective view
    beyond = dc.px(w, h, 5.0, 5.0, 1.5, 20.0, 8.0, 1.2)
    assert ref.clip_and_snap(beyond[0:3], beyond[3:6], dc.IDENTITY, w, h)["rejected"]
    vp = dc.perspective_view(w, h)
    lines = dc.perspective_lines()
    results = [ref.clip_and_snap(l[0:3], l[3:6], vp, w, h) for l in lines]
    assert [r["rejected"] for r in results] == [False, False, True, False, False, False]
    assert [r["clipped"] for r in results] == [False, True, False, True, False, True]
    # an end beyond the guard band (|x| > 32 w) is cut on the guard plane: 32 half-widths from the centre
    far = dc.px(w, h, 10.0, 10.0, 0.95, 40.0 * w, 12.0, 0.95)
    r = ref.clip_and_snap(far[0:3], far[3:6], dc.IDENTITY, w, h)
    assert not r["rejected"] and r["clipped"] and abs(r["X1"] - int(16.5 * w * 256)) <= 256
    # a NaN coordinate is outside every plane
    assert ref.clip_and_snap((np.nan, 0.0, 0.5), (np.nan, 0.1, 0.5), dc.IDENTITY, w, h)["rejected"]


def test_box_edge_order_and_world_box():
    lo, hi = np.array([0, 0, 0], F32), np.array([1, 2, 4], F32)
    edges = ref.box_edges(lo, hi)
    assert len(edges) == 12
    corner = lambda k: [hi[r] if (k >> r) & 1 else lo[r] for r in range(3)]
    want = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
    for (a, b), (ka, kb) in zip(edges, want):
        assert a.tolist() == corner(ka) and b.tolist() == corner(kb)
    # the world box is axis-aligned: a rotation by 45 degrees about z widens a unit square's box to its diagonal
    s = np.sqrt(0.5)
    model = np.array([[s, -s, 0, 3], [s, s, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).T.astype(F32).reshape(16)
    wlo, whi = ref.world_box((-1, -1, -1), (1, 1, 1), model)
    assert np.allclose(wlo, (3 - 2 * s, -2 * s, -1), atol=1e-6) and np.allclose(whi, (3 + 2 * s, 2 * s, 1), atol=1e-6)
    slots, segs = ref.segments(draws=np.array([[0, 36, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 36, 0, 9, 0, 0]], np.uint32), bounds=np.tile(np.array([-1, -1, -1, 1, 1, 1], F32), (3, 1)),
                               transforms=np.concatenate([model, np.zeros(32, F32)])[None, :], sdf_boxes=np.arange(8, dtype=F32)[None, :], lines=np.ones((2, 9), F32), draws_culled=True)
    assert slots == 3 * 12 + 12 + 2
    assert [s for s, _, _, _ in segs] == list(range(12)) + list(range(36, 48)) + [48, 49], "a culled draw and one whose transform is out of range submit nothing and keep their numbers"
    assert segs[12][3] == ref.SDF_BOX_RGB and segs[0][3] == ref.DRAW_BOX_RGB and segs[12][1].tolist() == [0, 1, 2] and segs[12][2].tolist() == [4, 1, 2]


def test_the_cases_are_what_their_names_say():
    w, h = 256, 144
    ref_of = lambda name: dc.reference(w, h, name)
    steps = [s for s in ref_of("steps")[3]["segments"]]
    assert [s["steps"] for s in steps] == [n for n in dc.STEP_COUNTS for _ in range(2)] and [s["x_major"] for s in steps] == [True, False] * 6
    color, depth, stats, details = ref_of("depth test")
    c0, d0 = dc.images(w, h)
    assert (details["winner"][dc.NEAR_ROW] == -1).all(), "hidden behind the nearer band"
    assert (details["winner"][dc.EQUAL_ROW, 2:60] == 1).all() and np.array_equal(depth[dc.EQUAL_ROW], d0[dc.EQUAL_ROW]), "bit-equal depth passes GreaterEqual"
    row = details["winner"][dc.EQUAL_ROW + 1]
    assert (row[2:25] == -1).all() and (row[36:60] == 2).all(), "the sloped line appears where it comes in front of the band"
    assert ((details["winner"] == 3) & (d0 == 0)).any() and not ((details["winner"] == 3) & (d0 > 0.01)).any(), "a far line shows over the sky only"
    _, _, _, crossing = ref_of("crossing at equal depth")
    both = crossing["winner"][5, 28:32]
    assert (both == 1).any(), "where two lines cross at bit-equal depth the later one wins"
    for name in ("300 through one pixel, distinct depths", "300 through one pixel, equal depths"):
        _, _, stats, d = ref_of(name)
        assert stats["drawn"] == 300 and stats["fragments"] > 300 * 8
        covering = sum(1 for s in d["segments"] if ((s["xs"] == 33) & (s["ys"] == 17)).any())
        assert covering == 300
    assert ref_of("300 through one pixel, equal depths")[3]["winner"][17, 33] == 299
    off = ref_of("off each side")
    assert off[2]["rejected"] == 1 and off[2]["clipped"] == 2 and off[2]["drawn"] == 8, off[2]
    assert off[2]["submitted"] == 11
    zero = ref_of("zero length")
    assert zero[2] == dict(submitted=2, clipped=0, rejected=0, drawn=0, fragments=0, pixels_written=0)
    plain, odd, culled = ref_of("boxes")[2], ref_of("boxes, odd inputs")[2], ref_of("boxes, culled copy")[2]
    assert plain["submitted"] == 5 * 12 + 2 * 12 + 1 and culled["submitted"] == plain["submitted"] - 12
    assert odd["submitted"] == plain["submitted"] - 12 and odd["rejected"] >= 12, "the out-of-range draw submits nothing, the NaN box is rejected edge by edge"
    for n in dc.SEGMENT_COUNTS:
        assert ref_of("%d segments" % n)[2]["submitted"] == n
    # every case leaves the pixels without a winner alone
    for name, c in dc.named_cases(w, h):
        color, depth, stats, d = ref_of(name)
        lost = d["winner"] < 0
        assert np.array_equal(color[lost], c["color"][lost]) and np.array_equal(depth[lost].view(np.uint32), c["depth"][lost].view(np.uint32))
        assert stats["pixels_written"] == int((~lost).sum()) <= stats["fragments"]


def test_the_library_exports_the_calls():
    from plainrenderer_amd import backend
    lib = ctypes.CDLL(backend.LIB_PATH)
    for name in ("plrf_set_debug_geometry", "plrf_set_debug_lines", "plrf_get_debug_geometry_stats"):
        assert hasattr(lib, name), name
    from plainrenderer_amd import frame
    assert (frame.DEBUG_DRAW_BOXES, frame.DEBUG_SDF_BOXES, frame.DEBUG_LINES) == (1, 2, 4)
    assert ctypes.sizeof(frame.PlrfDebugGeometryStats) == 32
    for name in ("set_debug_geometry", "set_debug_lines", "debug_geometry_stats"):
        assert hasattr(frame.FramePipeline, name)
