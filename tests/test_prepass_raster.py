"""The "depthPrepassRaster.comp" pass through the C-ABI against tests/prepass_raster_reference.py, in both math modes: every texel of the five images (depth as
its 32 bits, motion, normal, albedo, specular) and the four counters must be bit-identical.

The images are pre-filled with a bit pattern (the pass clears: an untouched texel would keep it) and the scratch buffer with 0xA5 bytes (the pass resets its own
header). The global UBO holds the case's two jitters and nothing else. Cases, the smallest that reach every way the kernels can go wrong:
  unit96x80   96 x 80 = 1.5 x 1.25 tiles (a ragged tile column and row), w = 1: the hand-made triangles of the shadow test's unit96 - quads split along a
              diagonal through pixel centres and with edges on pixel centres, the largest lane-path box (4 x 4) and the smallest wave-path box (5 x 4), triangles
              across the tile boundary, two spans either side of the int32 / int64 limit, a back face and a zero-area triangle
  ties        96 x 80: two coplanar triangles at bit-equal depth over the same pixels, small after large and large after small within a draw, and once in two
              different draws; the later t must win. Two interpenetrating triangles
  fans        96 x 80: the shadow test's fans - the eight edge directions through pixel centres at r = 1.5, r = 20, r = 3 on the corner of four tiles, and as an
              execution of its own r = 150 on the int64 path
  near_clip   96 x 64, camera near 0.1: a ramp quad that reaches behind the camera and more than 10^6 pixels out on both axes where it meets the near plane (its two
              triangles share the clipped diagonal: the keys partition the pixels); a triangle that cuts one corner of the guard volume and one that cuts two
  behind_and_beyond  96 x 64: triangles wholly behind the near plane, wholly beyond the far plane, one straddling far, NaN / inf positions, a NaN matrix, and
              three draws that leave their buffers by one element (index slot, vertex, transform)
  mesh130x70  130 x 70 (odd rows), box + uv_sphere + torus twice under four transforms, two with vertex normals and two without, current and previous jitter, a
              previous camera that differs and one draw whose previous model matrix differs
  far_tiny    64 x 64: 400 triangles half a pixel across at distance 100
  dense64     64 x 64, one tile: the shadow test's 20 011 random small triangles
  draws700    136 x 136: the shadow test's draw-lookup executions
  nothing     72 x 40: no draws; only culled; only rejects. The images are still cleared
  small_frames  1 x 1, 7 x 5, 63 x 65, 65 x 63
The largest image (16384 wide, 3 rows: tile indices 0, 127, 128 and 255) has a test of its own.
"""
import struct

import numpy as np
import pytest

import prepass_raster_cases as pc
import prepass_raster_reference as ref
import test_shadow_raster as tsr
from shadow_raster_cases import quad
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

F32 = np.float32
IMAGES = ("depth", "motion", "normal", "albedo", "specular")


def _unit96x80():
    tris = quad(2.5, 2.5, 10.5, 10.5, 0.3, 0.6) + quad(20.5, 4.5, 30.5, 9.5, 0.4, 0.7) + [tsr.TRI_4X4, tsr.TRI_5X4]
    tris += [[(60.25, 20.5, 0.2), (70.75, 22.0, 0.5), (66.0, 30.25, 0.8)], [(62.0, 50.0, 0.3), (66.0, 50.0, 0.3), (66.0, 53.0, 0.9)]]
    tris += [[(5.0, 66.0, 0.5), (60.0, 66.0, 0.5), (60.0, 94.0, 0.5)], [(10.0, 70.0, 0.25), (50.0, 70.0, 0.25), (50.0, 90.0, 0.25)],
             [(30.0, 68.0, 0.8), (58.0, 68.0, 0.8), (58.0, 96.0, 0.8)]]
    tris += quad(70.5, 60.5, 90.5, 79.5, 0.2, 0.9) + [tsr.TRI_SPAN_32767, tsr.TRI_SPAN_33280]
    tris += [[(10.0, 40.0, 0.5), (20.0, 40.0, 0.5), (20.0, 50.0, 0.5)]]  # keeps its winding: A > 0, a back face
    tris += [[(30.0, 60.0, 0.5), (35.0, 65.0, 0.5), (40.0, 70.0, 0.5)]]  # A == 0
    return [pc.pixel_case([tris], 96, 80, keep_winding=(15,))]


TIE_LARGE = lambda x, y, z: [(x, y, z), (x + 20.0, y, z), (x + 20.0, y + 16.0, z)]
TIE_SMALL = lambda x, y, z: [(x + 8.0, y + 1.0, z), (x + 18.0, y + 1.0, z), (x + 18.0, y + 8.0, z)]


def _ties():
    # draw 0: small after large at (4, 4), large after small at (34, 4), the large half of the third pair; draw 1: its small half; draw 2: interpenetrating
    d0 = [TIE_LARGE(4.0, 4.0, 0.5), TIE_SMALL(4.0, 4.0, 0.5), TIE_SMALL(34.0, 4.0, 0.625), TIE_LARGE(34.0, 4.0, 0.625), TIE_LARGE(64.0, 4.0, 0.375)]
    d1 = [TIE_SMALL(64.0, 4.0, 0.375)]
    d2 = [[(10.0, 40.0, 0.2), (70.0, 40.0, 0.8), (70.0, 76.0, 0.8)], [(10.0, 38.0, 0.8), (72.0, 38.0, 0.2), (72.0, 78.0, 0.2)]]
    return [pc.pixel_case([d0, d1, d2], 96, 80)]


def _fans():
    return [pc.pixel_case([sum((tsr.fan(*f) for f in tsr.FANS), [])], 96, 80), pc.pixel_case([tsr.fan(*tsr.FAN_INT64)], 96, 80)]


NEAR_CAMERA = dict(aspect=96 / 64, near=0.1, far=300.0)
RAMP = np.array([[-4000.0, 1500.0, -5.0], [4000.0, 1500.0, -5.0], [150.0, 1.0, 200.0], [-150.0, 1.0, 200.0]], F32)
ONE_CORNER = [(-0.5, -0.9, 0.5), (-0.5, -0.2, 0.5), (40.0, -0.5, 0.5)]   # NDC under an identity mvp, above the horizon: past x = 32
TWO_CORNERS = [(-0.9, -0.1, 0.3), (40.0, -0.2, 0.3), (-0.8, -40.0, 0.3)]  # past x = 32 and past y = -32


def _near_clip():
    cam = pc.camera(**NEAR_CAMERA)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    transforms = np.stack([ref.main_pass_matrices(vp, vp, [pc.IDENTITY])[0], pc.identity_matrices(1)[0]])
    positions = np.concatenate([RAMP, np.asarray(ONE_CORNER, F32), np.asarray(TWO_CORNERS, F32)])
    indices = [0, 2, 1, 0, 3, 2, 4, 5, 6, 7, 8, 9]
    return [pc.make_case(96, 64, transforms, positions, indices, [[0, 6, 0, 0], [6, 6, 0, 1]])]


def _both_windings(tri):
    return [tri, [tri[0], tri[2], tri[1]]]


def _behind_and_beyond():
    cam = pc.camera(**NEAR_CAMERA)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    nan_model = pc.IDENTITY.copy()
    nan_model[13] = np.nan
    transforms = np.stack([ref.main_pass_matrices(vp, vp, [pc.IDENTITY])[0], ref.main_pass_matrices(vp, vp, [nan_model])[0]])
    flat = lambda z, dx=0.0: [(-1.0 + dx, -0.5, z), (1.0 + dx, -0.5, z), (dx, 0.7, z)]
    tris = _both_windings(flat(8.0)) + _both_windings(flat(-1.0)) + _both_windings(flat(-3.0, 0.5))  # visible; wholly behind the camera
    tris += _both_windings(flat(0.05)) + _both_windings(flat(400.0)) + _both_windings(flat(1e4, 30.0))  # between the camera and near; wholly beyond far
    tris += _both_windings([(-30.0, 5.0, 250.0), (30.0, 5.0, 250.0), (0.0, -60.0, 420.0)])  # straddles far = 300
    bad = [flat(9.0, -2.0), flat(9.0, 2.0), flat(9.0, 0.3)]
    positions = np.asarray(tris + bad, F32).reshape(-1, 3)
    n = 3 * len(tris)
    positions[n, 0], positions[n + 4, 1], positions[n + 8, 2] = np.nan, np.inf, -np.inf
    ordinary = np.asarray(_both_windings(flat(6.0, 1.5)), F32).reshape(-1, 3)  # 6 vertices for the draws below
    base = positions.shape[0]
    positions = np.concatenate([positions, ordinary])
    indices = list(range(base)) + [base + k for k in range(6)] + [0, 1, 2, 3, 4, 6] + [base + k for k in range(6)] + [base + k for k in range(5)]
    # draw 0 everything above; draw 1 the NaN matrix; draw 2 (vertexOffset base): its second triangle's last vertex is the vertex count; draw 3: its transformIndex is
    # the transform count; draw 4, at the end of the index buffer: its second triangle's third slot is the index count
    draws = [[0, base, 0, 0], [base, 6, 0, 1], [base + 6, 6, base, 0], [base + 12, 6, 0, 2], [base + 18, 6, 0, 0]]
    return [pc.make_case(96, 64, transforms, positions, indices, draws)]


MESH_JITTER, MESH_JITTER_PREVIOUS = (0.25 / 130, -0.375 / 70), (-0.125 / 130, 0.3125 / 70)


def _mesh130x70():
    s = pc.mesh_scene()
    from plainrenderer_amd.scene import Camera
    cam = pc.camera(aspect=130 / 70)
    cam_previous = Camera.look((0.02, 0.01, -0.03), (0.0, 0.0, 1.0), world_up=(0.03, -1.0, 0.0), aspect=130 / 70)  # moved and rolled: motion of both signs on both axes
    models_previous = np.array([t for _, t in s["draws"]], F32)
    from shadow_raster_cases import affine
    models_previous[1] = affine((1.5, 0.6, 1.1), -0.45, 0.9, (1.6, -0.3, 9.1))
    return [pc.perspective_case(130, 70, s["meshes"], s["draws"], cam, MESH_JITTER, cam_previous, MESH_JITTER_PREVIOUS, models_previous)]


def _far_tiny():
    # a plane at distance ~100, 20 x 10 cells of 0.5 x 0.5 (a pixel is 0.985 across there), two triangles each, tilted in depth
    cam = pc.camera(aspect=1.0, near=0.1, far=300.0)
    gx, gy = np.meshgrid(np.arange(21) * 0.5 - 5.0, np.arange(11) * 0.5 - 2.5)
    pos = np.stack([gx, gy, 100.0 + 0.3 * gx - 0.2 * gy], -1).reshape(-1, 3).astype(F32)
    idx = []
    for j in range(10):
        for i in range(20):
            a, b, c, d = j * 21 + i, j * 21 + i + 1, (j + 1) * 21 + i + 1, (j + 1) * 21 + i
            idx += [a, b, c, a, c, d]
    mesh = (pos, pc.vertex_normals(pos, idx), np.asarray(idx, np.uint32))
    return [pc.perspective_case(64, 64, [mesh], [(0, pc.IDENTITY)], cam, (0.001, 0.002), cam, (-0.002, 0.001))]


def _dense64():
    return [pc.from_shadow_case(case) for case, _ in tsr._dense64()]


def _draws700():
    return [pc.from_shadow_case(case) for case, _ in tsr._draws700()]


def _nothing():
    empty = pc.make_case(72, 40, np.zeros((0, 48), F32), np.zeros((0, 3), F32), np.zeros(0, np.uint32), np.zeros((0, 6), np.uint32))
    undrawn = [[(10.0, 20.0, 0.5), (20.0, 20.0, 0.5), (20.0, 30.0, 0.5)],  # (keeps its winding) a back face
               [(30.0, 30.0, 0.5), (35.0, 35.0, 0.5), (40.0, 40.0, 0.5)], [(5.0, 5.0, 0.5), (5.0, 5.0, 0.5), (9.0, 9.0, 0.5)],  # zero area
               [(20.625, 20.625, 0.5), (21.375, 20.625, 0.5), (21.375, 21.375, 0.5)],  # between four pixel centres: an empty box inside the image
               [(-30.0, 10.0, 0.5), (-2.0, 10.0, 0.5), (-2.0, 30.0, 0.5)], [(73.0, 10.0, 0.5), (100.0, 10.0, 0.5), (100.0, 30.0, 0.5)],  # left and right of the image
               [(10.0, -40.0, 0.5), (50.0, -40.0, 0.5), (50.0, -1.0, 0.5)], [(10.0, 40.5, 0.5), (50.0, 40.5, 0.5), (50.0, 60.0, 0.5)],  # above and below
               [(10.0, 10.0, 0.0), (30.0, 10.0, 0.0), (30.0, 30.0, -0.5)]]  # on and beyond the far plane: every fragment has zf <= 0
    rejected = pc.pixel_case([[[(5.0, 5.0, 0.5), (60.0, 5.0, 0.5), (60.0, 30.0, 0.5)]] * 4], 72, 40)
    rejected["positions"][0, 0], rejected["positions"][4, 1], rejected["positions"][8, 2] = np.nan, np.inf, -np.inf
    rejected["transforms"] = np.concatenate([rejected["transforms"], rejected["transforms"]])
    rejected["transforms"][1, 16 + 13] = np.nan
    rejected["draws"] = pc.draws6([[0, 9, 0, 0], [9, 3, 0, 1]])
    return [empty, pc.pixel_case([undrawn], 72, 40, keep_winding=(0,)), rejected]


SMALL_FRAMES = ((1, 1), (7, 5), (63, 65), (65, 63))


def _small_frames():
    out = []
    for w, h in SMALL_FRAMES:
        tris = [[(-1.0, -1.0, 0.1), (2.0 * max(w, h) + 2.0, -1.0, 0.9), (-1.0, 2.0 * max(w, h) + 2.0, 0.5)]]
        if w >= 7:
            tris += tsr.SMALL_TRIS
        if w == 65:
            tris += [tsr.TRI_ACROSS_64]
        if h == 65:
            tris += [[(20.0, 61.5, 0.9), (23.5, 66.0, 0.6), (20.0, 66.0, 0.9)]]  # across y = 64
        out.append(pc.pixel_case([tris], w, h))
    return out


CASES = {"unit96x80": _unit96x80, "ties": _ties, "fans": _fans, "near_clip": _near_clip, "behind_and_beyond": _behind_and_beyond, "mesh130x70": _mesh130x70,
         "far_tiny": _far_tiny, "dense64": _dense64, "draws700": _draws700, "nothing": _nothing, "small_frames": _small_frames}
_reference_cache = {}


def reference(name):
    """[(case, reference result)], computed once per case and shared by the modes; callers must not modify it"""
    if name not in _reference_cache:
        _reference_cache[name] = [(case, pc.rasterise(case)) for case in CASES[name]()]
    return _reference_cache[name]


def counters(r):
    return r["submitted"], r["clipped"], r["drawn"], r["rejects"]


def owner(r):
    """the winning triangle number per pixel, -1 without a fragment"""
    return np.where(r["keys"] != 0, (r["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)


NARROW_SPAN = 32768  # device/sun_shadow_raster.h kNarrowSpan: snapped vertices that span less on both axes are evaluated in 32-bit arithmetic


def _pixel_box_and_span(tri, width, height):
    """one triangle alone, as pixel_case makes it (winding reversed): (its pixel box, its snapped spans in sub-pixel units, pixels it keeps)"""
    case = pc.pixel_case([[tri]], width, height)
    clip = np.concatenate([case["positions"], np.ones((3, 1), F32)], axis=1)
    X, Y, _, ok = ref.project(clip, width, height)
    assert ok.all()
    box = (((int(X.max()) - 128) >> 8) - ((int(X.min()) + 127) >> 8) + 1, ((int(Y.max()) - 128) >> 8) - ((int(Y.min()) + 127) >> 8) + 1)
    r = pc.rasterise(case)
    assert r["drawn"] == 1, "it faces front"
    return box, (int(X.max() - X.min()), int(Y.max() - Y.min())), int(r["coverage"].sum())


def _check_unit96x80(runs):
    case, r = runs[0]
    assert counters(r) == (17, 0, 15, 0), "the back face and the zero-area triangle are not drawn, nothing is clipped"
    own = owner(r)
    for tri, box in ((tsr.TRI_4X4, (4, 4)), (tsr.TRI_5X4, (5, 4))):  # the largest box of the lane path and the smallest of the wave path, under this pass' winding and viewport
        (w, h), _, covered = _pixel_box_and_span(tri, 96, 80)
        assert (w, h) == box and covered > 0
    for tri, span in ((tsr.TRI_SPAN_32767, 32767), (tsr.TRI_SPAN_33280, 33280)):  # either side of kNarrowSpan = 32768: the int32 and the int64 path
        _, spans, covered = _pixel_box_and_span(tri, 96, 80)
        assert max(spans) == span and covered > 100
    assert 32767 < NARROW_SPAN <= 33280
    c = r["coverage"]
    assert c[:, 63].any() and c[:, 64].any() and c[64:, :].any() and c[79].any() and c.max() == 3
    assert (own == 13).sum() > 100 and (own == 14).sum() > 100, "both long spans own pixels"
    assert set(np.unique(r["albedo"]).tolist()) == {0, pc.material(0)[0]} and (r["normal"][own >= 0] >> 24 == 255).all()
    assert not r["motion"].any(), "mvpPrevious = mvp and no jitter: no motion"


def _check_ties(runs):
    case, r = runs[0]
    own = owner(r)
    # the small triangle's pixels, from a rasterisation of its own
    for k, (small, large) in enumerate(((1, 0), (2, 3), (5, 4))):
        x = (4.0, 34.0, 64.0)[k]
        z = (0.5, 0.625, 0.375)[k]
        alone = pc.rasterise(pc.pixel_case([[TIE_SMALL(x, 4.0, z)]], 96, 80))["coverage"] > 0
        assert alone.sum() > 20 and (r["coverage"][alone] == 2).all() and (r["depth"][alone] == F32(z)).all(), "two fragments at bit-equal depth"
        assert (own[alone] == max(small, large)).all(), "the later triangle wins the tie"
    assert (r["albedo"][owner(r) == 5] == pc.material(1)[0]).all() and (own == 5).any(), "a tie across two draws: the later draw's material"
    assert (own == 6).sum() > 50 and (own == 7).sum() > 50 and (r["coverage"] == 2).sum() > 300, "interpenetrating: each wins where it is nearer"


def _check_fans(runs):
    centres_x, centres_y = np.arange(96) + 0.5, np.arange(80) + 0.5
    for (case, r), fans in zip(runs, (tsr.FANS, (tsr.FAN_INT64,))):
        assert counters(r) == (8 * len(fans), 0, 8 * len(fans), 0) and r["coverage"].max() == 1
        for cx, cy, radius in fans:
            inside = (np.abs(centres_y - cy) < radius)[:, None] & (np.abs(centres_x - cx) < radius)[None, :]
            assert inside.any() and (r["coverage"][inside] == 1).all(), "every centre strictly inside the outline belongs to exactly one triangle"
            assert len(np.unique(owner(r)[inside])) >= (8 if radius >= 3.0 else 7)
    big = runs[1][1]["coverage"]
    assert big[0].all() and big[-1].all() and big[:, 0].all() and big[:, -1].all(), "clipped at all four image edges"


def _check_near_clip(runs):
    case, r = runs[0]
    assert r["submitted"] == 4 and r["clipped"] == 4 and r["rejects"] == 0 and 4 <= r["drawn"] <= 24
    clip = ref.transform4(case["transforms"][0, 16:32], RAMP)
    assert (clip[:2, 3] < 0).all() and (clip[2:, 3] > 0).all(), "the ramp reaches behind the camera"
    # where its edges meet the near plane w = z (t along the edge from the far vertex), they are more than 10^6 pixels out on both axes
    for far, near in ((2, 1), (3, 0)):
        d_far, d_near = clip[far, 3] - clip[far, 2], clip[near, 3] - clip[near, 2]
        t = d_far / (d_far - d_near)
        v = clip[far] + t * (clip[near] - clip[far])
        assert abs(v[0] / v[3]) * 48 > 1e6 and abs(v[1] / v[3]) * 32 > 1e6
    own = owner(r)
    ramp = (own == 0) | (own == 1)
    assert (own == 0).sum() > 200 and (own == 1).sum() > 200, "both ramp triangles own pixels"
    alone = pc.rasterise(dict(case, draws=case["draws"][:1]))
    assert (alone["coverage"][40:] == 1).all() and alone["coverage"].max() == 1 and not alone["coverage"][:30].any(), \
        "below the horizon every pixel is covered exactly once: the two triangles' keys partition the pixels along the clipped diagonal"
    for number, vertices in ((2, 4), (3, 5)):
        tri = np.concatenate([case["positions"][4 + 3 * (number - 2):7 + 3 * (number - 2)], np.ones((3, 1), F32)], axis=1)
        poly, clipped = ref.clip_triangle(tri)
        assert clipped and len(poly) == vertices and (own == number).sum() > 100, "cuts %d corner(s) of the guard volume" % (vertices - 3)


def _check_behind_and_beyond(runs):
    case, r = runs[0]
    own = owner(r)
    assert r["submitted"] == 14 + 3 + 2 + 2 + 2 + 2 and r["rejects"] == 3 + 2 + 1 + 2 + 1, \
        "three bad positions, the NaN matrix' two triangles, the triangle past the vertices, both triangles of the draw past the transforms, the triangle past the indices"
    visible = set(np.unique(own[own >= 0]).tolist())
    assert len(visible & {0, 1}) == 1 and not visible & set(range(2, 12)), "behind the camera, inside near and beyond far: nothing drawn"
    straddling = visible & {12, 13}
    assert len(straddling) == 1
    t = straddling.pop()
    alone_depth = r["depth"][own == t]
    assert alone_depth.size > 20 and (alone_depth > 0).all() and alone_depth.min() < 1e-4, "the straddling triangle is cut at zf <= 0"
    assert not visible & {19, 20, 21, 22} and len(visible & {23, 24}) == 1 and (r["coverage"][own == 23] >= 2).all(), \
        "the in-buffer neighbours of the rejected triangles are drawn: triangles 19 and 23 are the same triangle, two fragments per pixel, the later wins"
    assert r["clipped"] >= 3


def _check_mesh130x70(runs):
    case, r = runs[0]
    assert r["submitted"] > 2000 and r["rejects"] == 0 and (r["depth"] > 0).sum() > 3000
    assert len(np.unique(r["albedo"])) == 5, "all four draws and the sky"
    m = r["motion"].astype(np.int64)
    for axis in range(2):
        assert (m[..., axis] > 0).any() and (m[..., axis] < 0).any(), "motion of both signs in both channels"
    assert len(np.unique(r["normal"])) > 500
    assert np.any(case["normals"] != 0) and np.any((case["normals"] == 0).all(axis=1)), "meshes with and without vertex normals"
    assert case["width"] % 2 == 0 and (case["width"] * 4) % 16 != 0, "odd rows: 520 bytes"
    assert not np.array_equal(case["transforms"][1, 32:48], case["transforms"][1, 16:32])


def _check_far_tiny(runs):
    case, r = runs[0]
    assert r["submitted"] == 400 and r["rejects"] == 0 and r["clipped"] == 0
    winners = int((r["keys"] != 0).sum())
    w = r["weights"]
    assert winners >= 40 and w.shape == (winners, 3)
    assert w.min() >= -1e-6 and w.max() <= 1 + 1e-6, "fp64 weights of a covered pixel lie inside the triangle: %r .. %r" % (w.min(), w.max())
    clip = ref.transform4(case["transforms"][0, 16:32], case["positions"])
    assert 95 < clip[:, 3].min() and clip[:, 3].max() < 105
    x = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * 64
    assert 0.4 < np.abs(np.diff(x.reshape(11, 21), axis=1)).max() < 0.6, "cells half a pixel across"


def _check_dense64(runs):
    case, r = runs[0]
    assert r["submitted"] == 20011 and 20011 % 64 != 0 and r["coverage"].max() >= 4 and r["drawn"] > 5000


def _check_draws700(runs):
    assert len(runs) == 2 and runs[0][0]["draws"].shape == (700, 6) and runs[0][1]["drawn"] > 1000 and runs[1][1]["drawn"] > 500
    for case, r in runs:
        assert r["submitted"] == int((case["draws"][:, 1] // 3).sum()) and r["rejects"] == 0
        assert len(np.unique(r["albedo"])) > 20, "many draws own pixels: the resolve finds each winner's draw"


def _check_nothing(runs):
    assert [counters(r) for _, r in runs] == [(0, 0, 0, 0), (9, 0, 1, 0), (4, 0, 0, 4)]
    assert not any(r["keys"].any() for _, r in runs)
    assert runs[1][1]["coverage"].sum() == 0, "the triangle on the far plane is set up and keeps no fragment"


def _check_small_frames(runs):
    assert [(case["width"], case["height"]) for case, _ in runs] == list(SMALL_FRAMES)
    for case, r in runs:
        assert (r["coverage"] >= 1).all() and r["rejects"] == 0
    assert runs[3][1]["coverage"][:, 63:65].max() >= 2 and runs[2][1]["coverage"][63:65, :].max() >= 2


CASE_CHECKS = {"unit96x80": _check_unit96x80, "ties": _check_ties, "fans": _check_fans, "near_clip": _check_near_clip, "behind_and_beyond": _check_behind_and_beyond,
               "mesh130x70": _check_mesh130x70, "far_tiny": _check_far_tiny, "dense64": _check_dense64, "draws700": _check_draws700, "nothing": _check_nothing,
               "small_frames": _check_small_frames}


def check_case_is_what_it_is_for(name):
    """on the reference alone: the properties the case is there for"""
    CASE_CHECKS[name](reference(name))


def scratch_bytes(triangles):
    align16 = lambda v: (v + 15) & ~15
    return align16(align16(64 + 8 * triangles) + 24 * triangles) + 576 * triangles


def prefill_pattern(texels, salt):
    return ((np.arange(texels, dtype=np.uint64) * 2654435761 + salt) & 0xFFFFFFFF).astype(np.uint32) | np.uint32(1)


def globals_with_jitter(case):
    g = np.zeros(85, F32)
    g[64:66], g[66:68] = case["jitter_current"], case["jitter_previous"]  # offsets 256 and 264 of the 340-byte global block
    return g.tobytes()


FORMATS = (ImageFormat.Depth32, ImageFormat.RG16_sNorm, ImageFormat.RGBA8, ImageFormat.RGBA8, ImageFormat.RGBA8)


def gpu_prepass(be, case, scratch=None, formats=FORMATS, sizes=None):
    """one execution through the C-ABI with the test's own buffers -> (dict of the five images as uint32 h x w, (submitted, clipped, drawn, rejects))"""
    import passes
    w, h = case["width"], case["height"]
    triangles = int((case["draws"][:, 1] // 3).sum())
    passes.global_binding(be).set(globals_with_jitter(case))
    buffers = []
    for a in (case["transforms"], case["positions"], case["normals"], case["indices"], case["draws"]):
        b = np.ascontiguousarray(a).tobytes() or b"\xa5" * 64  # (the backend refuses a buffer of size 0: an execution without draws binds dummies)
        buffers.append(be.createStorageBuffer(len(b), b))
    nbytes = scratch_bytes(triangles) if scratch is None else scratch
    buffers.append(be.createStorageBuffer(nbytes, b"\xa5" * nbytes))
    images = [be.createImage(image_desc_2d(*(sizes[k] if sizes else (w, h)), fmt), prefill_pattern((sizes[k][0] * sizes[k][1]) if sizes else w * h, 17 * k + 3))
              for k, fmt in enumerate(formats)]
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)], storageBuffers=[StorageBufferResource(b, i != 5, i) for i, b in enumerate(buffers)]),
        struct.pack("<2I", case["draws"].shape[0], triangles), (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = {name: be.downloadImage(img, 0, np.uint32).reshape(h, w).copy() for name, img in zip(IMAGES, images)}
    header = be.downloadStorageBuffer(buffers[5], 20, dtype=np.uint32)
    assert int(header[0]) == int(header[2]), "the cursor counts the drawn sub-triangles"
    return out, (int(header[1]), int(header[4]), int(header[2]), int(header[3]))


def reference_words(r):
    """the reference's five images as the uint32 words the pass stores"""
    motion = r["motion"].astype(np.int16).view(np.uint16).astype(np.uint32)
    return dict(depth=r["depth"].view(np.uint32), motion=motion[..., 0] | (motion[..., 1] << np.uint32(16)), normal=r["normal"], albedo=r["albedo"], specular=r["specular"])


def compare(label, out, counted, r):
    want = reference_words(r)
    differing = {name: int((out[name] != want[name]).sum()) for name in IMAGES}
    print("prepass raster %-28s: texels that differ %r of %d, counters %r (reference %r)" % (label, differing, out["depth"].size, counted, counters(r)))
    for name in IMAGES:
        assert differing[name] == 0, "%s: %d texels differ from the reference, first at %r" % (name, differing[name], tuple(np.argwhere(out[name] != want[name])[0]))
    assert counted == counters(r)


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_are_for(name):
    """not gpu: the input conditions of the GPU test"""
    check_case_is_what_it_is_for(name)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_prepass_raster_is_bit_identical_to_the_reference(backend, name, fast):
    check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for k, (case, r) in enumerate(reference(name)):
            out, counted = gpu_prepass(backend, case)
            general = backend.getGeneralKernelExecutions()
            compare("%s[%d] %s" % (name, k, "fast" if fast else "exact"), out, counted, r)
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


LARGEST_WIDTH, LARGEST_HEIGHT = 16384, 3
LARGEST_TILES = (0, 127, 128, 255)


def _largest():
    tris = [[(64.0 * tx + 10.5, -0.75, 0.3 + 0.002 * tx), (64.0 * tx + 80.5, 0.25, 0.5), (64.0 * tx + 30.25, 3.5, 0.4)] for tx in LARGEST_TILES]
    return pc.pixel_case([tris], LARGEST_WIDTH, LARGEST_HEIGHT)


def check_largest_is_what_it_is_for():
    if "largest" not in _reference_cache:
        case = _largest()
        _reference_cache["largest"] = (case, pc.rasterise(case))
    case, r = _reference_cache["largest"]
    assert counters(r) == (4, 0, 4, 0)
    for tx in LARGEST_TILES:
        assert r["coverage"][:, 64 * tx:64 * tx + 64].any() and (tx == 255 or r["coverage"][:, 64 * tx + 64:64 * tx + 128].any())
    assert r["coverage"][:, LARGEST_WIDTH - 1].any()
    return case, r


def test_largest_image_case_is_what_it_is_for():
    """not gpu: the input conditions of the GPU test below"""
    check_largest_is_what_it_is_for()


@pytest.mark.gpu
def test_gpu_prepass_raster_reaches_the_largest_width(backend):
    """16384 texels wide = 256 tile columns, the most a 4-byte tile rectangle addresses; one math mode (both registrations are one function)"""
    case, r = check_largest_is_what_it_is_for()
    out, counted = gpu_prepass(backend, case)
    compare("largest image %d x %d" % (LARGEST_WIDTH, LARGEST_HEIGHT), out, counted, r)


@pytest.mark.gpu
def test_gpu_launcher_refuses_what_it_cannot_run(backend):
    """fails loudly: a scratch buffer too small for the triangle count (the message states the size formula), a depth image that is not Depth32, images of two sizes"""
    from plainrenderer_amd.backend import PlrError
    case = _unit96x80()[0]
    with pytest.raises(PlrError, match="scratch.*576 triangleCount"):
        gpu_prepass(backend, case, scratch=64)
    with pytest.raises(PlrError, match="Depth32"):
        gpu_prepass(backend, case, formats=(ImageFormat.R16_sFloat,) + FORMATS[1:])
    with pytest.raises(PlrError, match="one size"):
        gpu_prepass(backend, case, sizes=[(96, 80), (96, 80), (96, 80), (96, 64), (96, 80)])
