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
The contract clause by clause, where the cases above do not reach:
  octagon     96 x 64: a triangle that crosses the near plane and all four guard planes, clipped to 8 vertices, in its three front-facing vertex orders at three
              depths that each win somewhere, as it is and translated twice so that every fan index 0 .. 5 is drawn; and as an execution of its own a 6- and
              a 7-vertex polygon under the near_clip camera
  sub_rejects 96 x 64: counted rejects of sub-triangles - a vertex (0, 0, 0, 0), inside all five planes and failing w > 0; a vertex whose z / w overflows to
              -inf; a clipped triangle of which one sub-triangle is a reject and the other is drawn, in both orders; a visible triangle behind them
  motion_edges  72 x 40, non-zero jitters: motion saturated at +-32767, a previous w sum of -1 and of 0, a NaN previous x, and one code below +1
  normal_edges  72 x 40: a singular mat3(model) (128, 128, 128), vertex normals that interpolate through zero, inf / NaN / 1e30 normals, normals that are not
              unit length under scale and shear, and the face normal under the same model
  denormal_depth  64 x 64: constant depths 1e-41, the least denormal and the least normal, ties among them, and a ramp that the far rule cuts inside the
              denormal range
  lane_int64  96 x 80: two thin triangles of span 35008 whose boxes are 64 x 4 in one tile and 3 x 4 in the next: 64-bit edge functions on the lane path
  crowded_large  64 x 64, one tile: 200 triangles of about 10 x 10 pixels and 50 small ones in one 256-rectangle step - more than 64 wave-path hits
The largest images (16384 wide and 3 rows, 3 wide and 16384 rows: tile indices 0, 127, 128 and 255 on either axis) have tests of their own.
"""
import struct
import time

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



def _grouped_case(width, height, transforms, groups, normals=None, **jitters):
    """one draw per group (transformIndex, triangles of three model-space positions), vertices in submission order"""
    positions = np.asarray([v for _, tris in groups for tri in tris for v in tri], F32).reshape(-1, 3)
    draws, first = [], 0
    for transform_index, tris in groups:
        draws.append([first, 3 * len(tris), 0, transform_index])
        first += 3 * len(tris)
    return pc.make_case(width, height, transforms, positions, np.arange(positions.shape[0]), draws, normals, **jitters)


def _matrices(mvp, model=pc.IDENTITY, previous=None):
    return np.concatenate([np.asarray(model, F32).reshape(16), np.asarray(mvp, F32).reshape(16), np.asarray(mvp if previous is None else previous, F32).reshape(16)])


# clip = (x, y, 0.05, z): w is the model-space z and the clip z a constant, so the near plane w >= z is the model-space plane z = 0.05. In (x, y, w) the triangle
# lies in the plane x + y - 50 (w - 1) = 45; cut at the near plane it is the NDC diamond (45, 0), (0, 45), (-50, 0), (0, -50), which the guard square |x|, |y| <= 32
# cuts at all four corners: an octagon, two vertices on every side. On screen w = 5 / (50 - (u + v)), about 0.1.
OCTAGON_S = 45.0 / 42.5
OCTAGON = ((45.0, 0.0, 1.0), (0.0, 45.0, 1.0), (-2.5 * OCTAGON_S, -2.5 * OCTAGON_S, 1.0 - 0.95 * OCTAGON_S))
OCTAGON_FRONT = ((0, 2, 1), (1, 0, 2), (2, 1, 0))  # the three vertex orders that face front
# the shape as it is, and translated in NDC (x + dx w, y + dy w) by less than the 13 that keep all four corners cut (half a unit more or less on either axis still
# gives 8 vertices): the fan starts at another place relative to the screen, and the boxes of sub-triangles 0, 1 and 5 reach it
OCTAGON_OFFSETS = ((0.0, 0.0), (-8.0, 6.0), (8.0, 10.0))
OCTAGON_COUNTERS = ((3, 3, 9, 0), (3, 3, 11, 0), (3, 3, 11, 0))
OCTAGON_FANS = (((2, 3, 4), (2, 3, 4), (2, 3, 4)), ((0, 1, 2, 3, 4), (2, 3, 4), (2, 3, 4)), ((1, 2, 3, 4), (2, 3, 4), (2, 3, 4, 5)))
# found by a random search under the near_clip camera: rng = np.random.default_rng(0x4F435447), per trial np.round(rng.uniform((-40, -40, -2), (40, 40, 12), (3, 3)), 3),
# the first trial whose polygon has 6 (trial 282) and 7 (trial 616) vertices, at least 2 drawn sub-triangles, no reject and more than 300 pixels
HEXAGON = ((9.489, -4.831, -1.397), (-20.575, 27.834, 7.088), (-25.875, -8.528, 1.056))
HEPTAGON = ((23.335, -36.792, 1.611), (-11.845, 25.58, -1.096), (-21.067, -35.488, 6.209))


def octagon_mvp(k, dx=0.0, dy=0.0):
    """clip = (x + dx z, y + dy z, a z + b, z): depth a + b / w, for k = 0 exactly (x, y, 0.05, z). The three lines in q = 1 / w have slopes b = 0.05, 0.0495 and
    0.049 (the near plane w >= a w + b hardly moves); lines 0 and 2 cross at the q of the screen centre, q0 = (50 + dx + dy) / 5, and line 1 lies 0.00005 above
    that crossing: it is the nearest where |q - q0| < 0.1, on a screen where q varies by +- 0.4"""
    q0 = (50.0 + dx + dy) / 5.0
    a, b = ((0.0, 0.05), (0.0005 * q0 + 0.00005, 0.0495), (0.001 * q0, 0.049))[k]
    return pc.glm([[1, 0, dx, 0], [0, 1, dy, 0], [0, 0, a, b], [0, 0, 1, 0]])


def _octagon():
    out = []
    for dx, dy in OCTAGON_OFFSETS:
        transforms = np.stack([_matrices(octagon_mvp(k, dx, dy)) for k in range(3)])
        out.append(_grouped_case(96, 64, transforms, [(k, [[OCTAGON[i] for i in order]]) for k, order in enumerate(OCTAGON_FRONT)]))
    cam = pc.camera(**NEAR_CAMERA)
    vp = np.asarray(cam.view_projection(), F32).reshape(16)
    out.append(_grouped_case(96, 64, ref.main_pass_matrices(vp, vp, [pc.IDENTITY]), [(0, [HEXAGON, HEPTAGON])]))
    return out


W_ZERO = ((0.0, 0.0, 0.0), (0.5, 0.0, 1.0), (0.0, 0.5, 1.0))          # under clip = (x, y, 0.05 z, z) its first vertex is (0, 0, 0, 0)
Z_OVERFLOW = ((0.0, 0.0, 1e-30), (0.5, 0.0, 1.0), (0.0, 0.5, 1.0))    # under clip = (x, y, 1e30 z - 1e30, z) its first vertex has z = -1e30, w = 1e-30
# under clip = (x, y, -4e8, z): the middle vertex, at the apex of the clip volume (NDC (-0.9, -0.9)) with z / w = -4e38, overflows. The third vertex is outside
# 32 w - x; the vertex the clipper puts on the edge from the middle one towards it has w = 3.6e-29 and z / w = -1.1e37, finite. The polygon is (v0, v1, that vertex,
# the one on v2 -> v0): sub-triangle 0 is a reject and sub-triangle 1 is not; in the reversed order the polygon ends with v1 and sub-triangle 1 is the reject
Z_OVERFLOW_PARTLY = ((-0.9, 0.5, 1.0), (-0.9e-30, -0.9e-30, 1e-30), (40.0, -0.5, 1.0))
VISIBLE_BEHIND = ((-0.9, -0.8, 2.0), (0.9, -0.8, 2.0), (0.0, 0.9, 2.0))


def _rotations(tri):
    return [[tri[(k + i) % 3] for i in range(3)] for k in range(3)]


def _sub_rejects():
    flat = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.05, 0], [0, 0, 1, 0]])
    steep = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1e30, -1e30], [0, 0, 1, 0]])
    deep = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, -4e8], [0, 0, 1, 0]])
    transforms = np.stack([_matrices(flat), _matrices(steep), _matrices(deep)])
    visible = _both_windings(VISIBLE_BEHIND)
    return [_grouped_case(96, 64, transforms, [(0, _both_windings(W_ZERO) + visible), (1, _both_windings(Z_OVERFLOW)), (2, _rotations(Z_OVERFLOW_PARTLY) + _rotations(Z_OVERFLOW_PARTLY[::-1])), (0, visible)])]


def _with_draw_transforms(case, transforms):
    """the case with one transform per draw"""
    case = dict(case, transforms=np.asarray(transforms, F32).reshape(-1, 48), draws=case["draws"].copy())
    assert case["transforms"].shape[0] == case["draws"].shape[0]
    case["draws"][:, 3] = np.arange(case["draws"].shape[0])
    return case


def _columns(count, width, height, z=0.5):
    """`count` triangles side by side, one per draw: each 12 pixels wide and height - 4 tall"""
    step = width // count
    return [[[(1.0 + step * k, 2.0, z), (13.0 + step * k, 2.0, z), (13.0 + step * k, height - 2.0, z)]] for k in range(count)]


MOTION_JITTER, MOTION_JITTER_PREVIOUS = (0.004, -0.003), (-0.002, -0.003)  # y: the same in both frames, so the draw with a NaN x stores 0 in y as well
MOTION_BELOW_ONE = 1.0 - 0.7 / 32767.0  # m * 32767 = 32766.3: code 32766
MOTION_BEYOND_ONE = 1.0 + 0.7 / 32767.0


def _translated(tx, ty):
    m = pc.IDENTITY.copy()
    m[12], m[13] = tx, ty
    return m


def _motion_edges():
    negated, zero_w, nan_x = pc.IDENTITY.copy(), pc.IDENTITY.copy(), pc.IDENTITY.copy()
    negated[15], zero_w[15], nan_x[12] = -1.0, 0.0, np.nan
    # m = (translation + previous jitter - current jitter) / 2
    jx, jy = MOTION_JITTER_PREVIOUS[0] - MOTION_JITTER[0], MOTION_JITTER_PREVIOUS[1] - MOTION_JITTER[1]
    edge = _translated(2.0 * MOTION_BELOW_ONE - jx, -2.0 * MOTION_BEYOND_ONE - jy)
    previous = [_translated(3.0, -3.0), negated, zero_w, nan_x, edge]
    case = _with_draw_transforms(pc.pixel_case(_columns(5, 72, 40), 72, 40), [_matrices(pc.IDENTITY, previous=p) for p in previous])
    case["jitter_current"], case["jitter_previous"] = tuple(float(F32(v)) for v in MOTION_JITTER), tuple(float(F32(v)) for v in MOTION_JITTER_PREVIOUS)
    return [case]


SHEAR_MODEL = pc.glm([[1.5, 0.4, 0.25, 0.0], [0.0, 0.7, 0.3, 0.0], [0.2, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def _normal_edges():
    singular = pc.IDENTITY.copy()
    singular[[0, 5, 10]] = 0.0
    models = [singular, pc.IDENTITY, pc.IDENTITY, SHEAR_MODEL, SHEAR_MODEL]
    columns = _columns(5, 72, 40)
    # draw 1 from y = 2.5 to 32.5, NDC -0.875 and 0.625: the weight of its lower vertex is 1/2 on the pixel centres of row 17, NDC -0.125, all three exact in binary
    columns[1] = [[(15.0, 2.5, 0.5), (27.0, 2.5, 0.5), (27.0, 32.5, 0.5)]]
    case = _with_draw_transforms(pc.pixel_case(columns, 72, 40), [_matrices(pc.IDENTITY, model=m) for m in models])
    normals = np.zeros((15, 3), F32)
    normals[0:3] = (0.0, 0.0, 1.0)                                              # draw 0: any normal under the singular model
    normals[3:6] = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)]         # draw 1: interpolates through zero
    normals[6:9] = [(np.inf, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, 1e30)]   # draw 2: only the third normalises to a non-zero vector
    normals[9:12] = [(0.3, 0.4, 2.0), (1.0, 2.0, -0.5), (-3.0, 0.25, 0.75)]     # draw 3: not unit length, under scale and shear
    case["normals"] = normals                                                   # draw 4: no stored normals, the face normal under the same model
    return [case]


DENORMAL_SMALL, DENORMAL_LEAST, NORMAL_LEAST = 1e-41, 1.4e-45, 1.1754944e-38
DENORMAL_TWO = 2.8e-45  # two units of the least denormal


def _denormal_depth():
    flat = lambda x, y, z, size=28.0: [(x, y, z), (x + size, y, z), (x + size, y + size, z)]
    tris = [flat(2.0, 2.0, DENORMAL_SMALL), flat(34.0, 2.0, DENORMAL_LEAST), flat(2.0, 34.0, NORMAL_LEAST),
            [(34.0, 34.0, DENORMAL_SMALL), (62.0, 34.0, -DENORMAL_SMALL), (62.0, 62.0, -DENORMAL_SMALL)],  # zf <= 0 from x = 48 on
            flat(12.0, 4.0, DENORMAL_LEAST, 12.0), flat(44.0, 4.0, DENORMAL_TWO, 12.0)]  # over the first: it loses; over the second: it wins by one unit
    return [pc.pixel_case([tris], 64, 64)]


# thin, span 136.75 pixels = 35008 sub-pixel units: 64 x 4 pixels in the first tile and 3 x 4 in the next one. The second is its transpose across y = 64
LANE_INT64_ROW = [(-70.0, 10.0, 0.3), (66.75, 10.0, 0.6), (66.75, 13.5, 0.7)]
LANE_INT64_COLUMN = [(10.0, -70.0, 0.4), (13.5, 66.75, 0.8), (10.0, 66.75, 0.5)]


def _lane_int64():
    return [pc.pixel_case([[LANE_INT64_ROW, LANE_INT64_COLUMN]], 96, 80)]


CROWDED_LARGE, CROWDED_SMALL = 200, 50


def _crowded_large():
    """250 consecutive triangles of one draw in one tile: one block of the set-up kernel, so the records are in submission order, and one 256-rectangle step of
    the tile kernel's first wave. Right triangles with legs of 9 to 12 pixels (the wave path) and, at 50 random places among them, of 2 to 3.5 pixels (the lane
    path); corners on the quarter-pixel grid, a random depth per vertex"""
    rng = np.random.default_rng(0x43524F57)
    n = CROWDED_LARGE + CROWDED_SMALL
    small = np.zeros(n, bool)
    small[rng.permutation(n)[:CROWDED_SMALL]] = True
    tris = []
    for k in range(n):
        leg = np.rint(rng.uniform((2.0, 2.0), (3.5, 3.5)) * 4) / 4 if small[k] else np.rint(rng.uniform((9.0, 9.0), (12.0, 12.0)) * 4) / 4
        x, y = np.rint(rng.uniform((-2.0, -2.0), (54.0, 54.0)) * 4) / 4
        z = rng.uniform(0.1, 0.9, 3)
        tris.append([(x, y, z[0]), (x + leg[0], y, z[1]), (x + leg[0], y + leg[1], z[2])])
    return [pc.pixel_case([tris], 64, 64)]


CASES = {"unit96x80": _unit96x80, "ties": _ties, "fans": _fans, "near_clip": _near_clip, "behind_and_beyond": _behind_and_beyond, "mesh130x70": _mesh130x70,
         "far_tiny": _far_tiny, "dense64": _dense64, "draws700": _draws700, "nothing": _nothing, "small_frames": _small_frames,
         "octagon": _octagon, "sub_rejects": _sub_rejects, "motion_edges": _motion_edges, "normal_edges": _normal_edges, "denormal_depth": _denormal_depth,
         "lane_int64": _lane_int64, "crowded_large": _crowded_large}
FIRST_ROUND = ("unit96x80", "ties", "fans", "near_clip", "behind_and_beyond", "mesh130x70", "far_tiny", "dense64", "draws700", "nothing", "small_frames")
_reference_cache = {}


def reference(name):
    """[(case, reference result with its diagnostic lists)], computed once per case and shared by the modes; callers must not modify it"""
    if name not in _reference_cache:
        _reference_cache[name] = [(case, pc.rasterise(case, diagnostics=True)) for case in CASES[name]()]
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



def _fan_indices(r, t=None):
    return tuple(f[1] for f in r["fan_drawn"] if t is None or f[0] == t)


def _check_octagon(runs):
    assert len(runs) == 4
    reached = set()
    for k, (case, r) in enumerate(runs[:3]):
        assert r["polygons"] == [(0, 8), (1, 8), (2, 8)], "every rotation is clipped to 8 vertices: %r" % (r["polygons"],)
        assert counters(r) == OCTAGON_COUNTERS[k] and not r["fan_rejected"]
        assert tuple(_fan_indices(r, t) for t in range(3)) == OCTAGON_FANS[k]
        assert (r["coverage"] == 3).all(), "each of the three octagons covers every pixel exactly once"
        alone = pc.rasterise(dict(case, draws=case["draws"][:1]))
        assert (alone["coverage"] == 1).all() and counters(alone)[:2] == (1, 1), "the sub-triangles of one fan partition the %d pixels" % alone["coverage"].size
        own = owner(r)
        assert all((own == t).sum() > 1000 for t in range(3)), "every rotation is seen"
        reached |= set(_fan_indices(r))
    assert counters(runs[0][1]) == (3, 3, 9, 0) and np.array_equal(runs[0][0]["transforms"][0, 16:32], pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.05], [0, 0, 1, 0]]))
    case, r = runs[3]
    assert r["polygons"] == [(0, 6), (1, 7)] and counters(r) == (2, 2, 6, 0) and (_fan_indices(r, 0), _fan_indices(r, 1)) == ((0, 1, 2), (1, 2, 3))
    own = owner(r)
    assert (own == 0).sum() > 1000 and (own == 1).sum() > 1000
    reached |= set(_fan_indices(r))
    # (sub-triangles 0 and 5 of an octagon on the guard square hold three consecutive vertices of it and cannot contain a point within 1 of the centre: they
    # reach the screen with their boxes only. They are set up, counted and walked; a wrong record would show as coverage that is not there)
    assert reached == {0, 1, 2, 3, 4, 5}, "every fan index is drawn somewhere in the case"
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        poly, clipped = ref.clip_triangle(ref.transform4(octagon_mvp(0), np.asarray([OCTAGON[i] for i in order], F32)))
        assert clipped and len(poly) == 8


def _check_sub_rejects(runs):
    case, r = runs[0]
    assert counters(r) == (14, 6, 4, 13)
    assert r["polygons"] == [(t, 3) for t in range(6)] + [(t, 4) for t in range(6, 12)] + [(12, 3), (13, 3)]
    for winding in range(2):  # the issue's two triangles alone, in either winding: submitted 1, clipped 0, drawn 0, rejects 1
        for first, transform_index in ((0, 0), (12, 1)):
            alone = pc.rasterise(dict(case, draws=pc.draws6([[first + 3 * winding, 3, 0, transform_index]])))
            assert counters(alone) == (1, 0, 0, 1)
    clip = ref.transform4(case["transforms"][0, 16:32], case["positions"][0:3])
    assert not clip[0].any() and all(ref.plane_distance(plane, clip[0]) >= 0 for plane in range(5)), "(0, 0, 0, 0) is inside all five planes"
    assert not ref.project(clip, 96, 64)[3][0], "and fails w > 0"
    clip = ref.transform4(case["transforms"][1, 16:32], case["positions"][12:15])
    with np.errstate(all="ignore"):
        assert np.isfinite(clip).all() and clip[0, 2] < F32(-9e29) and 0 < clip[0, 3] < F32(2e-30) and clip[0, 2] / clip[0, 3] == -np.inf
    assert all(ref.plane_distance(plane, clip[0]) >= 0 for plane in range(5)), "z / w overflows inside the near plane"
    rejected, drawn = set(r["fan_rejected"]), {(f[0], f[1]) for f in r["fan_drawn"]}
    assert rejected == {(0, 0), (1, 0), (4, 0), (5, 0), (6, 0), (7, 0), (7, 1), (8, 0), (8, 1), (9, 0), (10, 0), (10, 1), (11, 1)}
    assert drawn == {(3, 0), (9, 1), (11, 0), (13, 0)}, "triangles 9 and 11 hold a reject and a drawn sub-triangle, in either order"
    own = owner(r)
    assert set(np.unique(own).tolist()) == {-1, 13} and (own == 13).sum() > 500 and (r["coverage"][own == 13] == 2).all(), \
        "the visible triangle behind them, drawn in both draws: the later one wins the tie"


def _motion_of(r, t):
    return np.unique(r["motion"][owner(r) == t].reshape(-1, 2), axis=0).tolist()


def _check_motion_edges(runs):
    case, r = runs[0]
    assert counters(r) == (5, 0, 5, 0) and all((owner(r) == t).sum() == 222 for t in range(5))
    assert all(v != 0 for v in case["jitter_current"] + case["jitter_previous"]) and case["jitter_current"] != case["jitter_previous"]
    assert _motion_of(r, 0) == [[32767, -32767]], "m = (1.5, -1.5) saturates"
    assert _motion_of(r, 1) == [[0, 0]] and _motion_of(r, 2) == [[0, 0]], "a previous w sum of -1 and of 0"
    assert _motion_of(r, 3) == [[0, 0]], "a NaN x stores 0; y has the same jitter in both frames"
    assert _motion_of(r, 4) == [[32766, -32767]], "one code below +1, and just beyond -1"
    previous = case["transforms"][:, 32:48]
    assert previous[1, 15] == -1 and previous[2, 15] == 0 and not previous[2, [3, 7, 11]].any() and np.isnan(previous[3, 12]) and np.isnan(previous[3]).sum() == 1
    assert (case["transforms"][:, :32] == np.tile(pc.IDENTITY, 2)).all(), "identity current matrices"


def _check_normal_edges(runs):
    case, r = runs[0]
    own = owner(r)
    words = lambda t: set(np.unique(r["normal"][own == t]).tolist())
    assert counters(r) == (5, 0, 5, 0)
    assert words(0) == {0xFF808080} and (own == 0).sum() == 222, "a singular mat3(model): n = 0"
    assert words(1) == {0xFF008080, 0xFF808080, 0xFFFF8080}, "(0, 0, 1) and (0, 0, -1) interpolate through zero: z codes 0, 128 and 255"
    assert words(2) == {0xFF008080, 0xFFFF8080}, "only the 1e30 normal normalises to a non-zero vector: +z, or -z where rounding leaves its weight below zero"
    assert len(words(3)) > 100, "normals of three lengths and directions through scale and shear: a word of its own for almost every pixel"
    assert len(words(4)) == 1 and words(4) != {0xFFFF8080}, "the face normal (0, 0, 1) through the sheared mat3"
    m = case["transforms"][3, :16].reshape(4, 4).T[:3, :3].astype(np.float64)
    want = m @ np.array([0.0, 0.0, 1.0])
    want /= np.linalg.norm(want)
    got = np.array([(words(4).copy().pop() >> s) & 0xFF for s in (0, 8, 16)])
    assert np.abs(got - np.rint((want * 0.5 + 0.5) * 255)).max() <= 1 and abs(want[0]) > 0.05
    assert np.array_equal(case["transforms"][4, :16], case["transforms"][3, :16]) and not case["normals"][12:15].any()
    lengths = np.linalg.norm(case["normals"][9:12].astype(np.float64), axis=1)
    assert (np.abs(lengths - 1.0) > 0.5).all(), "stored normals that are not unit length"


DENORMAL_LIMIT = 0x00800000  # the bits of the least normal float


def _check_denormal_depth(runs):
    case, r = runs[0]
    bits, own = r["depth"].view(np.uint32), owner(r)
    assert counters(r) == (6, 0, 6, 0)
    assert F32(DENORMAL_LEAST).view(np.uint32) == 1 and F32(DENORMAL_TWO).view(np.uint32) == 2 and F32(NORMAL_LEAST).view(np.uint32) == DENORMAL_LIMIT
    assert 1 < F32(DENORMAL_SMALL).view(np.uint32) < DENORMAL_LIMIT
    for t, z, pixels in ((0, DENORMAL_SMALL, 406), (1, DENORMAL_LEAST, 328), (2, NORMAL_LEAST, 406), (5, DENORMAL_TWO, 78)):
        assert (own == t).sum() == pixels and (r["depth"][own == t] == F32(z)).all(), "a constant denormal depth is kept and stored as it is"
    assert not (own == 4).any() and (r["coverage"][2:16, 12:24].max() == 2), "the least denormal loses to 1e-41, and wins nowhere else"
    ramp = own == 3
    assert ramp.sum() > 80 and (bits[ramp] > 0).all() and (bits[ramp] < F32(DENORMAL_SMALL).view(np.uint32)).all() and len(np.unique(bits[ramp])) >= 10
    assert ramp[:, :48].sum() == ramp.sum() and ramp[35, 47], "the far rule cuts the ramp at x = 48, inside the denormal range"
    kept = r["keys"] != 0
    assert ((bits[kept] < DENORMAL_LIMIT).sum() > 800) and (bits[kept] != 0).all(), "no kept depth is 0"


def _tiles_of(tri, width, height):
    """by hand from ref.project and the box formula: per 64 x 64 tile the triangle's box reaches, (tile, box inside the tile, pixels it keeps there, snapped span)"""
    case = pc.pixel_case([[tri]], width, height)
    X, Y, _, ok = ref.project(np.concatenate([case["positions"], np.ones((3, 1), F32)], axis=1), width, height)
    assert ok.all()
    ix0, ix1 = max(0, (int(X.min()) + 127) >> 8), min(width - 1, (int(X.max()) - 128) >> 8)
    iy0, iy1 = max(0, (int(Y.min()) + 127) >> 8), min(height - 1, (int(Y.max()) - 128) >> 8)
    kept = pc.rasterise(case)["coverage"]
    out = []
    for ty in range(iy0 >> 6, (iy1 >> 6) + 1):
        for tx in range(ix0 >> 6, (ix1 >> 6) + 1):
            bx0, bx1, by0, by1 = max(ix0, 64 * tx), min(ix1, 64 * tx + 63), max(iy0, 64 * ty), min(iy1, 64 * ty + 63)
            out.append(((tx, ty), (bx1 - bx0 + 1, by1 - by0 + 1), int(kept[by0:by1 + 1, bx0:bx1 + 1].sum()), max(int(X.max() - X.min()), int(Y.max() - Y.min()))))
    return out


def _check_lane_int64(runs):
    case, r = runs[0]
    assert counters(r) == (2, 0, 2, 0) and (owner(r) == 0).sum() > 100 and (owner(r) == 1).sum() > 100
    row, column = _tiles_of(LANE_INT64_ROW, 96, 80), _tiles_of(LANE_INT64_COLUMN, 96, 80)
    assert [(tile, box) for tile, box, _, _ in row] == [((0, 0), (64, 4)), ((1, 0), (3, 4))]
    assert [(tile, box) for tile, box, _, _ in column] == [((0, 0), (4, 64)), ((0, 1), (4, 3))]
    for tiles in (row, column):
        assert all(span >= NARROW_SPAN and kept > 0 for _, _, kept, span in tiles), "64-bit edge functions in both tiles, and pixels kept in both"
        (_, large, _, _), (_, small, kept, _) = tiles
        assert max(large) > 4 and max(small) <= 4 and kept >= 5, "the wave path in the first tile, the lane path in the next one"
    c = r["coverage"]
    assert c[10:14, 64:67].sum() >= 5 and c[64:67, 10:14].sum() >= 5


def _check_crowded_large(runs):
    case, r = runs[0]
    assert counters(r) == (250, 0, 250, 0) and case["draws"].shape[0] == 1 and case["width"] == case["height"] == 64
    first = r["fan_drawn"][:256]
    assert [f[0] for f in first] == list(range(250)), "one set-up block: the records are in submission order, all within the first 256-rectangle step"
    large = [max(x1 - x0, y1 - y0) >= 4 for _, _, (x0, y0, x1, y1), _ in first]
    assert sum(large) >= 150 and len(large) - sum(large) >= 40, "%d boxes larger than 4 x 4 (the wave path), %d lane-path boxes among them" % (sum(large), len(large) - sum(large))
    assert max(sum(large[k:k + 64]) for k in range(0, 256, 64)) < 64 and sum(large[64:]) > 100, "wave-path hits in the second and later rounds of 64"
    own = owner(r)
    assert len(np.unique(own[own >= 0])) >= 100 and r["coverage"].max() >= 8, "winners interleave"


CASE_CHECKS = {"unit96x80": _check_unit96x80, "ties": _check_ties, "fans": _check_fans, "near_clip": _check_near_clip, "behind_and_beyond": _check_behind_and_beyond,
               "mesh130x70": _check_mesh130x70, "far_tiny": _check_far_tiny, "dense64": _check_dense64, "draws700": _check_draws700, "nothing": _check_nothing,
               "small_frames": _check_small_frames, "octagon": _check_octagon, "sub_rejects": _check_sub_rejects, "motion_edges": _check_motion_edges,
               "normal_edges": _check_normal_edges, "denormal_depth": _check_denormal_depth, "lane_int64": _check_lane_int64, "crowded_large": _check_crowded_large}


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


def gpu_prepass(be, case, scratch=None, formats=FORMATS, sizes=None, dispatch=(1, 1, 1), push=None, scratch_read_only=False, same_image=None, scratch_as_input=None):
    """one execution through the C-ABI with the test's own buffers -> (dict of the five images as uint32 h x w, (submitted, clipped, drawn, rejects)).
    For the refusals: `scratch` its size in bytes, `formats` and `sizes` of the five images, `dispatch`, `push` the push constant bytes, `scratch_read_only`,
    `same_image` (a, b): storage binding b gets the image of binding a, `scratch_as_input`: the input binding that gets the scratch buffer as well"""
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
    if same_image is not None:
        images[same_image[1]] = images[same_image[0]]
    bound = list(buffers)
    if scratch_as_input is not None:
        bound[scratch_as_input] = buffers[5]
    p = be.createComputePass("depthPrepassRaster.comp", [], "Depth prepass")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(img, 0, k) for k, img in enumerate(images)],
        storageBuffers=[StorageBufferResource(b, i != 5 or scratch_read_only, i) for i, b in enumerate(bound)]),
        struct.pack("<2I", case["draws"].shape[0], triangles) if push is None else push, tuple(dispatch)))
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
            start = time.perf_counter()
            out, counted = gpu_prepass(backend, case)
            seconds = time.perf_counter() - start
            general = backend.getGeneralKernelExecutions()
            print("prepass raster %s[%d] %s: upload, pass and download %.2f ms" % (name, k, "fast" if fast else "exact", 1e3 * seconds))
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


TALLEST_WIDTH, TALLEST_HEIGHT = 3, 16384


def _tallest():
    """the widest image's triangles transposed, second and third vertex exchanged so that they face front again"""
    tris = [[(-0.75, 64.0 * ty + 10.5, 0.3 + 0.002 * ty), (3.5, 64.0 * ty + 30.25, 0.4), (0.25, 64.0 * ty + 80.5, 0.5)] for ty in LARGEST_TILES]
    return pc.pixel_case([tris], TALLEST_WIDTH, TALLEST_HEIGHT)


def check_tallest_is_what_it_is_for():
    if "tallest" not in _reference_cache:
        case = _tallest()
        _reference_cache["tallest"] = (case, pc.rasterise(case))
    case, r = _reference_cache["tallest"]
    assert counters(r) == (4, 0, 4, 0), "all four face front"
    for ty in LARGEST_TILES:
        assert r["coverage"][64 * ty:64 * ty + 64].any() and (ty == 255 or r["coverage"][64 * ty + 64:64 * ty + 128].any())
    assert r["coverage"][TALLEST_HEIGHT - 1].any()
    return case, r


def test_tallest_image_case_is_what_it_is_for():
    """not gpu: the input conditions of the GPU test below"""
    check_tallest_is_what_it_is_for()


@pytest.mark.gpu
def test_gpu_prepass_raster_reaches_the_largest_height(backend):
    """16384 texels tall = 256 tile rows: the tile rectangle keeps its rows in bits 8 .. 15 and 24 .. 31, rows 128 and above set the top bit of each; one math mode"""
    case, r = check_tallest_is_what_it_is_for()
    start = time.perf_counter()
    out, counted = gpu_prepass(backend, case)
    print("prepass raster tallest image: upload, pass and download %.2f ms" % (1e3 * (time.perf_counter() - start)))
    compare("tallest image %d x %d" % (TALLEST_WIDTH, TALLEST_HEIGHT), out, counted, r)


@pytest.mark.gpu
def test_gpu_launcher_refuses_what_it_cannot_run(backend):
    """fails loudly: a scratch buffer too small for the triangle count (the message states the size formula), a depth image that is not Depth32, images of two sizes,
    images wider than the largest, another dispatch, push constants that are short or contradict themselves or count too many triangles, a scratch buffer that is
    read-only or also an input, one image at two bindings. A refusal leaves nothing behind: the next execution is bit-identical to the reference"""
    from plainrenderer_amd.backend import PlrError
    case = _unit96x80()[0]
    with pytest.raises(PlrError, match="scratch.*576 triangleCount"):
        gpu_prepass(backend, case, scratch=64)
    with pytest.raises(PlrError, match="Depth32"):
        gpu_prepass(backend, case, formats=(ImageFormat.R16_sFloat,) + FORMATS[1:])
    with pytest.raises(PlrError, match="one size"):
        gpu_prepass(backend, case, sizes=[(96, 80), (96, 80), (96, 80), (96, 64), (96, 80)])
    with pytest.raises(PlrError, match="at most 16384"):
        gpu_prepass(backend, case, sizes=[(16385, 1)] * 5)
    for dispatch in ((2, 1, 1), (1, 3, 1), (1, 1, 2)):
        with pytest.raises(PlrError, match=r"the dispatch is \{1, 1, 1\}"):
            gpu_prepass(backend, case, dispatch=dispatch)
    for counts in ((0, 3), (1, 0)):
        with pytest.raises(PlrError, match="both be zero or both be non-zero"):
            gpu_prepass(backend, case, push=struct.pack("<2I", *counts))
    with pytest.raises(PlrError, match=r"triangleCount 268435457 exceeds 2\^28"):  # (before the scratch size is looked at: the scratch buffer is the case's own)
        gpu_prepass(backend, case, push=struct.pack("<2I", 1, (1 << 28) + 1))
    with pytest.raises(PlrError, match="scratch buffer.*bound read-only"):
        gpu_prepass(backend, case, scratch_read_only=True)
    with pytest.raises(PlrError, match="one image is bound at two storage bindings"):
        gpu_prepass(backend, case, same_image=(2, 3))
    with pytest.raises(PlrError, match="scratch buffer is also bound as an input"):
        gpu_prepass(backend, case, scratch_as_input=1)
    for short in (b"", struct.pack("<I", 1), struct.pack("<2I", 1, 17)[:7]):
        with pytest.raises(PlrError, match="push constants.*missing"):
            gpu_prepass(backend, case, push=short)
    check_case_is_what_it_is_for("unit96x80")
    case, r = reference("unit96x80")[0]
    out, counted = gpu_prepass(backend, case)
    compare("unit96x80 after the refusals", out, counted, r)
