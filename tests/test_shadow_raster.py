"""The "sunShadowRaster.comp" pass through the C-ABI against tests/shadow_raster_reference.py, in both math modes: every texel of the Depth16 map and the three
counters must be bit-identical.

The map is pre-filled with a bit pattern (the pass clears: an untouched texel would keep it) and the scratch buffer with 0xA5 bytes (the pass resets its own
header). Every case binds a sunShadowInfo block whose other light matrices are garbage, so the cascade index constant is what selects the matrix.
Cases, the smallest that reach every way the kernels can go wrong:
  unit96    res 96 = 1.5 tiles per axis (a ragged tile column and row, 16-byte rows). Hand-made triangles on the sub-pixel grid: a quad split along a diagonal
            through pixel centres and an axis-aligned quad with edges on pixel centres, two depths per half; a triangle whose pixel box is exactly 4 x 4 (the
            lane-per-triangle path's largest) and one that is 5 x 4 (the wave path's smallest); a triangle that straddles the tile boundary x = 64 and a small
            one that does; overlapping triangles at three depths in the second tile row; two long triangles, one
            just inside and one outside the span the kernel evaluates in 32-bit arithmetic; a front face and a zero-area triangle that draw nothing
  mesh200   res 200 (3.125 tiles, rows of 400 bytes: 16-byte stores), box + uv_sphere + torus under three affine transforms, 1496 triangles, once per cascade
            with the three matrices of SynthScene.shadow_cascades
  dense64   res 64, one tile, 20 011 random triangles a quarter of a pixel to 3 pixels across (not a multiple of 64: the list's tail), some outside the map,
            two fifths of them clustered so that texels collect eight fragments and more
  big130    res 130 (odd rows: texel-by-texel stores): a triangle over the whole map with one vertex 99 970 pixels outside and depths from below 0 to above 1,
            two slivers narrower than a pixel across the whole map (apex 270 pixels outside), one triangle with a vertex 2^21 pixels out (the guard band's reject)
  draws700  res 136 (2.125 tiles, 16-byte rows): the set-up kernel's draw lookup. 700 draws of a 12-triangle box, a 528-triangle sphere (one draw spans three
            set-up blocks) and an empty mesh; the first two draws, the last three and draws 200 .. 599 - the whole chunk 256 .. 511 - are empty, a few box draws
            have an indexCount of 34 and 35 (11 triangles), 450 transforms serve the 700 draws through a permutation, so slots are shared and no draw's
            transformIndex is its own number by construction. A second execution of 300 box draws puts triangles into draw 256, the first of a later chunk
  nothing   res 72, three executions that draw nothing and must still clear the map: no draw and no triangle at all (the set-up kernel is not launched);
            only front faces, zero-area triangles and triangles whose pixel box is empty or misses the map (a cursor of 0 behind a set-up launch); only rejects
  small_maps  res 1, 7, 8, 63 and 65 - smaller than a tile, a row of exactly one 16-byte store, the last texel-wise row below and the first above a tile: a triangle
            over the whole map with a depth gradient, from res 7 on two triangles of at most 4 x 4 pixels, at res 65 one that crosses x = 64
  fans      res 96, eight back faces around a centre vertex on a pixel centre, rim vertices at (+-r, 0), (0, +-r), (+-r, +-r), a depth per triangle: all eight
            edge directions through pixel centres, every tie-break decides a code. r = 1.5 (the lane path), r = 20 (the wave path in int32), r = 3 on the
            corner of four tiles; as an execution of its own r = 150 around (48.5, 47.5): every triangle spans 38400 units, the int64 path, clipped at all four map edges
  steep_huge  res 64, one triangle with vertices a million pixels out whose depth plane crosses the map inside 0 .. 1 at about 0.002 per pixel: some 3660
            distinct codes, so that the fragment's float part (int64 -> fp32 to nearest even, a true divide, no contraction) shows in thousands of texels
  band_edges  res 64 (xf = 32 (cx + 1) is exact): vertices at xf, yf = 2^20 - 1/16 and -(2^20 - 1/8) are drawn, at +-2^20 rejected; a NaN x, a +inf y, a -inf z,
            a finite 3e38 under a model matrix of scale 2 and a draw whose transform has a NaN translation are rejected; z = 3.4e38 at one vertex is
            drawn and clamps; a triangle with z0 = -3e38, z1 = 3e38 has zf = NaN on its edge 2 -> 0 (a left edge through 15 pixel centres) and +inf beside it:
            code 0 under the clamp's fmax / fmin, so those texels keep the code of the flat quad below
  outside_buffers  res 64, ten ordinary triangles and three draws that leave their buffers by exactly one element: the last index slot, a vertex equal to the
            vertex count through vertexOffset, a transformIndex equal to the transform count. Those triangles are counted rejects; their neighbours are drawn
The largest map (16384: tile indices 0, 127, 128 and 255 in every byte of a tile rectangle) has a test of its own.
"""
import struct

import numpy as np
import pytest

import shadow_raster_cases as sc
import shadow_raster_reference as ref
from plainrenderer_amd.backend import spec_uint
from util import ComputePassExecution, ImageFormat, ImageResource, RenderPassResources, StorageBufferResource, image_desc_2d

TRI_4X4 = [(40.0, 40.0, 0.35), (44.0, 40.0, 0.35), (44.0, 44.0, 0.45)]
TRI_5X4 = [(50.0, 40.0, 0.55), (55.0, 40.0, 0.55), (55.0, 44.0, 0.65)]
# the kernel evaluates a triangle whose snapped vertices span less than 2^15 sub-pixel units on both axes in 32-bit arithmetic: the widest that does, and one that does not
TRI_SPAN_32767 = [(-20.0, 60.0, 0.45), (107.99609375, 61.0, 0.45), (-20.0, 63.0, 0.7)]
TRI_SPAN_33280 = [(-20.0, 56.0, 0.4), (110.0, 57.0, 0.4), (-20.0, 59.0, 0.6)]


def _unit96():
    tris = sc.quad(2.5, 2.5, 10.5, 10.5, 0.3, 0.6) + sc.quad(20.5, 4.5, 30.5, 9.5, 0.4, 0.7) + [TRI_4X4, TRI_5X4]
    tris += [[(60.25, 20.5, 0.2), (70.75, 22.0, 0.5), (66.0, 30.25, 0.8)], [(62.0, 50.0, 0.3), (66.0, 50.0, 0.3), (66.0, 53.0, 0.9)]]
    tris += [[(5.0, 66.0, 0.5), (60.0, 66.0, 0.5), (60.0, 94.0, 0.5)], [(10.0, 70.0, 0.25), (50.0, 70.0, 0.25), (50.0, 90.0, 0.25)],
             [(30.0, 68.0, 0.8), (58.0, 68.0, 0.8), (58.0, 96.0, 0.8)]]
    tris += sc.quad(70.5, 70.5, 90.5, 95.5, 0.2, 0.9) + [TRI_SPAN_32767, TRI_SPAN_33280]
    tris += [[(10.0, 40.0, 0.5), (10.0, 50.0, 0.5), (20.0, 40.0, 0.5)]]  # A < 0: a front face
    tris += [[(30.0, 60.0, 0.5), (35.0, 65.0, 0.5), (40.0, 70.0, 0.5)]]  # A == 0
    return [(sc.pixel_case(tris, 96), 2)]


def _mesh200():
    lights = ref.light_matrices(sc.mesh_scene()["info"])
    return [(sc.mesh_case(lights[c], 200), c) for c in range(3)]


def _dense64():
    """three fifths of the triangles uniform over the tile and 2 pixels around it, two fifths clustered (sigma 3 pixels) so that some texels collect many fragments;
    each triangle three points on a circle of diameter `across` at roughly 120 degrees, random winding"""
    rng = np.random.default_rng(0x53484457)
    n = 20011
    centre = np.where(rng.random((n, 1)) < 0.6, rng.uniform(-2.0, 66.0, (n, 2)), rng.normal((21.3, 40.7), 3.0, (n, 2)))[:, None, :]
    across = rng.uniform(0.25, 3.0, (n, 1))
    angle = rng.uniform(0.0, 2.0 * np.pi, (n, 1)) + np.where(rng.random((n, 1)) < 0.5, 1.0, -1.0) * (np.arange(3)[None, :] * 2.0 * np.pi / 3.0 + rng.uniform(-0.4, 0.4, (n, 3)))
    px = centre + 0.5 * across[:, :, None] * np.stack([np.cos(angle), np.sin(angle)], -1)
    pos = np.concatenate([2.0 * px / 64.0 - 1.0, rng.uniform(0.05, 0.95, (n, 3, 1))], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(3 * n, dtype=np.uint32)
    return [(dict(res=64, light=sc.IDENTITY.copy(), transforms=sc.IDENTITY.reshape(1, 16).copy(), positions=pos, indices=idx, draws=np.array([[0, 3 * n, 0, 0]], np.uint32)), 1)]


SLIVERS = [[(-5.0, 30.25, 0.9), (400.0, 75.0, 0.9), (-5.0, 30.875, 0.9)], [(-3.0, -3.0, 0.95), (400.0, 399.0, 0.95), (-3.0, -2.25, 0.95)]]


def _big130():
    tris = [[(-200.0, -20.0, -0.5), (99970.0, 60.0, 0.5), (-200.0, 150.0, 1.5)],
            SLIVERS[0], SLIVERS[1],
            [(float(2 ** 21), 10.0, 0.5), (5.0, 5.0, 0.5), (5.0, 20.0, 0.5)]]
    return [(sc.pixel_case(tris, 130), 3)]


def raw_case(res, positions, indices, draws, transforms=None):
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    transforms = sc.IDENTITY.reshape(1, 16).copy() if transforms is None else np.asarray(transforms, np.float32).reshape(-1, 16)
    return dict(res=res, light=sc.IDENTITY.copy(), transforms=transforms, positions=positions, indices=np.asarray(indices, np.uint32).reshape(-1),
                draws=np.asarray(draws, np.uint32).reshape(-1, 4))


DRAWS700_SHORT = {20: 34, 21: 35, 150: 34, 640: 35}  # box draws whose indexCount is no multiple of 3: 11 triangles each
DRAWS700_TRANSFORMS = 450


def _draws700_mesh(d):
    """0 the box, 1 the empty mesh, 2 the sphere"""
    if d < 2 or d >= 697 or 200 <= d < 600:
        return 1
    return 2 if d % 97 == 0 else 0


def _draws700():
    from plainrenderer_amd import meshes
    ms = [sc.as_arrays(meshes.box(subdiv=1)), (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.zeros(0, np.uint32)),
          sc.as_arrays(meshes.uv_sphere(1.0, segments=24, rings=12))]
    assert [m[1].size for m in ms] == [36, 0, 1584]
    rng = np.random.default_rng(0x44523730)
    transforms = np.array([sc.affine(np.full(3, 0.06 * rng.uniform(0.8, 1.25)), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(-1.0, 1.0),
                                     (rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), rng.uniform(0.2, 0.8))) for _ in range(DRAWS700_TRANSFORMS)], np.float32)
    slot = rng.permutation(DRAWS700_TRANSFORMS)
    pos, idx, merged, _ = ref.merge_meshes(ms, [(m, sc.IDENTITY) for m in range(3)])  # (one draw per mesh: its firstIndex and vertexOffset)
    draws = np.zeros((700, 4), np.uint32)
    for d in range(700):
        m = _draws700_mesh(d)
        draws[d] = (merged[m, 0], DRAWS700_SHORT.get(d, merged[m, 1]), merged[m, 2], slot[d % DRAWS700_TRANSFORMS])
    # a second execution for the `running` carry alone: 300 box draws, so that draw 256 - the first of the second chunk, whose base is the carry and not an
    # entry of the prefix sum - holds triangles; its neighbours 255 and 257 are empty
    carry = np.zeros((300, 4), np.uint32)
    for d in range(300):
        m = 1 if d in (255, 257) else 0
        carry[d] = (merged[m, 0], merged[m, 1], merged[m, 2], slot[d])
    return [(raw_case(136, pos, idx, draws, transforms), 1), (raw_case(136, pos, idx, carry, transforms), 3)]


def _nothing():
    empty = raw_case(72, np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint32))
    undrawn = [[(10.0, 40.0, 0.5), (10.0, 50.0, 0.5), (20.0, 40.0, 0.5)],  # a front face
               [(30.0, 60.0, 0.5), (35.0, 65.0, 0.5), (40.0, 70.0, 0.5)], [(5.0, 5.0, 0.5), (5.0, 5.0, 0.5), (9.0, 9.0, 0.5)],  # zero area
               [(20.625, 20.625, 0.5), (21.375, 20.625, 0.5), (21.375, 21.375, 0.5)],  # between four pixel centres: an empty box inside the map
               [(-30.0, 10.0, 0.5), (-2.0, 10.0, 0.5), (-2.0, 40.0, 0.5)], [(73.0, 10.0, 0.5), (100.0, 10.0, 0.5), (100.0, 40.0, 0.5)],  # left and right of the map
               [(10.0, -40.0, 0.5), (50.0, -40.0, 0.5), (50.0, -1.0, 0.5)], [(10.0, 72.5, 0.5), (50.0, 72.5, 0.5), (50.0, 99.0, 0.5)],  # above and below
               [(71.75, 10.0, 0.5), (90.0, 10.0, 0.5), (90.0, 40.0, 0.5)]]  # starts behind the last pixel centre 71.5
    far = float(2 ** 21)
    rejected = [[(far, 10.0, 0.5), (5.0, 5.0, 0.5), (5.0, 20.0, 0.5)], [(5.0, 5.0, 0.5), (60.0, -far, 0.5), (60.0, 30.0, 0.5)],
                [(-far, 10.0, 0.5), (50.0, 5.0, 0.5), (50.0, 20.0, 0.5)], [(5.0, 5.0, 0.5), (60.0, 5.0, 0.5), (60.0, far, 0.5)],
                [(5.0, 40.0, 0.5), (60.0, 40.0, np.inf), (60.0, 60.0, 0.5)]]
    return [(empty, 0), (sc.pixel_case(undrawn, 72), 1), (sc.pixel_case(rejected, 72), 2)]


SMALL_MAPS = (1, 7, 8, 63, 65)
SMALL_TRIS = [[(1.0, 2.0, 0.95), (5.0, 2.0, 0.95), (5.0, 6.0, 0.85)], [(3.25, 0.5, 0.75), (6.75, 1.0, 0.8), (4.5, 3.5, 0.7)]]  # at most 4 x 4 pixels, inside a 7 x 7 map
TRI_ACROSS_64 = [(61.5, 20.0, 0.9), (66.0, 20.0, 0.9), (66.0, 23.5, 0.6)]


def _small_maps():
    out = []
    for k, res in enumerate(SMALL_MAPS):
        tris = [[(-1.0, -1.0, 0.1), (2.0 * res + 2.0, -1.0, 0.9), (-1.0, 2.0 * res + 2.0, 0.5)]]
        if res >= 7:
            tris += SMALL_TRIS
        if res == 65:
            tris += [TRI_ACROSS_64]
        out.append((sc.pixel_case(tris, res), k % 4))
    return out


FANS = ((10.5, 10.5, 1.5), (40.5, 60.5, 20.0), (63.5, 63.5, 3.0))
FAN_INT64 = (48.5, 47.5, 150.0)
FAN_RIM = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))  # clockwise on the y-down screen: (centre, rim k, rim k + 1) has A > 0


def fan(cx, cy, r):
    """eight triangles, triangle k at depth 0.1 (k + 1)"""
    return [[(cx, cy, 0.1 * (k + 1)), (cx + r * FAN_RIM[k][0], cy + r * FAN_RIM[k][1], 0.1 * (k + 1)),
             (cx + r * FAN_RIM[(k + 1) % 8][0], cy + r * FAN_RIM[(k + 1) % 8][1], 0.1 * (k + 1))] for k in range(8)]


def _fans():
    return [(sc.pixel_case(sum((fan(*f) for f in FANS), []), 96), 0), (sc.pixel_case(fan(*FAN_INT64), 96), 3)]


STEEP_HUGE = ((-1000001.0, -900007.0), (1000003.0, -800011.0), (3.0, 1000033.0))


def _steep_huge():
    tri = [(x, y, float(np.float32(0.5 + 0.0017 * (x - 32.0) - 0.0011 * (y - 32.0)))) for x, y in STEEP_HUGE]
    return [(sc.pixel_case([tri], 64), 2)]


def fragment_codes(case, to_f32=None, divide=None, mad=None):
    """the codes of the case's first triangle at every texel of its map, from the contract's formula with the three steps that a kernel can get subtly wrong
    replaceable: the int64 -> fp32 conversion, the divide, the multiply-add. With the defaults it is the contract's arithmetic."""
    to_f32 = to_f32 or (lambda e: e.astype(np.float32))
    divide = divide or (lambda a, b: a / b)
    mad = mad or (lambda a, b, c: a + b * c)
    res = case["res"]
    X, Y, z, inside = ref.project(case["light"], case["transforms"][0], case["positions"][:3], res)
    assert inside.all()
    (x0, x1, x2), (y0, y1, y2) = (int(v) for v in X), (int(v) for v in Y)
    px = (np.arange(res, dtype=np.int64) * 256 + 128)[None, :]
    py = (np.arange(res, dtype=np.int64) * 256 + 128)[:, None]
    e01 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
    e20 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
    area = np.array([(x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)], np.int64)
    fa = to_f32(area)[0]
    l1, l2 = divide(to_f32(e20), fa), divide(to_f32(e01), fa)
    zf = mad(mad(z[0], l1, np.float32(z[1] - z[0])), l2, np.float32(z[2] - z[0]))
    return np.rint(ref.clamp01(zf) * np.float32(65535.0)).astype(np.uint16)


def truncating_f32(e):
    """int64 -> fp32 towards zero"""
    f = e.astype(np.float32)
    return np.where(np.abs(f.astype(np.int64)) > np.abs(e), np.nextafter(f, np.float32(0.0)), f)


def reciprocal_divide(a, b):
    return a * (np.float32(1.0) / b)


def fused_mad(a, b, c):
    """fma(b, c, a): the product of two fp32 is exact in fp64; one rounding to fp64 and one to fp32 instead of fp32's two"""
    return (np.float64(a) + np.asarray(b, np.float64) * np.float64(c)).astype(np.float32)


WRONG_FRAGMENTS = {"truncating int64 -> fp32": dict(to_f32=truncating_f32), "reciprocal times numerator": dict(divide=reciprocal_divide), "contracted multiply-adds": dict(mad=fused_mad)}

BAND_IN_HIGH, BAND_IN_LOW, BAND = 2.0 ** 20 - 1.0 / 16.0, -(2.0 ** 20 - 1.0 / 8.0), 2.0 ** 20
NAN_DEPTH_TRI = [(20.5, 44.5, -3e38), (36.5, 52.5, 3e38), (20.5, 60.5, 0.5)]  # edge 2 -> 0 runs up the pixel centres (20.5, 45.5 .. 59.5): a left edge


def _band_edge_tris(x_high, x_low, y_low, y_high, z):
    """four long triangles, each with one vertex at the given coordinate far outside the map"""
    return [[(10.0, 10.0, z), (x_high, 12.0, z), (10.0, 20.0, z)], [(x_low, 30.0, z), (20.0, 28.0, z), (20.0, 36.0, z)],
            [(40.0, y_low, z), (44.0, 50.0, z), (36.0, 50.0, z)], [(50.0, 5.0, z), (58.0, 5.0, z), (54.0, y_high, z)]]


BAND_DRAWN = _band_edge_tris(BAND_IN_HIGH, BAND_IN_LOW, BAND_IN_LOW, BAND_IN_HIGH, 0.4)
BAND_REJECTED = _band_edge_tris(BAND, -BAND, -BAND, BAND, 0.9)


def _band_edges():
    res = 64
    ordinary = lambda z: [(2.0, 52.0, z), (12.0, 52.0, z), (12.0, 62.0, z)]
    # draw 0, identity: the band's two sides, three non-finite positions, the depth that clamps, the NaN depth over its flat quad
    tris = BAND_DRAWN + BAND_REJECTED + [ordinary(0.9)] * 3 + [[(2.0, 40.0, 3.4e38), (8.0, 40.0, 0.5), (8.0, 46.0, 0.5)]] + sc.quad(18.0, 42.0, 40.0, 63.0, 0.25, 0.25) + [NAN_DEPTH_TRI]
    # draw 1, scale 2 (positions halved): a finite 3e38 whose product overflows; draw 2, a NaN translation: two triangles that would be drawn under a finite one
    tris += [ordinary(0.9)] + [ordinary(0.9), [(30.0, 2.0, 0.9), (34.0, 2.0, 0.9), (34.0, 8.0, 0.9)]]
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    pos = t.reshape(-1, 3).copy()
    pos[:, :2] = 2.0 * pos[:, :2] / res - 1.0
    pos = pos.astype(np.float32)
    n0 = len(tris) - 3
    first = 3 * (len(BAND_DRAWN) + len(BAND_REJECTED))
    pos[first, 0], pos[first + 4, 1], pos[first + 8, 2] = np.nan, np.inf, -np.inf
    pos[3 * n0:3 * n0 + 3] *= np.float32(0.5)
    pos[3 * n0, 0] = 3e38
    scale2, nan_translation = sc.glm(np.diag([2.0, 2.0, 2.0, 1.0])), sc.IDENTITY.copy()
    nan_translation[13] = np.nan
    draws = [[0, 3 * n0, 0, 0], [3 * n0, 3, 0, 1], [3 * n0 + 3, 6, 0, 2]]
    return [(raw_case(res, pos, np.arange(pos.shape[0]), draws, [sc.IDENTITY, scale2, nan_translation]), 0)]


def _outside_buffers():
    res = 64
    ordinary = [[(3.0 + 12.0 * (k % 5), 4.0 + 28.0 * (k // 5), 0.2 + 0.05 * k), (12.0 + 12.0 * (k % 5), 5.0 + 28.0 * (k // 5), 0.3), (11.0 + 12.0 * (k % 5), 24.0 + 28.0 * (k // 5), 0.6)]
                for k in range(10)]
    extra = [[(20.0, 26.0, 0.9), (30.0, 26.0, 0.9), (30.0, 31.0, 0.9)], [(40.0, 26.0, 0.95), (50.0, 26.0, 0.95), (50.0, 31.0, 0.95)]]  # the vertices of the vertexOffset draw
    base = sc.pixel_case(ordinary + extra, res)
    pos = base["positions"]  # 36 vertices
    shift = lambda dx, dy: sc.glm([[1, 0, 0, 2.0 * dx / res], [0, 1, 0, 2.0 * dy / res], [0, 0, 1, 0.02], [0, 0, 0, 1]])
    transforms = [sc.IDENTITY, shift(1.0, 26.0), shift(-2.0, 27.0)]
    # draw 0 the ordinary triangles; draw 1 (vertexOffset 30): its second triangle's last vertex is 6 + 30 = 36, the vertex count; draw 2: its transformIndex is 3, the
    # transform count; draw 3, at the end of the index buffer: its second triangle's third slot is the index count
    idx = list(range(30)) + [0, 1, 2, 3, 4, 6] + [0, 1, 2, 3, 4, 5] + [0, 1, 2, 3, 4]
    draws = [[0, 30, 0, 0], [30, 6, 30, 0], [36, 6, 0, 3], [42, 6, 0, 1]]
    case = raw_case(res, pos, idx, draws, transforms)
    return [(case, 1)]


CASES = {"unit96": _unit96, "mesh200": _mesh200, "dense64": _dense64, "big130": _big130, "draws700": _draws700, "nothing": _nothing, "small_maps": _small_maps,
         "fans": _fans, "steep_huge": _steep_huge, "band_edges": _band_edges, "outside_buffers": _outside_buffers}
# per execution (submitted, drawn, rejects) where the case fixes them
DRAWS_NOTHING = {"nothing": [(0, 0, 0), (9, 0, 0), (5, 0, 5)]}
REJECTS = {"big130": [1], "nothing": [0, 0, 5], "band_edges": [10], "outside_buffers": [4]}
_reference_cache = {}


def reference(name):
    """[(case, cascade index, reference result)], computed once per case and shared by the modes; callers must not modify it"""
    if name not in _reference_cache:
        _reference_cache[name] = [(case, cascade, sc.rasterise(case)) for case, cascade in CASES[name]()]
    return _reference_cache[name]


def _pixel_box(tri, res):
    case = sc.pixel_case([tri], res)
    X, Y, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], res)
    return ((int(X.max()) - 128) >> 8) - ((int(X.min()) + 127) >> 8) + 1, ((int(Y.max()) - 128) >> 8) - ((int(Y.min()) + 127) >> 8) + 1, sc.rasterise(case)["coverage"].sum()


def check_case_is_what_it_is_for(name):
    """on the reference alone: the properties the case is there for"""
    runs = reference(name)
    assert [r["rejects"] for _, _, r in runs] == REJECTS.get(name, [0] * len(runs))
    if name in DRAWS_NOTHING:
        assert [(r["submitted"], r["drawn"], r["rejects"]) for _, _, r in runs] == DRAWS_NOTHING[name]
        assert not any(r["map"].any() or r["coverage"].any() for _, _, r in runs)
    else:
        assert all(r["drawn"] > 0 and r["map"].any() for _, _, r in runs)
    if name in NEW_CASE_CHECKS:
        NEW_CASE_CHECKS[name](runs)
    elif name == "unit96":
        w, h, covered = _pixel_box(TRI_4X4, 96)
        assert (w, h) == (4, 4) and covered > 0
        w, h, covered = _pixel_box(TRI_5X4, 96)
        assert (w, h) == (5, 4) and covered > 0
        r = runs[0][2]
        assert r["submitted"] == 17 and r["drawn"] == 15, "the front face and the zero-area triangle are not drawn"
        for tri, span in ((TRI_SPAN_32767, 32767), (TRI_SPAN_33280, 33280)):
            case = sc.pixel_case([tri], 96)
            X, _, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], 96)
            assert int(X.max() - X.min()) == span and sc.rasterise(case)["coverage"].sum() > 100
        assert r["coverage"][:, 63].any() and r["coverage"][:, 64].any() and r["coverage"][64:, :].any() and r["coverage"].max() == 3
    elif name == "mesh200":
        assert all(1400 <= r["submitted"] <= 1600 for _, _, r in runs)
        assert len({r["map"].tobytes() for _, _, r in runs}) == 3
    elif name == "dense64":
        assert runs[0][2]["submitted"] == 20011 and 20011 % 64 != 0
        assert runs[0][2]["coverage"].max() >= 8
    else:
        r = runs[0][2]
        assert (r["coverage"] >= 1).all(), "the large triangle covers the whole map"
        assert (r["map"] == 0).any() and (r["map"] == 65535).any(), "depths below 0 and above 1 on covered texels"
        assert r["drawn"] == 3 and r["submitted"] == 4
        for sliver in SLIVERS:  # at most 5 / 8 of a pixel high at the left edge, tapering to 2 / 5 at the right: never two centres of a column, centres all the way across
            alone = sc.rasterise(sc.pixel_case([sliver], 130))["coverage"]
            columns = np.flatnonzero(alone.any(axis=0))
            assert alone.sum(axis=0).max() == 1 and columns.min() < 15 and columns.max() >= 115 and alone.sum() >= 40


def _check_draws700(runs):
    case, _, r = runs[0]
    counts = (case["draws"][:, 1] // 3).astype(np.int64)
    assert len(runs) == 2 and case["draws"].shape[0] == 700 and r["submitted"] == int(counts.sum()) and r["drawn"] > 2000
    assert not counts[:2].any() and not counts[-3:].any() and not counts[200:600].any() and not counts[256:512].any(), "an empty chunk of 256 draws"
    assert sorted(int(c) for c in set(counts.tolist())) == [0, 11, 12, 528] and set(case["draws"][list(DRAWS700_SHORT), 1].tolist()) == {34, 35}
    slots = case["draws"][:, 3]
    assert case["transforms"].shape[0] == DRAWS700_TRANSFORMS < 700 and int(slots.max()) == DRAWS700_TRANSFORMS - 1
    used = slots[counts > 0]
    assert len(set(used.tolist())) < used.size, "non-empty draws share a transform slot"
    assert int((slots == np.arange(700)).sum()) < 10, "transformIndex is not the draw's own number"
    draw_of = np.repeat(np.arange(700), counts)  # the draw of every triangle, in the set-up kernel's order
    per_block = [len(set(draw_of[b:b + 256].tolist())) for b in range(0, draw_of.size, 256)]
    assert max(per_block) >= 20 and min(per_block) == 1, "a set-up block that spans 20 draws and one inside a single draw"
    assert draw_of.size > 3 * 256 and draw_of.size % 256 != 0
    case, _, r = runs[1]
    counts = (case["draws"][:, 1] // 3).astype(np.int64)
    assert counts[256] > 0 and counts[:256].sum() > 0 and not counts[255] and not counts[257], "the first draw of the second chunk holds triangles behind earlier ones"
    alone = sc.rasterise(dict(case, draws=case["draws"][256:257]))
    assert r["submitted"] == int(counts.sum()) and r["drawn"] > 1000 and alone["drawn"] >= 4 and alone["map"].any()


def _check_nothing(runs):
    assert runs[0][0]["draws"].shape == (0, 4) and runs[0][0]["res"] == 72


def _check_small_maps(runs):
    assert [case["res"] for case, _, _ in runs] == list(SMALL_MAPS)
    for case, _, r in runs:
        res = case["res"]
        assert (r["coverage"] >= 1).all() and len(np.unique(r["map"])) >= min(res * res, 20), "the large triangle covers the map with a depth gradient"
        assert r["drawn"] == r["submitted"] == (1 if res < 7 else 4 if res == 65 else 3)
        if res >= 7:
            for tri in SMALL_TRIS:
                w, h, covered = _pixel_box(tri, res)
                assert w <= 4 and h <= 4 and covered > 0
            assert r["coverage"][:7, :7].max() >= 2
    alone = sc.rasterise(sc.pixel_case([TRI_ACROSS_64], 65))["coverage"]
    assert alone[:, 63].any() and alone[:, 64].any()


def _fan_spans(f):
    case = sc.pixel_case(fan(*f), 96)
    X, Y, _, _ = ref.project(case["light"], case["transforms"][0], case["positions"], 96)
    X, Y = X.reshape(8, 3), Y.reshape(8, 3)
    return np.maximum(X.max(axis=1) - X.min(axis=1), Y.max(axis=1) - Y.min(axis=1))


def _check_fans(runs):
    centres = np.arange(96) + 0.5
    for (case, _, r), fans in zip(runs, (FANS, (FAN_INT64,))):
        assert r["drawn"] == r["submitted"] == 8 * len(fans) and r["coverage"].max() == 1
        for cx, cy, radius in fans:
            inside = (np.abs(centres - cy) < radius)[:, None] & (np.abs(centres - cx) < radius)[None, :]
            assert inside.any() and (r["coverage"][inside] == 1).all(), "every centre strictly inside the outline belongs to exactly one triangle"
            alone = sc.rasterise(sc.pixel_case(fan(cx, cy, radius), 96))
            # a triangle owns texels: all eight do from r = 3 on; at r = 1.5 the nine centres inside lie on the eight rays and at most one triangle goes without
            assert len(np.unique(alone["map"][inside])) >= (8 if radius >= 3.0 else 7)
    assert all((_fan_spans(f) < 32768).all() for f in FANS) and (_fan_spans(FAN_INT64) == 38400).all()
    for f in FANS[:1] + FANS[2:]:
        assert all(_pixel_box(tri, 96)[0] <= 4 and _pixel_box(tri, 96)[1] <= 4 for tri in fan(*f)), "the lane path"
    assert all(max(_pixel_box(tri, 96)[:2]) > 4 for tri in fan(*FANS[1]))
    big = runs[1][2]["coverage"]
    assert big[0].all() and big[-1].all() and big[:, 0].all() and big[:, -1].all(), "clipped at all four map edges"


def _check_steep_huge(runs):
    case, _, r = runs[0]
    X, Y, _, inside = ref.project(case["light"], case["transforms"][0], case["positions"], 64)
    assert inside.all() and [(int(x), int(y)) for x, y in zip(X, Y)] == [(int(x * 256), int(y * 256)) for x, y in STEEP_HUGE]
    assert (r["coverage"] == 1).all() and r["map"].min() > 0 and r["map"].max() < 65535, "every texel covered, none clamped"
    assert len(np.unique(r["map"])) >= 3000
    assert np.array_equal(fragment_codes(case), r["map"]), "the emulation with the contract's own steps is the reference"
    for what, wrong in WRONG_FRAGMENTS.items():
        changed = int((fragment_codes(case, **wrong) != r["map"]).sum())
        print("steep_huge: %s changes %d of 4096 texels" % (what, changed))
        assert changed >= 500, "%s changes only %d texels: the input no longer discriminates" % (what, changed)


def _check_band_edges(runs):
    case, _, r = runs[0]
    clip = ref.transform(ref.mat_mul(case["light"], case["transforms"][0]), case["positions"])
    with np.errstate(all="ignore"):
        xf, yf = (clip[:, 0] * np.float32(0.5) + np.float32(0.5)) * np.float32(64), (clip[:, 1] * np.float32(0.5) + np.float32(0.5)) * np.float32(64)
    n = len(BAND_DRAWN)
    assert (xf[1], xf[3], yf[6], yf[11]) == (BAND_IN_HIGH, BAND_IN_LOW, BAND_IN_LOW, BAND_IN_HIGH)
    assert (xf[3 * n + 1], xf[3 * n + 3], yf[3 * n + 6], yf[3 * n + 11]) == (BAND, -BAND, -BAND, BAND)
    assert (case["positions"][1, 0], case["positions"][3 * n + 3, 0]) == (32767.0 - 1.0 / 512.0, -32769.0)
    assert r["submitted"] == 18 and r["drawn"] == 8
    for tris, drawn in ((BAND_DRAWN, True), (BAND_REJECTED, False)):
        for tri in tris:
            alone = sc.rasterise(sc.pixel_case([tri], 64))
            assert (alone["drawn"], alone["rejects"]) == ((1, 0) if drawn else (0, 1)) and (alone["coverage"].sum() > 20) == drawn
    assert (r["map"][40:46, 2:8] == 65535).any(), "z = 3.4e38 at a vertex is drawn and clamps"
    # the NaN depth: edge 2 -> 0 of NAN_DEPTH_TRI is column 20, rows 45 .. 59
    flat = int(np.rint(np.float32(0.25) * np.float32(65535.0)))
    rows = np.arange(45, 60)
    assert (r["coverage"][rows, 20] == 2).all() and (r["map"][rows, 20] == flat).all(), "zf is NaN on the left edge: code 0, the flat quad's code stays"
    assert (r["map"][rows, 21] == 65535).all() and (r["map"][rows, 19] == flat).all(), "+inf beside it"
    with np.errstate(all="ignore"):
        alone = sc.rasterise(sc.pixel_case([NAN_DEPTH_TRI], 64))
    assert (alone["coverage"][rows, 20] == 1).all() and not alone["map"][rows, 20].any() and (alone["map"][alone["coverage"] > 0] == 65535).sum() > 50


def _check_outside_buffers(runs):
    case, _, r = runs[0]
    v, n, t = case["positions"].shape[0], case["indices"].size, case["transforms"].shape[0]
    assert (r["submitted"], r["drawn"], r["rejects"]) == (16, 12, 4)
    d = case["draws"].astype(np.int64)
    assert int((d[:, 0] + d[:, 1]).max()) == n + 1, "one index slot past the end"
    assert max(int(case["indices"][f:f + c].max()) + o for f, c, o, _ in d.tolist()) == v, "one vertex past the end"
    assert int(d[:, 3].max()) == t, "one transform past the end"
    assert all(a.nbytes % 4096 != 0 for a in (case["positions"], case["indices"], case["transforms"], case["draws"]))
    inside = raw_case(64, case["positions"], case["indices"], [[0, 30, 0, 0], [30, 3, 30, 0], [42, 3, 0, 1]], case["transforms"])
    alone = sc.rasterise(inside)
    assert alone["rejects"] == 0 and alone["drawn"] == 12 and np.array_equal(alone["map"], r["map"]), "the rejected triangles draw nothing"
    assert r["coverage"].max() >= 2


NEW_CASE_CHECKS = {"draws700": _check_draws700, "nothing": _check_nothing, "small_maps": _check_small_maps, "fans": _check_fans, "steep_huge": _check_steep_huge,
                   "band_edges": _check_band_edges, "outside_buffers": _check_outside_buffers}


def prefill_pattern(res):
    """the bit pattern the map holds in front of an execution (the pass clears: an untouched texel would keep it)"""
    if res <= 4096:
        return ((np.arange(res * res, dtype=np.uint64) * 40503 + 0x1234) & 0xFFFF).astype(np.uint16)
    row = ((np.arange(res, dtype=np.uint64) * 40503 + 0x1234) & 0xFFFF).astype(np.uint16)  # one row's pattern, tiled: no 2 GB arange for the largest map
    return np.tile(row | np.uint16(1), res)


def gpu_raster(be, case, cascade):
    """one execution through the C-ABI with the test's own buffers -> (map, (submitted, drawn, rejects))"""
    res = case["res"]
    triangles = int(case["draws"][:, 1].sum()) // 3
    info = np.full(76, 7.25, np.float32)  # splits, 4 matrices, scales: anything but the cascade's own matrix is garbage
    info[4 + 16 * cascade:4 + 16 * (cascade + 1)] = case["light"]
    scratch_bytes = 64 + 16 * ((triangles + 3) // 4) + 80 * triangles
    prefill = prefill_pattern(res)
    buffers = [be.createStorageBuffer(304, info.tobytes())]
    for a in (case["transforms"], case["positions"], case["indices"], case["draws"]):
        b = np.ascontiguousarray(a).tobytes() or b"\xa5" * 64  # (the backend refuses a buffer of size 0: an execution without draws binds dummies)
        buffers.append(be.createStorageBuffer(len(b), b))
    buffers.append(be.createStorageBuffer(scratch_bytes, b"\xa5" * scratch_bytes))
    target = be.createImage(image_desc_2d(res, res, ImageFormat.Depth16), prefill)
    p = be.createComputePass("sunShadowRaster.comp", [spec_uint(0, cascade)], "Sun shadow cascade %d" % cascade)
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(target, 0, 0)], storageBuffers=[StorageBufferResource(b, i != 5, i) for i, b in enumerate(buffers)]),
        struct.pack("<2I", case["draws"].shape[0], triangles), (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
    out = be.downloadImage(target, 0, np.uint16).reshape(res, res).copy()
    header = be.downloadStorageBuffer(buffers[5], 16, dtype=np.uint32)
    assert int(header[0]) == int(header[2]), "the cursor counts the drawn triangles"
    return out, (int(header[1]), int(header[2]), int(header[3]))


@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_what_they_are_for(name):
    """not gpu: the input conditions of the GPU test"""
    check_case_is_what_it_is_for(name)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_shadow_raster_is_bit_identical_to_the_reference(backend, name, fast):
    check_case_is_what_it_is_for(name)
    backend.setMathMode(fast)
    try:
        for case, cascade, r in reference(name):
            out, counters = gpu_raster(backend, case, cascade)
            general = backend.getGeneralKernelExecutions()
            differing = int((out != r["map"]).sum())
            print("shadow raster %-8s cascade %d %-5s: %d of %d texels differ, counters %r (reference %r)"
                  % (name, cascade, "fast" if fast else "exact", differing, out.size, counters, (r["submitted"], r["drawn"], r["rejects"])))
            assert differing == 0, "%d texels differ from the reference, first at %r" % (differing, tuple(np.argwhere(out != r["map"])[0]))
            assert counters == (r["submitted"], r["drawn"], r["rejects"])
            if fast:
                assert general[0] == 0, "the fast set ran a general kernel: %r" % (general,)
    finally:
        backend.setMathMode(False)


LARGEST_MAP = 16384
LARGEST_MAP_TILES = (0, 127, 128, 255)  # a tile rectangle's bytes with the top bit clear, set, and all ones


def _largest_map():
    tris = [[(64.0 * tx + 10.5, 64.0 * ty + 40.25, 0.3 + 0.002 * tx), (64.0 * tx + 80.5, 64.0 * ty + 41.0, 0.5), (64.0 * tx + 30.25, 64.0 * ty + 70.5, 0.4 + 0.002 * ty)]
            for ty in LARGEST_MAP_TILES for tx in LARGEST_MAP_TILES]
    return sc.pixel_case(tris, LARGEST_MAP), 1


def check_largest_map_is_what_it_is_for():
    if "largest" not in _reference_cache:
        case, cascade = _largest_map()
        _reference_cache["largest"] = (case, cascade, sc.rasterise(case))
    case, cascade, r = _reference_cache["largest"]
    assert (r["submitted"], r["drawn"], r["rejects"]) == (16, 16, 0)
    for ty in LARGEST_MAP_TILES:
        for tx in LARGEST_MAP_TILES:  # every triangle starts in its tile and reaches the next one on both axes, where the map has one
            tile = r["coverage"][64 * ty:64 * ty + 64, 64 * tx:64 * tx + 64]
            assert tile.any() and (tx == 255 or r["coverage"][64 * ty:64 * ty + 64, 64 * tx + 64:64 * tx + 128].any())
            assert ty == 255 or r["coverage"][64 * ty + 64:64 * ty + 128, 64 * tx:64 * tx + 64].any()
    assert r["coverage"][:, LARGEST_MAP - 1].any() and r["coverage"][LARGEST_MAP - 1, :].any() and 10000 < int(r["coverage"].sum()) < 20000
    return case, cascade, r


def test_largest_map_case_is_what_it_is_for():
    """not gpu: the input conditions of the GPU test below"""
    check_largest_map_is_what_it_is_for()


@pytest.mark.gpu
def test_gpu_shadow_raster_reaches_the_largest_map(backend):
    """res 16384 = 256 tiles per axis, the most a 4-byte tile rectangle addresses; one math mode (both registrations are one function)"""
    import time
    case, cascade, r = check_largest_map_is_what_it_is_for()
    start = time.perf_counter()
    out, counters = gpu_raster(backend, case, cascade)
    seconds = time.perf_counter() - start
    differing = int((out != r["map"]).sum())
    print("shadow raster largest map %d: %d of %d texels differ, counters %r (reference %r), %.2f s for upload, pass and download"
          % (LARGEST_MAP, differing, out.size, counters, (r["submitted"], r["drawn"], r["rejects"]), seconds))
    assert differing == 0, "%d texels differ from the reference, first at %r" % (differing, tuple(np.argwhere(out != r["map"])[0]))
    assert counters == (r["submitted"], r["drawn"], r["rejects"])


@pytest.mark.gpu
def test_gpu_launcher_refuses_what_it_cannot_run(backend):
    """fails loudly: a scratch buffer too small for the triangle count, a map that is not Depth16"""
    from plainrenderer_amd.backend import PlrError
    case, cascade = _unit96()[0]
    small = dict(case)
    be = backend
    with pytest.raises(PlrError, match="scratch"):
        _run_with(be, small, cascade, scratch_bytes=64)
    with pytest.raises(PlrError, match="Depth16"):
        _run_with(be, small, cascade, fmt=ImageFormat.R16_sFloat)


def _run_with(be, case, cascade, scratch_bytes=None, fmt=ImageFormat.Depth16):
    res = case["res"]
    triangles = int(case["draws"][:, 1].sum()) // 3
    info = np.zeros(76, np.float32)
    buffers = [be.createStorageBuffer(304, info.tobytes())]
    for a in (case["transforms"], case["positions"], case["indices"], case["draws"]):
        b = np.ascontiguousarray(a).tobytes()
        buffers.append(be.createStorageBuffer(len(b), b))
    buffers.append(be.createStorageBuffer(scratch_bytes or 64 + 96 * triangles))
    target = be.createImage(image_desc_2d(res, res, fmt))
    p = be.createComputePass("sunShadowRaster.comp", [spec_uint(0, cascade)], "Sun shadow cascade refused")
    be.newFrame()
    be.setComputePassExecution(ComputePassExecution(p, RenderPassResources(
        storageImages=[ImageResource(target, 0, 0)], storageBuffers=[StorageBufferResource(b, i != 5, i) for i, b in enumerate(buffers)]),
        struct.pack("<2I", case["draws"].shape[0], triangles), (1, 1, 1)))
    be.prepareForDrawcallRecording()
    be.renderFrame()
