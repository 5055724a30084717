"""Inputs of the "debugGeometry.comp" tests (tests/test_debug_lines_cpu.py, tests/test_debug_lines.py): synthetic colour and depth images and named sets of
segments, each built once; callers must not modify one.

Lines are written in pixel coordinates under the identity viewProjection (w = 1: clip.xy = 2 p / size - 1, clip.z = the depth; the near plane is z = 1), so that a
case says what it covers; `perspective` runs the same clip under a camera. A case is a dict: width, height, view_projection (16 floats), color, depth (the images as
the pass finds them) and any of lines (n x 9), draws (d x 6), bounds (d x 6), transforms (n x 48), sdf_boxes (i x 8), draws_culled.

The depth image: 8 x 8 blocks alternate between sky (0) and geometry (0.05 .. 0.9), except a band of rows that is all 0.25 (`EQUAL_ROW`: the bit-equal test) and
a band that is all 0.8 (`NEAR_ROW`: nearer than most lines). Colour is a bit pattern no line colour equals.
"""
import numpy as np

import debug_lines_reference as ref

F32 = np.float32
IDENTITY = np.eye(4, dtype=F32).reshape(16)
SIZES = ((70, 37), (256, 144))  # ragged with an odd pitch; more than one chunk on both axes
STEP_COUNTS = (1, 63, 64, 65, 128, 129)
SEGMENT_COUNTS = (1, 63, 64, 65, 1000)
EQUAL_ROW, NEAR_ROW = 10, 20  # rows 10 .. 11 hold depth 0.25, rows 20 .. 21 depth 0.8
RED, GREEN, BLUE, WHITE = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.25, 4.0), (0.5, 0.5, 0.5)

_cache = {}


def images(width, height):
    key = ("images", width, height)
    if key not in _cache:
        rng = np.random.default_rng(0x4C494E45 + width)
        yy, xx = np.mgrid[0:height, 0:width]
        geometry = ((xx // 8) + (yy // 8)) % 2 == 1
        depth = np.where(geometry, rng.uniform(0.05, 0.9, (height, width)), 0.0).astype(F32)
        depth[EQUAL_ROW:EQUAL_ROW + 2] = F32(0.25)
        depth[NEAR_ROW:NEAR_ROW + 2] = F32(0.8)
        color = ((np.arange(width * height, dtype=np.uint64) * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF).astype(np.uint32).reshape(height, width)
        _cache[key] = (color, depth)
    return _cache[key]


def px(width, height, x0, y0, z0, x1, y1, z1, rgb=WHITE):
    """a line given in pixel coordinates and depths, as 9 floats under the identity viewProjection"""
    return [2.0 * x0 / width - 1.0, 2.0 * y0 / height - 1.0, z0, 2.0 * x1 / width - 1.0, 2.0 * y1 / height - 1.0, z1, *rgb]


def case(width, height, lines=None, view_projection=IDENTITY, **more):
    color, depth = images(width, height)
    out = dict(width=width, height=height, view_projection=np.asarray(view_projection, F32).reshape(16), color=color, depth=depth)
    if lines is not None:
        out["lines"] = np.asarray(lines, F32).reshape(-1, 9)
    out.update(more)
    return out


def step_lines(width, height):
    """x-major and y-major segments of 1, 63, 64, 65, 128 and 129 major steps (as far as the image reaches), each on rows / columns of its own, with a slope"""
    lines = []
    for k, n in enumerate(STEP_COUNTS):
        slope = min(0.5 * n, 2.5)
        lines.append(px(width, height, 3.25, 1.5 + 5.0 * k, 0.95, 3.25 + n, 1.5 + slope + 5.0 * k, 0.9, RED))         # x-major, n centres from column 3 on
        lines.append(px(width, height, 2.0 + slope + 9.0 * k, 2.25 + n, 0.93, 2.0 + 9.0 * k, 2.25, 0.97, GREEN))     # y-major, given bottom-up
    return lines


def random_lines(width, height, count):
    """the first `count` of one seeded sequence: ends up to a quarter of the frame outside it, depths on both sides of the near plane now and then"""
    key = ("random", width, height)
    if key not in _cache:
        rng = np.random.default_rng(0x52414E44 + width)
        n = max(SEGMENT_COUNTS)
        ends = rng.uniform(-0.25, 1.25, (n, 2, 2)) * (width, height)
        z = rng.uniform(0.02, 1.05, (n, 2))
        rgb = rng.uniform(0.0, 8.0, (n, 3))
        _cache[key] = [px(width, height, ends[k, 0, 0], ends[k, 0, 1], z[k, 0], ends[k, 1, 0], ends[k, 1, 1], z[k, 1], rgb[k]) for k in range(n)]
    return _cache[key][:count]


def through_one_pixel(width, height, count, equal_depths):
    """`count` short segments in all directions through the centre of pixel (33, 17)"""
    rng = np.random.default_rng(0x50495845)
    out = []
    for k in range(count):
        angle = np.pi * k / count
        dx, dy = 6.0 * np.cos(angle), 6.0 * np.sin(angle)
        z = 0.95 if equal_depths else 0.6 + 0.35 * float(rng.random())
        out.append(px(width, height, 33.5 - dx, 17.5 - dy, z, 33.5 + dx, 17.5 + dy, z, (k % 7, k % 5, k % 3)))
    return out


def box_case(width, height, odd=False, culled=False):
    """five draws of a unit box under models that put them into the identity view's clip volume, and two SDF boxes; `odd`: a NaN in one draw's model matrix and a
    transformIndex one past the end; `culled`: draw 1 has indexCount 0 and the record says the array is a culled copy"""
    bounds = np.tile(np.array([-1, -1, -1, 1, 1, 1], F32), (5, 1))
    bounds[2] = (-0.5, -2.0, -0.25, 1.5, 0.5, 0.75)
    transforms = np.zeros((5, 48), F32)
    draws = np.zeros((5, 6), np.uint32)
    for d in range(5):
        a = 0.4 * d
        m = np.eye(4)
        m[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.diag([0.12 + 0.03 * d, 0.2, 0.1])
        m[:3, 3] = (-0.7 + 0.35 * d, 0.1 * (d - 2), 0.5 + 0.08 * d)
        transforms[d, :16] = m.T.astype(F32).reshape(16)
        transforms[d, 16:] = 7.0  # mvp, mvpPrevious: not the pass's
        draws[d] = (3 * d, 36, 0, d, 0xFF0000FF, 0x80808080)
    sdf = np.array([[-0.9, -0.8, 0.3, 99.0, -0.4, -0.2, 0.6, 99.0], [0.2, 0.3, 0.1, 99.0, 1.4, 0.9, 0.2, 99.0]], F32)
    if odd:
        transforms[1, 5] = np.nan
        draws[3, 3] = 5
    if culled:
        draws[1, 1] = 0
    return case(width, height, draws=draws, bounds=bounds, transforms=transforms, sdf_boxes=sdf, draws_culled=culled,
                lines=[px(width, height, 1.0, 1.0, 0.99, width - 1.0, height - 1.0, 0.99, BLUE)])


def perspective_view(width, height):
    from prepass_raster_cases import camera
    return np.asarray(camera(aspect=width / height).view_projection((0.3 / width, -0.2 / height)), F32).reshape(16)


def perspective_lines():
    """world-space segments in front of a camera at the origin that looks down +z (near 0.1): inside, through the near plane, wholly behind the camera, with an end
    far outside the guard band, and a long one towards the horizon"""
    return [[-1.0, -0.5, 5.0, 1.0, 0.5, 7.0, *RED], [0.2, 0.1, 2.0, 0.1, -0.1, -3.0, *GREEN], [0.5, 0.5, -1.0, -0.5, 0.2, -4.0, *BLUE],
            [0.0, 0.3, 3.0, 400.0, 0.3, 3.0, *WHITE], [-2.0, 1.0, 1.0, 30.0, -4.0, 250.0, *GREEN], [0.0, 0.0, 0.05, 0.3, 0.2, 0.3, *RED]]


def named_cases(width, height):
    """[(name, case)] - the pass-level cases of one frame size"""
    key = ("named", width, height)
    if key in _cache:
        return _cache[key]
    W, H = float(width), float(height)
    out = [("steps", case(width, height, step_lines(width, height))),
           ("diagonal", case(width, height, [px(width, height, 0.0, 0.0, 0.9, W, H, 0.99, BLUE), px(width, height, W, 0.0, 0.99, 0.0, H, 0.9, RED)])),
           ("off each side", case(width, height, [
               px(width, height, -20.0, 5.3, 0.95, 12.0, 8.1, 0.95), px(width, height, W - 9.0, 3.0, 0.95, W + 30.0, 6.0, 0.95),        # partly off left, right
               px(width, height, 14.2, -15.0, 0.95, 16.9, 9.0, 0.95), px(width, height, 30.0, H - 4.0, 0.95, 27.0, H + 40.0, 0.95),     # partly off top, bottom
               px(width, height, -30.0, 5.0, 0.95, -2.0, 9.0, 0.95), px(width, height, W + 1.0, 5.0, 0.95, W + 25.0, 9.0, 0.95),        # wholly off left, right
               px(width, height, 5.0, -9.0, 0.95, 40.0, -0.6, 0.95), px(width, height, 5.0, H + 0.6, 0.95, 40.0, H + 7.0, 0.95),        # wholly off top, bottom: drawn, no fragment
               px(width, height, 10.0, 10.0, 0.95, 40.0 * W, 12.0, 0.95), px(width, height, 5.0, 5.0, 0.5, 20.0, 8.0, 1.5),             # past the guard band; through the near plane
               px(width, height, 5.0, 5.0, 1.5, 20.0, 8.0, 1.2)])),                                                                   # wholly in front of the near plane
           ("zero length", case(width, height, [px(width, height, 12.5, 7.5, 0.9, 12.5, 7.5, 0.9), px(width, height, 12.6, 7.4, 0.9, 12.9, 7.45, 0.9)])),
           ("depth test", case(width, height, [
               px(width, height, 2.0, NEAR_ROW + 0.5, 0.5, 60.0, NEAR_ROW + 0.5, 0.5, RED),          # hidden behind the 0.8 band
               px(width, height, 2.0, EQUAL_ROW + 0.5, 0.25, 60.0, EQUAL_ROW + 0.5, 0.25, GREEN),    # bit-equal to the 0.25 band: GreaterEqual lets it pass
               px(width, height, 2.0, EQUAL_ROW + 1.5, 0.2, 60.0, EQUAL_ROW + 1.5, 0.3, BLUE),       # crosses the band's depth half way
               px(width, height, 1.0, 30.5, 0.001, 65.0, 33.0, 0.002, WHITE)])),                     # over sky and geometry blocks, far away
           ("crossing at equal depth", case(width, height, [px(width, height, 20.0, 2.0, 0.96, 40.0, 9.0, 0.96, RED), px(width, height, 20.0, 9.0, 0.96, 40.0, 2.0, 0.96, GREEN)])),
           ("300 through one pixel, distinct depths", case(width, height, through_one_pixel(width, height, 300, False))),
           ("300 through one pixel, equal depths", case(width, height, through_one_pixel(width, height, 300, True))),
           ("boxes", box_case(width, height)), ("boxes, odd inputs", box_case(width, height, odd=True)), ("boxes, culled copy", box_case(width, height, culled=True)),
           ("perspective", case(width, height, perspective_lines(), perspective_view(width, height)))]
    out += [("%d segments" % n, case(width, height, random_lines(width, height, n))) for n in SEGMENT_COUNTS]
    _cache[key] = out
    return out


def reference(width, height, name):
    """(color, depth, stats, details) of a named case, computed once"""
    key = ("reference", width, height, name)
    if key not in _cache:
        c = dict(named_cases(width, height))[name]
        _cache[key] = draw(c, details=True)
    return _cache[key]


def draw(c, details=False):
    return ref.draw(c["color"], c["depth"], c["view_projection"], c.get("draws"), c.get("bounds"), c.get("transforms"), c.get("sdf_boxes"), c.get("lines"),
                    c.get("draws_culled", False), details=details)
