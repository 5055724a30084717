"""Inputs of the "drawCulling.comp" tests (tests/test_draw_culling_cpu.py, tests/test_draw_culling.py, tests/test_draw_culling_frame.py): small meshes of one to
twelve triangles under a perspective camera (the main view) and under an affine light matrix (a shadow view), each case built once; callers must not modify one.

A draw is placed by the clip coordinates its model origin should get: `main_at(depth, u, v)` is the world point with w = depth and x / w = u, y / w = v under
CAMERA; `shadow_at(u, v, z)` the world point with clip (u, v, z) under LIGHT. Which plane a named draw is culled by - or that it is kept - is asserted on the
reference by tests/test_draw_culling_cpu.py, not assumed here.

Named draws, the same names in both views unless marked (M: main view only):
  in_view            a box in the middle of the view (kept)
  culled_near (M)    a small box between the camera and the near plane;  behind_camera (M)  a box wholly behind the camera (both: the near plane)
  culled_+x, culled_-x, culled_+y, culled_-y      a box outside that plane and inside the others that come before it in the order
  straddles_near (M), straddles_+x .. straddles_-y  a box with the plane through it (kept)
  within_tolerance   a triangle whose three vertices coincide - its box is a point, g is one number - outside +x by about a third of the tolerance (kept)
  contains_camera (M)  a box around the camera (kept);  around_map (shadow)  a box around the whole map
  across_corner      a thin box turned 45 degrees about the view axis beside the +x +y corner: outside the view, outside no single plane (kept)
  rotated_in, rotated_out   the twelve-triangle box rotated and non-uniformly scaled, in view and out of it
  empty              a draw with indexCount 0, in view
  in_front_of_range, behind_range (shadow)   boxes inside the map's x and y with clip z = -3 and 5: there is no depth plane (kept)
  short              a box draw with indexCount 2: fewer than three indices (tested like any other; it lies outside +y)
Behind the named draws a seeded random fill follows, so that a case of n draws is the first n of one sequence: n = 1, 63, 64, 65, 257, 600 cross wave and block edges.
"""
import numpy as np

import draw_culling_reference as cull_ref
import prepass_raster_cases as pc
import shadow_raster_reference as shadow_ref

F32 = np.float32
WIDTH, HEIGHT, SHADOW_RES = 192, 128, 256
DRAW_COUNTS = (1, 63, 64, 65, 257, 600)
CAMERA = dict(position=(0.0, 0.0, 0.0), forward=(0.0, 0.0, 1.0), aspect=WIDTH / HEIGHT, near=0.1, far=300.0, fov=35.0)
MESH_BOX, MESH_QUAD, MESH_TRIANGLE, MESH_EMPTY, MESH_POINT = range(5)

_cache = {}


def meshes():
    """[(positions n x 3, indices)]: a box of 12 triangles, a quad of 2, a triangle, a mesh without indices, a triangle whose three vertices coincide"""
    if "meshes" not in _cache:
        from plainrenderer_amd import meshes as m
        box = m.box((1.0, 1.0, 1.0), subdiv=1)
        quad = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F32), np.array([0, 2, 1, 0, 3, 2], np.uint32))
        triangle = (np.array([[-1, -0.5, 0.25], [1, -0.5, -0.25], [0, 1, 0]], F32), np.array([0, 2, 1], np.uint32))
        empty = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.zeros(0, np.uint32))
        point = (np.zeros((3, 3), F32), np.array([0, 1, 2], np.uint32))
        out = [(np.asarray(p, F32).reshape(-1, 3), np.asarray(i, np.uint32).reshape(-1)) for p, i in (box, quad, triangle, empty, point)]
        assert [i.size // 3 for _, i in out] == [12, 2, 1, 0, 1]
        _cache["meshes"] = out
    return _cache["meshes"]


def model(scale=(1.0, 1.0, 1.0), yaw=0.0, pitch=0.0, roll=0.0, translate=(0.0, 0.0, 0.0)):
    """translate * rotateY(yaw) * rotateX(pitch) * rotateZ(roll) * scale as 16 floats, column-major"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ rz @ np.diag(np.asarray(scale, np.float64))
    m[:3, 3] = translate
    return pc.glm(m)


def camera():
    return pc.camera(**CAMERA)


def view_projection(cam=None, jitter=(0.0, 0.0)):
    return np.asarray((cam or camera()).view_projection(jitter), F32).reshape(16)


def _math(m16):
    """16 floats column-major -> 4 x 4 float64 math matrix"""
    return np.asarray(m16, np.float64).reshape(4, 4).T


def main_at(depth, u, v, cam=None):
    """the world point whose clip coordinates under the camera have w = depth, x / w = u, y / w = v (float64)"""
    vp = _math(view_projection(cam))
    # rows x, y, w of the view projection are linear in the world point: solve the three equations
    a = np.array([vp[0, :3] - u * vp[3, :3], vp[1, :3] - v * vp[3, :3], vp[3, :3]])
    b = np.array([u * vp[3, 3] - vp[0, 3], v * vp[3, 3] - vp[1, 3], depth - vp[3, 3]])
    return np.linalg.solve(a, b)


LIGHT = model((1.0 / 20.0, 1.0 / 16.0, 1.0 / 60.0), 0.5, -0.9, 0.2, (0.1, -0.05, 0.5))


def shadow_at(u, v, z, light=None):
    """the world point whose clip coordinates under the light are (u, v, z) (float64)"""
    return np.linalg.solve(_math(LIGHT if light is None else light), np.array([u, v, z, 1.0]))[:3]


def _named(at, main):
    """[(name, mesh, model)] for one view; at(u, v, along): the world point at clip (u, v) and depth `along` (main: w; shadow: z scaled to a comparable range)"""
    s = 0.4 if main else 1.2  # box scale: small against the view at its distance
    quarter = np.pi / 4.0
    out = [("in_view", MESH_BOX, model((s, s, s), 0.3, 0.2, 0.0, at(0.1, -0.2, 10.0)))]
    if main:
        out += [("culled_near", MESH_BOX, model((0.01, 0.01, 0.01), 0.0, 0.0, 0.0, at(0.0, 0.0, 0.05))),
                ("behind_camera", MESH_BOX, model((s, s, s), 0.4, 0.1, 0.0, at(0.2, 0.1, -6.0))),
                ("straddles_near", MESH_BOX, model((0.05, 0.05, 0.05), 0.0, 0.0, 0.0, at(0.0, 0.0, 0.1))),
                ("contains_camera", MESH_BOX, model((40.0, 40.0, 40.0), 0.2, 0.1, 0.0, at(0.0, 0.0, 1.0)))]
    else:
        out += [("around_map", MESH_BOX, model((60.0, 60.0, 60.0), 0.2, 0.1, 0.0, at(0.0, 0.0, 10.0))),
                ("in_front_of_range", MESH_BOX, model((s, s, s), 0.0, 0.0, 0.0, at(0.3, 0.3, -200.0))),
                ("behind_range", MESH_BOX, model((s, s, s), 0.0, 0.0, 0.0, at(-0.3, 0.2, 300.0)))]
    for name, u, v in (("+x", 1.5, 0.2), ("-x", -1.5, -0.1), ("+y", 0.3, 1.5), ("-y", -0.2, -1.5)):
        out.append(("culled_" + name, MESH_BOX, model((s, s, s), 0.3, 0.5, 0.1, at(u, v, 10.0))))
        out.append(("straddles_" + name, MESH_QUAD if name[1] == "x" else MESH_BOX, model((s, s, s), 0.2, 0.3, 0.0, at(u / 1.5, v, 10.0) if name[1] == "x" else at(u, v / 1.5, 10.0))))
    out += [("within_tolerance", MESH_POINT, model(translate=at(1.0 + 1e-5, 0.0, 10.0))),
            ("across_corner", MESH_BOX, model((0.28 * 10.0 * _extent(main, 0), 0.28 * 10.0 * _extent(main, 1), 0.01), 0.0, 0.0, quarter, at(1.25, 1.25, 10.0))),
            ("rotated_in", MESH_BOX, model((1.5 * s, 0.6 * s, 1.1 * s), -0.4, 0.9, 0.3, at(-0.3, 0.3, 14.0))),
            ("rotated_out", MESH_BOX, model((1.5 * s, 0.6 * s, 1.1 * s), 1.1, -0.7, 0.5, at(-1.7, 0.4, 14.0))),
            ("empty", MESH_EMPTY, model(translate=at(0.0, 0.1, 8.0))),
            ("short", MESH_BOX, model((s, s, s), 0.0, 0.0, 0.0, at(0.0, 1.6, 9.0)))]
    return out


def _extent(main, axis):
    """world units per clip unit at depth 10 along the view's x (0) or y (1) axis, roughly: what scales `across_corner` so that its diamond has a half-diagonal of
    about 0.4 clip units"""
    if main:
        return abs(np.linalg.norm(main_at(1.0, 1.0 if axis == 0 else 0.0, 1.0 if axis == 1 else 0.0) - main_at(1.0, 0.0, 0.0)))
    return abs(np.linalg.norm(shadow_at(1.0 if axis == 0 else 0.0, 1.0 if axis == 1 else 0.0, 0.5) - shadow_at(0.0, 0.0, 0.5))) / 10.0


def _fill(rng, at, main, count):
    """seeded random draws: about two fifths in view"""
    s = 0.4 if main else 1.2
    out = []
    for _ in range(count):
        u, v = rng.uniform(-1.7, 1.7, 2)
        along = rng.uniform(-4.0, 40.0) if main else rng.uniform(-20.0, 80.0)
        scale = s * rng.uniform(0.4, 2.0, 3) * (max(along, 2.0) / 10.0 if main else 1.0)
        out.append((int(rng.choice([MESH_BOX, MESH_BOX, MESH_QUAD, MESH_TRIANGLE, MESH_EMPTY], p=[0.35, 0.35, 0.15, 0.1, 0.05])),
                    model(scale, rng.uniform(0, 6.28), rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), at(u, v, along))))
    return out


def _sequence(main):
    key = "sequence_main" if main else "sequence_shadow"
    if key not in _cache:
        at = (lambda u, v, along: main_at(along, u, v)) if main else (lambda u, v, along: shadow_at(u, v, along / 60.0 + 0.3))
        named = _named(at, main)
        rng = np.random.default_rng(0x43554C4C if main else 0x43554C53)
        draws = [(m, t) for _, m, t in named] + _fill(rng, at, main, max(DRAW_COUNTS) - len(named))
        _cache[key] = (draws, {name: k for k, (name, _, _) in enumerate(named)})
    return _cache[key]


def draw_list(main, count):
    """([(mesh, 16 floats)] * count, {name: draw number} of the named draws among them)"""
    draws, names = _sequence(main)
    return draws[:count], {n: k for n, k in names.items() if k < count}


def main_case(count, cam=None, jitter=(0.0, 0.0), draws=None):
    """a prepass case (tests/prepass_raster_cases.py) of the first `count` draws - or of `draws` - plus bounds (d x 6), names, draw_list"""
    key = ("main", count)
    if draws is None and cam is None and jitter == (0.0, 0.0) and key in _cache:
        return _cache[key]
    dl, names = draw_list(True, count) if draws is None else (draws, {})
    ms = [(p, None, i) for p, i in meshes()]
    case = pc.perspective_case(WIDTH, HEIGHT, ms, dl, cam or camera(), jitter_current=jitter, jitter_previous=jitter)
    if "short" in names:
        case["draws"][names["short"], 1] = 2
    case.update(bounds=cull_ref.draw_bounds([p for p, _ in meshes()], [m for m, _ in dl]), names=names, draw_list=dl)
    if draws is None and cam is None and jitter == (0.0, 0.0):
        _cache[key] = case
    return case


def shadow_case(count, light=None, draws=None):
    """a shadow case (tests/shadow_raster_cases.py: res, light, transforms, positions, indices, draws d x 4) plus bounds, names, draw_list"""
    key = ("shadow", count)
    if draws is None and light is None and key in _cache:
        return _cache[key]
    dl, names = draw_list(False, count) if draws is None else (draws, {})
    pos, idx, dr, tr = shadow_ref.merge_meshes(meshes(), dl)
    if "short" in names:
        dr[names["short"], 1] = 2
    case = dict(res=SHADOW_RES, light=np.asarray(LIGHT if light is None else light, F32).reshape(16).copy(), transforms=tr, positions=pos, indices=idx, draws=dr,
                bounds=cull_ref.draw_bounds([p for p, _ in meshes()], [m for m, _ in dl]), names=names, draw_list=dl)
    if draws is None and light is None:
        _cache[key] = case
    return case


ODD_INPUTS = ("transform_out_of_range", "nan_bound", "inf_bound", "nan_matrix", "inf_matrix")


def with_odd_inputs(case, main):
    """pass level only: a copy of the case with five more draws, each a copy of culled_+x - which the pass culls - with one odd input, so that keeping it is what
    shows: a transformIndex equal to the transform count, a NaN and an infinity in a bound, a NaN and an infinity in the draw's own matrix"""
    k = case["names"]["culled_+x"]
    out = dict(case)
    d0, n0 = case["draws"].shape[0], case["transforms"].shape[0]
    draws = np.concatenate([case["draws"], np.repeat(case["draws"][k:k + 1], 5, axis=0)])
    bounds = np.concatenate([case["bounds"], np.repeat(case["bounds"][k:k + 1], 5, axis=0)])
    own = case["transforms"][case["draws"][k, 3]]
    transforms = np.concatenate([case["transforms"], np.repeat(own[None, :], 2, axis=0)])
    draws[d0, 3] = n0 + 2  # one past the end
    bounds[d0 + 1, 1] = np.nan
    bounds[d0 + 2, 3] = np.inf
    draws[d0 + 3, 3] = n0
    transforms[n0, (16 if main else 0) + 12] = np.nan  # the translation's x: the matrix's own for a shadow view, mvp's for the main view
    draws[d0 + 4, 3] = n0 + 1
    transforms[n0 + 1, (16 if main else 0) + 5] = np.inf
    out.update(draws=draws, bounds=bounds, transforms=transforms, names=dict(case["names"], **{name: d0 + i for i, name in enumerate(ODD_INPUTS)}))
    return out


def cull(case, main):
    if main:
        return cull_ref.cull_main(case["draws"], case["bounds"], case["transforms"])
    return cull_ref.cull_shadow(case["draws"], case["bounds"], case["transforms"], case["light"])


def corner_g(case, main, draw, plane):
    """float64: g of `plane` at the eight corners of the draw's box under the case's own fp32 matrix, and the contract's tolerance from the same numbers"""
    lo, hi = case["bounds"][draw, :3].astype(np.float64), case["bounds"][draw, 3:].astype(np.float64)
    t = case["transforms"][case["draws"][draw, 3]]
    m = _math(t[16:32]) if main else _math(case["light"]) @ _math(t)
    comp = (2, 0, 0, 1, 1)[plane]
    sign = -1.0 if plane in (2, 4) else 1.0
    g = []
    for k in range(8):
        p = np.array([hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2], 1.0])
        c = m @ p
        g.append(sign * c[comp] - (c[3] if main else 1.0))
    a = np.maximum(np.abs(lo), np.abs(hi))
    S = np.abs(m[:, :3]) @ a + np.abs(m[:, 3])
    return np.array(g), 2.0 ** -16 * (S[comp] + (S[3] if main else 1.0))
