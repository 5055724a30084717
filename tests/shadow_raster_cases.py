"""Inputs of the "sunShadowRaster.comp" tests (tests/test_shadow_raster.py, tests/test_shadow_frame.py, tools/shadow_raster_cost.py): hand-made triangles in
pixel coordinates and the mesh scene, each built once.

Hand-made triangles are given in pixels of the map, vertices on multiples of 1 / 256 pixel, under identity light and model matrices. A position is the float32
nearest to 2 p / res - 1; within a few hundred pixels of the map what the viewport transform makes of it is within 1e-4 pixels of p (a float32 below 8
carries 5e-7, times res / 2), far inside the 1 / 512 pixel that snapping forgives, so the snapped vertex IS 256 p; a vertex further out is given where
2 p / res - 1 is a float32. `pixel_case` asserts the snapped positions on the reference's own projection.
A triangle (a, b, c) with a -> b pointing right and b -> c pointing down has A > 0: it is a back face and is drawn.
"""
import numpy as np

import shadow_raster_reference as ref

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def glm(m):
    """4 x 4 math matrix -> 16 floats, column-major"""
    return np.asarray(m, np.float64).T.astype(np.float32).reshape(16)


def pixel_case(triangles, res):
    """triangles: n x 3 x 3 (x, y in pixels, z) -> dict of the pass' inputs, one draw, identity matrices"""
    t = np.asarray(triangles, np.float64).reshape(-1, 3, 3)
    assert np.array_equal(t[..., :2] * 256, np.rint(t[..., :2] * 256)), "vertices lie on the sub-pixel grid"
    pos = t.reshape(-1, 3).copy()
    pos[:, :2] = 2.0 * pos[:, :2] / res - 1.0
    pos = pos.astype(np.float32)
    X, Y, _, inside = ref.project(IDENTITY, IDENTITY, pos, res)
    want = np.rint(t.reshape(-1, 3)[:, :2] * 256).astype(np.int64)
    assert np.array_equal(X[inside], want[inside, 0]) and np.array_equal(Y[inside], want[inside, 1]), "a vertex did not snap to the position it was given"
    idx = np.arange(pos.shape[0], dtype=np.uint32)
    return dict(res=res, light=IDENTITY.copy(), transforms=IDENTITY.reshape(1, 16).copy(), positions=pos, indices=idx,
                draws=np.array([[0, idx.size, 0, 0]], np.uint32))


def quad(x0, y0, x1, y1, z_upper, z_lower):
    """the rectangle as two back faces split along the diagonal (x0, y0) -> (x1, y1): the upper-right half at z_upper, the lower-left half at z_lower"""
    return [[(x0, y0, z_upper), (x1, y0, z_upper), (x1, y1, z_upper)], [(x0, y0, z_lower), (x1, y1, z_lower), (x0, y1, z_lower)]]


def flipped(mesh):
    """the mesh with every triangle's winding reversed. plainrenderer_amd.meshes emits triangles clockwise seen from outside; under the light matrices of
    lightMatrix.comp (SynthScene.shadow_cascades) those face front where they face the light, so the pass draws a closed mesh's far side - and the near side
    of the flipped mesh"""
    pos, idx = mesh
    return np.asarray(pos, np.float32), np.asarray(idx, np.uint32).reshape(-1, 3)[:, [0, 2, 1]].reshape(-1).copy()


def as_arrays(mesh):
    return np.asarray(mesh[0], np.float32), np.asarray(mesh[1], np.uint32).reshape(-1)


def affine(scale, yaw, pitch, translate):
    """translate * rotateY(yaw) * rotateX(pitch) * scale(sx, sy, sz) as 16 floats, column-major"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx @ np.diag(np.asarray(scale, np.float64))
    m[:3, 3] = translate
    return glm(m)


_cache = {}


def mesh_scene():
    """mesh200's scene: box, uv_sphere and torus as plainrenderer_amd.meshes emits them, under three affine transforms, one with non-uniform scale, in front of the smoke frame's
    camera, and the sunShadowInfo block SynthScene.shadow_cascades fits to that camera. Built once; callers must not modify it."""
    if "scene" not in _cache:
        from plainrenderer_amd import meshes, synth
        from plainrenderer_amd.scene import Camera
        cam = Camera.look((15.0, -7.0, -6.0), (0.0, 0.16, 1.0), aspect=96 / 54)
        sun = np.asarray((0.35, -0.8, 0.45), np.float64)
        sun /= np.linalg.norm(sun)
        scene = synth.SynthScene(grid=4, cell=8.0, seed_id=600)
        info, _ = scene.shadow_cascades(cam, sun, 2.0, 40.0, 16, cascade_count=3)  # (the matrices do not depend on the resolution the maps are marched at)
        ms = [as_arrays(meshes.box((1.0, 1.5, 0.75), subdiv=4)), as_arrays(meshes.uv_sphere(1.25, segments=28, rings=14)),
              as_arrays(meshes.torus(1.5, 0.5, segments=24, sides=12))]
        fwd, pos = np.asarray(cam.forward, np.float64), np.asarray(cam.position, np.float64)
        right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)
        draws = [(0, affine((1.0, 1.0, 1.0), 0.6, 0.25, pos + 6.0 * fwd - 1.5 * right)),
                 (1, affine((1.5, 0.6, 1.1), -0.4, 0.9, pos + 9.0 * fwd + 2.0 * right + 0.5 * up)),
                 (2, affine((1.2, 1.2, 1.2), 1.1, -0.7, pos + 14.0 * fwd + 0.5 * right - 1.0 * up))]
        _cache["scene"] = dict(meshes=ms, draws=draws, info=bytes(info), cam=cam, sun=sun, synth=scene)
    return _cache["scene"]


def mesh_case(light_matrix, res, draws=None):
    s = mesh_scene()
    pos, idx, dr, tr = ref.merge_meshes(s["meshes"], draws if draws is not None else s["draws"])
    return dict(res=res, light=np.asarray(light_matrix, np.float32).reshape(16).copy(), transforms=tr, positions=pos, indices=idx, draws=dr)


def rasterise(case):
    return ref.rasterise(case["light"], case["transforms"], case["positions"], case["indices"], case["draws"], case["res"])
