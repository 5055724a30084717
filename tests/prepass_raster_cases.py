"""Inputs of the "depthPrepassRaster.comp" tests (tests/test_prepass_raster.py, tests/test_prepass_frame.py, tests/test_prepass_raster_cpu.py,
tools/prepass_raster_cost.py): hand-made triangles in pixel coordinates, perspective scenes and the shadow test's cases converted, each built once.

A case is a dict of the pass' inputs: width, height, transforms (n x 48), positions, normals, indices, draws (d x 6), jitter_current, jitter_previous.

Winding. The pass draws A < 0 (cull mode Back, counter-clockwise front face). Hand-made triangles are written the way tests/shadow_raster_cases.py writes them -
(a, b, c) with a -> b pointing right and b -> c pointing down, A > 0 - and `pixel_case` reverses every triangle's vertex order unless told not to; a triangle
given with keep_winding is therefore a back face here. plainrenderer_amd.meshes emits triangles clockwise seen from outside, which under
projectionMatrixFromCameraIntrinsic (it carries Vulkan's Y flip) has A < 0 on the screen: the outside of those meshes is the DRAWN side (asserted in
tests/test_prepass_raster_cpu.py on a sphere: the near hemisphere wins), and the contract's face normal cross(v0 - v2, v0 - v1) points outward. `mesh_arrays`
therefore takes them as they are; `reversed_winding` serves the shadow tests' cases, which are built for a pass that draws A > 0. There is no winding option.
"""
import numpy as np

import prepass_raster_reference as ref

F32 = np.float32
IDENTITY = np.eye(4, dtype=F32).reshape(16)


def glm(m):
    """4 x 4 math matrix -> 16 floats, column-major"""
    return np.asarray(m, np.float64).T.astype(F32).reshape(16)


def reversed_winding(indices):
    """every whole triple (i0, i1, i2) of the index list becomes (i0, i2, i1); a tail of one or two indices stays"""
    idx = np.asarray(indices, np.uint32).reshape(-1).copy()
    n = idx.size // 3 * 3
    idx[:n] = idx[:n].reshape(-1, 3)[:, [0, 2, 1]].reshape(-1)
    return idx


def material(d):
    """two distinct RGBA8 words per draw number"""
    return (0xFF000000 | ((d * 2654435761) & 0xFFFFFF)) & 0xFFFFFFFF, (0x80000000 | ((d * 40503 + 0x1234) & 0xFFFFFF)) & 0xFFFFFFFF


def draws6(draws4):
    d = np.asarray(draws4, np.uint32).reshape(-1, 4)
    return np.array([list(row) + list(material(k)) for k, row in enumerate(d.tolist())], np.uint32).reshape(-1, 6)


def make_case(width, height, transforms, positions, indices, draws, normals=None, jitter_current=(0.0, 0.0), jitter_previous=(0.0, 0.0)):
    positions = np.asarray(positions, F32).reshape(-1, 3)
    normals = np.zeros_like(positions) if normals is None else np.asarray(normals, F32).reshape(-1, 3)
    draws = np.asarray(draws, np.uint32)
    draws = draws6(draws) if draws.reshape(-1).size and draws.shape[-1] == 4 else draws.reshape(-1, 6)
    return dict(width=int(width), height=int(height), transforms=np.asarray(transforms, F32).reshape(-1, 48), positions=positions, normals=normals,
                indices=np.asarray(indices, np.uint32).reshape(-1), draws=draws, jitter_current=tuple(float(F32(v)) for v in jitter_current),
                jitter_previous=tuple(float(F32(v)) for v in jitter_previous))


def rasterise(case, diagnostics=False):
    return ref.rasterise(case["transforms"], case["positions"], case["normals"], case["indices"], case["draws"], case["width"], case["height"],
                         case["jitter_current"], case["jitter_previous"], diagnostics=diagnostics)


def identity_matrices(count=1, previous=None):
    """{model, mvp, mvpPrevious} = identity (w = 1); `previous`: another mvpPrevious"""
    m = np.tile(np.concatenate([IDENTITY, IDENTITY, IDENTITY if previous is None else np.asarray(previous, F32).reshape(16)]), (count, 1))
    return m.astype(F32)


def pixel_case(groups, width, height, keep_winding=(), previous=None):
    """groups: one list of triangles (x, y in pixels on the sub-pixel grid, z = depth) per draw, under identity matrices. Triangles are given in the shadow
    cases' orientation and reversed (module docstring); keep_winding: numbers (over all groups) of triangles that keep theirs"""
    pos, draws, first = [], [], 0
    number = 0
    for group in groups:
        t = np.asarray(group, np.float64).reshape(-1, 3, 3).copy()
        assert np.array_equal(t[..., :2] * 256, np.rint(t[..., :2] * 256)), "vertices lie on the sub-pixel grid"
        for k in range(t.shape[0]):
            if number not in keep_winding:
                t[k] = t[k][[0, 2, 1]]
            number += 1
        pos.append(t.reshape(-1, 3))
        draws.append([first, 3 * t.shape[0], 0, 0])
        first += 3 * t.shape[0]
    want = np.concatenate(pos) if pos else np.zeros((0, 3))
    p = want.copy()
    p[:, 0] = 2.0 * p[:, 0] / width - 1.0
    p[:, 1] = 2.0 * p[:, 1] / height - 1.0
    p = p.astype(F32)
    clip = np.concatenate([p, np.ones((p.shape[0], 1), F32)], axis=1)
    X, Y, _, ok = ref.project(clip, width, height)
    near = np.abs(p[:, :2]).max(axis=1) < 32.0 if p.size else np.zeros(0, bool)
    snapped = np.rint(want[:, :2] * 256).astype(np.int64)
    assert np.array_equal(X[ok & near], snapped[ok & near, 0]) and np.array_equal(Y[ok & near], snapped[ok & near, 1]), "a vertex did not snap to the position it was given"
    return make_case(width, height, identity_matrices(1, previous), p, np.arange(p.shape[0]), np.asarray(draws, np.uint32).reshape(-1, 4))


def from_shadow_case(case):
    """a case of tests/shadow_raster_cases.py / test_shadow_raster.py as a prepass case: mvp = light * model (orthographic, w = 1), every triangle's index order
    reversed so that what the shadow pass draws (A > 0) faces front here"""
    from shadow_raster_reference import mat_mul
    transforms = np.asarray(case["transforms"], F32).reshape(-1, 16)
    t48 = np.stack([np.concatenate([t, mat_mul(case["light"], t), mat_mul(case["light"], t)]) for t in transforms]) if transforms.size else np.zeros((0, 48), F32)
    return make_case(case["res"], case["res"], t48, case["positions"], reversed_winding(case["indices"]), case["draws"])


def vertex_normals(positions, indices):
    """area-weighted vertex normals in the contract's face-normal sense, cross(v0 - v2, v0 - v1); float32"""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    c = np.cross(p[tri[:, 0]] - p[tri[:, 2]], p[tri[:, 0]] - p[tri[:, 1]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, tri[:, k], c)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return (n / np.where(length > 0, length, 1.0)).astype(F32)


def mesh_arrays(mesh, with_normals):
    """a plainrenderer_amd.meshes mesh as (positions, normals or None, indices), winding as emitted (module docstring)"""
    pos = np.asarray(mesh[0], F32).reshape(-1, 3)
    idx = np.asarray(mesh[1], np.uint32).reshape(-1)
    return pos, (vertex_normals(pos, idx) if with_normals else None), idx


def merge_meshes(meshes, draw_list):
    """meshes: [(positions, normals or None, indices)], draw_list: [(mesh, 16 floats)] -> positions, normals, indices, draws (d x 6), models (d x 16), laid out
    the way plrf_set_scene_meshes lays them out: meshes back to back, zeros for absent normals, one transform per draw, the draw's material from `material`"""
    first, base, pos, nrm, idx = [], [], [], [], []
    nv = ni = 0
    for p, n, i in meshes:
        p = np.asarray(p, F32).reshape(-1, 3)
        i = np.asarray(i, np.uint32).reshape(-1)
        first.append(ni); base.append(nv)
        pos.append(p); idx.append(i)
        nrm.append(np.zeros_like(p) if n is None else np.asarray(n, F32).reshape(-1, 3))
        nv += p.shape[0]; ni += i.size
    draws = np.array([[first[m], np.asarray(meshes[m][2]).size, base[m], d, *material(d)] for d, (m, _) in enumerate(draw_list)], np.uint32).reshape(-1, 6)
    models = np.array([np.asarray(t, F32).reshape(16) for _, t in draw_list], F32).reshape(-1, 16)
    return np.concatenate(pos), np.concatenate(nrm), np.concatenate(idx), draws, models


def camera(position=(0.0, 0.0, 0.0), forward=(0.0, 0.0, 1.0), aspect=1.0, near=0.1, far=300.0, fov=35.0):
    from plainrenderer_amd.scene import Camera
    return Camera.look(position, forward, aspect=aspect, near=near, far=far, fov=fov)


def perspective_case(width, height, meshes, draw_list, cam, jitter_current=(0.0, 0.0), cam_previous=None, jitter_previous=(0.0, 0.0), models_previous=None):
    """a scene under a perspective camera: mvp from Camera.view_projection (the frame pipeline's matrices) with the jitter in the projection"""
    pos, nrm, idx, draws, models = merge_meshes(meshes, draw_list)
    vp = np.asarray(cam.view_projection(jitter_current), F32).reshape(16)
    vp_previous = np.asarray((cam_previous or cam).view_projection(jitter_previous), F32).reshape(16)
    return make_case(width, height, ref.main_pass_matrices(vp, vp_previous, models, models_previous), pos, idx, draws, nrm, jitter_current, jitter_previous)


_cache = {}


def mesh_scene():
    """the three meshes of the shadow tests' scene in front of a camera at the origin looking down +z, with and without vertex normals; built once, callers
    must not modify it"""
    if "scene" not in _cache:
        from plainrenderer_amd import meshes
        from shadow_raster_cases import affine
        raw = [meshes.box((1.0, 1.5, 0.75), subdiv=4), meshes.uv_sphere(1.25, segments=28, rings=14), meshes.torus(1.5, 0.5, segments=24, sides=12)]
        ms = [mesh_arrays(raw[0], False), mesh_arrays(raw[1], True), mesh_arrays(raw[2], True), mesh_arrays(raw[2], False)]
        draws = [(0, affine((1.0, 1.0, 1.0), 0.6, 0.25, (-2.2, 0.3, 7.0))), (1, affine((1.5, 0.6, 1.1), -0.4, 0.9, (1.8, -0.4, 9.0))),
                 (2, affine((1.2, 1.2, 1.2), 1.1, -0.7, (0.3, 0.9, 12.0))), (3, affine((0.8, 0.8, 0.8), 0.2, 0.5, (-0.5, -1.2, 5.0)))]
        _cache["scene"] = dict(meshes=ms, draws=draws)
    return _cache["scene"]
