"""The scene mesh entry points at the C boundary, the tests' own rasteriser (tests/prepass_raster_reference.py) against hand-computed cases, and the host's
validation and packing of both mesh sets under the sanitizers (tools/scene_packing_check.cpp, a stand-alone program); no GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import prepass_raster_cases as pc
import prepass_raster_reference as ref
from shadow_raster_cases import quad

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counters(r):
    return r["submitted"], r["clipped"], r["drawn"], r["rejects"]


def test_diagonal_through_pixel_centres_covers_every_centre_once():
    """the shadow contract's fill rule, mirrored: corners on pixel centres, split along the diagonal through the centres (k + 0.5, k + 0.5); every centre strictly
    inside belongs to exactly one of the two front faces, and the diagonal to the upper-right half (for the rasterised (v0, v2, v1) it is a left edge)"""
    r = pc.rasterise(pc.pixel_case([quad(2.5, 2.5, 10.5, 10.5, 0.25, 0.75)], 16, 16))
    assert counters(r) == (2, 0, 2, 0)
    assert (r["coverage"][3:10, 3:10] == 1).all() and r["coverage"].max() == 1
    k = np.arange(3, 10)
    assert (r["depth"][k, k] == F32(0.25)).all() and (r["depth"][5, 6:10] == F32(0.25)).all() and (r["depth"][6:10, 5] == F32(0.75)).all()


def test_axis_aligned_quad_owns_its_top_row_and_left_column_only():
    r = pc.rasterise(pc.pixel_case([quad(2.5, 3.5, 11.5, 9.5, 0.5, 0.5)], 16, 12))
    expect = np.zeros((12, 16), np.int32)
    expect[3:9, 2:11] = 1
    assert np.array_equal(r["coverage"], expect)


def test_back_faces_are_culled_and_depth_is_stored_as_it_is():
    tri = [(2.0, 2.0, 0.3), (12.0, 2.0, 0.3), (12.0, 12.0, 0.3)]
    front, back = pc.rasterise(pc.pixel_case([[tri]], 16, 16)), pc.rasterise(pc.pixel_case([[tri]], 16, 16, keep_winding=(0,)))
    assert counters(front) == (1, 0, 1, 0) and counters(back) == (1, 0, 0, 0) and not back["keys"].any()
    covered = front["coverage"] > 0
    assert covered.sum() == 55 and (front["depth"][covered] == F32(0.3)).all() and (front["depth"][~covered] == 0).all()
    assert (front["albedo"][covered] == pc.material(0)[0]).all() and (front["specular"][covered] == pc.material(0)[1]).all()
    assert not front["albedo"][~covered].any() and not front["normal"][~covered].any() and not front["motion"].any()


def test_the_far_plane_is_a_per_fragment_rule():
    """z runs from 0.5 at x = 2 to -0.5 at x = 12: zf <= 0 from x = 7 on, so of the pixel centres 2.5 .. 11.5 only 2.5 .. 6.5 keep a fragment"""
    r = pc.rasterise(pc.pixel_case([[[(2.0, 2.0, 0.5), (12.0, 2.0, -0.5), (12.0, 12.0, -0.5)], [(2.0, 2.0, 0.5), (12.0, 12.0, -0.5), (2.0, 12.0, 0.5)]]], 16, 16))
    assert counters(r) == (2, 0, 2, 0)
    assert r["coverage"][2:12, 2:7].all() and not r["coverage"][:, 7:].any()
    assert r["depth"][5, 2] == F32(0.45)


def test_the_later_triangle_wins_a_tie():
    tri = [(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]
    r = pc.rasterise(pc.pixel_case([[tri], [tri]], 16, 16))
    covered = r["coverage"] > 0
    assert (r["coverage"][covered] == 2).all() and (r["albedo"][covered] == pc.material(1)[0]).all()
    assert ((r["keys"][covered] & np.uint64(0xFFFFFFFF)) == 1).all()


def test_clipping_by_hand():
    """a triangle under an identity matrix with one vertex at x = 40: the plane 32 w - x cuts edges 0 -> 1 and 1 -> 2. The new vertices come from the inside
    vertex: on 0 -> 1, t = 32 / (32 + 8) = 0.8, y = -0.5 + 0.8 * 0.25"""
    tri = np.array([[0.0, -0.5, 0.5, 1.0], [40.0, -0.25, 0.5, 1.0], [0.0, 0.5, 0.5, 1.0]], F32)
    poly, clipped = ref.clip_triangle(tri)
    assert clipped and len(poly) == 4
    t = F32(32.0) / F32(F32(32.0) - F32(-8.0))
    assert np.array_equal(poly[0], tri[0]) and np.array_equal(poly[3], tri[2])
    assert poly[1][0] == F32(0.0) + t * F32(40.0) and poly[1][1] == F32(-0.5) + t * F32(0.25)
    t2 = F32(32.0) / F32(F32(32.0) - F32(-8.0))  # from vertex 2 (inside, d = 32) towards vertex 1 (outside, d = -8)
    assert poly[2][1] == F32(0.5) + t2 * F32(F32(-0.25) - F32(0.5))
    inside, unchanged = ref.clip_triangle(np.array([[0.0, 0.0, 0.5, 1.0], [1.0, 0.0, 0.5, 1.0], [0.0, 1.0, 0.5, 1.0]], F32))
    assert not unchanged and len(inside) == 3
    behind, was = ref.clip_triangle(np.array([[0.0, 0.0, 2.0, 1.0], [1.0, 0.0, 2.0, 1.0], [0.0, 1.0, 2.0, 1.0]], F32))  # z > w everywhere: in front of near
    assert was and behind == []


def test_a_shared_clipped_edge_gets_the_identical_vertex_whatever_the_winding():
    a, b = np.array([0.3, 0.2, 0.9, 1.0], F32), np.array([-0.4, 0.7, 0.5, -0.2], F32)  # b is behind the camera and outside the near plane
    c, d = np.array([0.9, 0.9, 0.5, 1.0], F32), np.array([-0.9, -0.5, 0.5, 1.0], F32)
    p1, _ = ref.clip_triangle(np.stack([a, b, c]))
    p2, _ = ref.clip_triangle(np.stack([b, a, d]))
    on_edge = lambda poly: {tuple(v.tolist()) for v in poly if abs(float(v[3] - v[2])) < 1e-6}
    assert on_edge(p1) & on_edge(p2), "both triangles hold the vertex where a -> b meets the near plane, bit for bit"


def test_attributes_by_hand():
    """one triangle under an identity matrix whose previous matrix shifts x by 0.25 NDC: motion.x = 0.125 -> rint(0.125 * 32767) = 4096, motion.y = 0; with a
    current jitter of 0.125 the shift from the jittered centre is 0.125: code 2048. The face normal of a screen-aligned front face is +z (reverse Z: towards the viewer): stored (128, 128, 255, 255)"""
    previous = pc.IDENTITY.copy()
    previous[12] = 0.25
    tri = [(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]
    r = pc.rasterise(pc.pixel_case([[tri]], 16, 16, previous=previous))
    covered = r["coverage"] > 0
    assert (r["motion"][covered, 0] == 4096).all() and not r["motion"][covered, 1].any()
    assert np.all(r["weights"] >= -1e-12) and np.allclose(r["weights"].sum(axis=1), 1.0, atol=1e-12)
    code = np.unique(r["normal"][covered])
    assert code.size == 1 and code[0] == 0xFFFF8080, hex(int(code[0]))
    case = pc.pixel_case([[tri]], 16, 16, previous=previous)
    case["jitter_current"], case["jitter_previous"] = (0.125, 0.0), (0.0, -0.0625)
    r = pc.rasterise(case)
    assert (r["motion"][covered, 0] == 2048).all() and (r["motion"][covered, 1] == -1024).all(), "((P + 0.25) - (P + 0.125)) / 2 and (-0.0625 - 0) / 2"


def test_vertex_normals_are_interpolated_and_transformed():
    """normals (1, 0, 0), (0, 1, 0), (0, 0, 1) under a model matrix that is a rotation x -> y -> z -> x: at the centroid pixel n = (1, 1, 1) / sqrt 3 -> 0.7887 -> 201"""
    model = pc.glm([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    case = pc.pixel_case([[[(1.5, 1.5, 0.5), (13.5, 1.5, 0.5), (1.5, 13.5, 0.5)]]], 16, 16, keep_winding=())
    case["transforms"][0, 0:16] = model
    case["normals"] = np.eye(3, dtype=F32)
    r = pc.rasterise(case)
    assert r["coverage"][5, 5] == 1 and r["normal"][5, 5] == (201 | (201 << 8) | (201 << 16) | (255 << 24))


def test_the_outside_of_the_generated_meshes_is_the_drawn_side():
    """a sphere 6 in front of the camera: with the index order plainrenderer_amd.meshes emits, the near hemisphere is drawn (reverse Z: the larger depths); reversed,
    the far one. The stored normal of the centre pixel then points at the camera: -z"""
    from plainrenderer_amd import meshes
    raw = meshes.uv_sphere(1.25, segments=28, rings=14)
    model = pc.glm(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 6.0], [0, 0, 0, 1]]))
    out = {}
    for name, idx in (("emitted", np.asarray(raw[1], np.uint32)), ("reversed", pc.reversed_winding(raw[1]))):
        out[name] = pc.rasterise(pc.perspective_case(64, 64, [(raw[0], None, idx)], [(0, model)], pc.camera()))
    covered = out["emitted"]["coverage"] > 0
    assert covered.sum() > 1000 and np.array_equal(covered, out["reversed"]["coverage"] > 0)
    assert (out["emitted"]["depth"][covered] > out["reversed"]["depth"][covered]).all()
    n = out["emitted"]["normal"][32, 32]
    assert (n >> 16) & 0xFF < 16 and abs(int(n & 0xFF) - 128) < 24 and abs(int((n >> 8) & 0xFF) - 128) < 24


OCTAGON_MVP = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0.05], [0, 0, 1, 0]])  # clip = (x, y, 0.05, z)


def test_a_triangle_across_the_near_plane_and_all_four_guard_planes_is_clipped_to_an_octagon():
    """clip = (x, y, 0.05, z) by hand. In (x, y, w) the triangle lies in the plane x + y - 50 (w - 1) = 45; the near plane w = 0.05 cuts its two edges towards the
    vertex behind the camera at NDC (0, -50) and (-50, 0): the diamond (45, 0), (0, 45), (-50, 0), (0, -50). The guard square |x|, |y| <= 32 cuts each of its
    edges twice: x + y = 45 at (32, 13) and (13, 32), y = 0.9 x + 45 at (-14.44, 32) and (-32, 16.2), x + y = -50 at (-32, -18) and (-18, -32),
    y = x / 0.9 - 50 at (16.2, -32) and (32, -14.44)"""
    s = 45.0 / 42.5
    tri = np.array([(45.0, 0.0, 0.05, 1.0), (0.0, 45.0, 0.05, 1.0), (-2.5 * s, -2.5 * s, 0.05, 1.0 - 0.95 * s)], F32)
    want = np.array([(32.0, 13.0), (13.0, 32.0), (-130.0 / 9.0, 32.0), (-32.0, 16.2), (-32.0, -18.0), (-18.0, -32.0), (16.2, -32.0), (32.0, -130.0 / 9.0)])
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        poly, clipped = ref.clip_triangle(tri[list(order)])
        assert clipped and len(poly) == 8
        ndc = np.array([(float(v[0]) / float(v[3]), float(v[1]) / float(v[3])) for v in poly])
        assert np.allclose(np.abs(ndc).max(axis=1), 32.0, atol=1e-3), "every vertex lies on the guard square"
        for axis, side in ((0, 32.0), (0, -32.0), (1, 32.0), (1, -32.0)):
            assert (np.abs(ndc[:, axis] - side) < 1e-3).sum() == 2, "two per side"
        assert all(np.abs(ndc - w).max(axis=1).min() < 1e-3 for w in want), "each of the eight positions worked out above is there (to fp32 rounding at 32: 4e-6 a step)"
        assert all(abs(float(v[2]) - 0.05) < 1e-7 and 0.05 - 1e-6 <= float(v[3]) <= 1.0 for v in poly)
        # around the outline in one sense: the cross products of consecutive edges have one sign
        e = np.roll(ndc, -1, axis=0) - ndc
        cross = e[:, 0] * np.roll(e[:, 1], -1) - e[:, 1] * np.roll(e[:, 0], -1)
        assert (cross > 0).all() or (cross < 0).all()
    positions = tri[:, [0, 1, 3]]  # model-space (x, y, z): z becomes w
    r = pc.rasterise(pc.make_case(96, 64, np.concatenate([pc.IDENTITY, OCTAGON_MVP, OCTAGON_MVP])[None], positions, [0, 2, 1], [[0, 3, 0, 0]]), diagnostics=True)
    assert counters(r) == (1, 1, 3, 0) and (r["coverage"] == 1).all() and r["polygons"] == [(0, 8)] and [f[1] for f in r["fan_drawn"]] == [2, 3, 4]
    assert np.allclose(r["depth"], 0.5, atol=0.03) and r["depth"].min() < 0.49 and r["depth"].max() > 0.51, "w = 5 / (50 - (u + v)): depth 0.05 / w = 0.5 +- 0.02"


def test_a_vertex_at_the_apex_of_the_clip_volume_is_inside_every_plane_and_fails_projection():
    """clip = (x, y, 0.05 z, z): the vertex (0, 0, 0) becomes (0, 0, 0, 0). Every plane distance is 0, and 0 >= 0: inside, so the triangle is not clipped; w > 0
    fails: its one sub-triangle is a counted reject, in either winding. A vertex with w = 1e-30 and z = -1e30 is inside as well and its z / w is -inf"""
    mvp = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.05, 0], [0, 0, 1, 0]])
    apex = np.zeros(4, F32)
    for d in (apex[3] - apex[2], F32(32) * apex[3] - apex[0], F32(32) * apex[3] + apex[0], F32(32) * apex[3] - apex[1], F32(32) * apex[3] + apex[1]):
        assert d == 0 and d >= 0
    positions = np.array([(0.0, 0.0, 0.0), (0.5, 0.0, 1.0), (0.0, 0.5, 1.0)], F32)
    for indices in ([0, 1, 2], [0, 2, 1]):
        r = pc.rasterise(pc.make_case(96, 64, np.concatenate([pc.IDENTITY, mvp, mvp])[None], positions, indices, [[0, 3, 0, 0]]), diagnostics=True)
        assert counters(r) == (1, 0, 0, 1) and r["polygons"] == [(0, 3)] and r["fan_rejected"] == [(0, 0)] and not r["keys"].any()
    steep = pc.glm([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1e30, -1e30], [0, 0, 1, 0]])
    positions[0, 2] = 1e-30
    with np.errstate(all="ignore"):
        z, w = F32(F32(1e30) * F32(1e-30)) + F32(-1e30), F32(1e-30)
        assert z == F32(-1e30) and w - z >= 0 and F32(32) * w >= 0 and np.isneginf(z / w)
    for indices in ([0, 1, 2], [0, 2, 1]):
        r = pc.rasterise(pc.make_case(96, 64, np.concatenate([pc.IDENTITY, steep, steep])[None], positions, indices, [[0, 3, 0, 0]]), diagnostics=True)
        assert counters(r) == (1, 0, 0, 1) and r["fan_rejected"] == [(0, 0)]


def test_motion_saturates_and_a_bad_previous_w_stores_zero():
    """m = (ndcPrevious - ndcCurrent) / 2: a previous matrix that shifts by (+3, -3) NDC gives (1.5, -1.5), clamped to +-1: codes +-32767; by (2 - 1 / 32767, 0)
    gives 1 - 0.5 / 32767 ... the code below; a previous w of -1, of 0 and of NaN store (0, 0); a NaN previous x stores 0 in x and leaves y"""
    tri = [(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]

    def motion(previous, jitter_current=(0.0, 0.0), jitter_previous=(0.0, 0.0)):
        case = pc.pixel_case([[tri]], 16, 16, previous=previous)
        case["jitter_current"], case["jitter_previous"] = jitter_current, jitter_previous
        r = pc.rasterise(case)
        assert (r["coverage"] > 0).sum() == 55
        return np.unique(r["motion"][r["coverage"] > 0].reshape(-1, 2), axis=0).tolist()

    def previous_with(**entries):
        m = pc.IDENTITY.copy()
        for k, v in entries.items():
            m[int(k[1:])] = v
        return m

    assert motion(previous_with(m12=3.0, m13=-3.0)) == [[32767, -32767]]
    assert motion(previous_with(m12=3.0, m13=-3.0), (0.25, -0.125), (-0.5, 0.375)) == [[32767, -32767]]
    assert motion(previous_with(m12=2.0 - 1.4 / 32767.0)) == [[32766, 0]], "m = 1 - 0.7 / 32767: 32766.3 rounds to 32766"
    assert motion(previous_with(m12=2.0 + 1.4 / 32767.0)) == [[32767, 0]]
    assert motion(previous_with(m12=0.25, m15=-1.0)) == [[0, 0]] and motion(previous_with(m12=0.25, m15=0.0)) == [[0, 0]]
    assert motion(previous_with(m12=0.25, m15=np.nan)) == [[0, 0]] and motion(previous_with(m12=0.25, m15=np.inf)) == [[0, 0]]
    assert motion(previous_with(m12=np.nan, m13=0.25)) == [[0, 4096]], "the NaN rule is per channel"
    assert motion(previous_with(m12=0.25, m15=-1.0), (0.25, -0.125), (-0.5, 0.375)) == [[0, 0]], "not the jitter difference either"


def test_a_normal_that_normalises_to_zero_stores_128_128_128():
    tri = [(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]
    case = pc.pixel_case([[tri]], 16, 16)
    covered = pc.rasterise(case)["coverage"] > 0

    def words(model=None, normals=None):
        c = dict(case, transforms=case["transforms"].copy())
        if model is not None:
            c["transforms"][0, :16] = model
        if normals is not None:
            c["normals"] = np.asarray(normals, F32)
        r = pc.rasterise(c)
        assert not r["normal"][~covered].any()
        return [hex(int(v)) for v in np.unique(r["normal"][covered])]

    singular = pc.IDENTITY.copy()
    singular[[0, 5, 10]] = 0.0
    assert words() == ["0xffff8080"]
    assert words(model=singular) == ["0xff808080"] and words(model=singular, normals=[(1.0, 2.0, 3.0)] * 3) == ["0xff808080"]
    assert words(normals=[(np.inf, 0.0, 0.0)] * 3) == ["0xff808080"] and words(normals=[(0.0, np.nan, 0.0)] * 3) == ["0xff808080"]
    assert words(normals=[(1e30, 0.0, 0.0)] * 3) == ["0xff8080ff"], "1e30 has a finite length in fp64"
    assert words(normals=[(1e-30, 0.0, 0.0)] * 3) == ["0xff8080ff"]
    flat = pc.IDENTITY.copy()
    flat[10] = 0.0  # mat3(model) of rank 2 that sends the face normal (0, 0, 1) to zero
    assert words(model=flat) == ["0xff808080"]


def test_a_denormal_depth_survives():
    """a fragment is kept when zf > 0 and its bits are the key: 1.4e-45, the least positive float, has the bits 1"""
    tri = lambda z: [(2.0, 2.0, z), (12.0, 2.0, z), (12.0, 12.0, z)]
    for z, bits in ((1.4e-45, 1), (1e-41, int(F32(1e-41).view(np.uint32))), (1.1754944e-38, 0x00800000)):
        r = pc.rasterise(pc.pixel_case([[tri(z)]], 16, 16))
        covered = r["coverage"] > 0
        assert covered.sum() == 55 and 0 < bits <= 0x00800000 and (r["depth"].view(np.uint32)[covered] == bits).all() and (r["keys"][covered] >> np.uint64(32) == bits).all()
    r = pc.rasterise(pc.pixel_case([[tri(1.4e-45), tri(2.8e-45), tri(-1.4e-45), tri(0.0), tri(-0.0)]], 16, 16))
    assert ((r["keys"][r["coverage"] > 0] & np.uint64(0xFFFFFFFF)) == 1).all() and r["coverage"].max() == 2, "two units beat one; -1.4e-45 and both zeros are dropped"


def test_the_diagnostic_lists_change_no_output_of_the_first_round_cases():
    """the reference's added output (polygons, fan_drawn, fan_rejected): all five images, the keys, the coverage, the weights and the counters of the 11 cases
    that were there before it are the same with and without it"""
    import test_prepass_raster as tpr
    assert len(tpr.FIRST_ROUND) == 11
    for name in tpr.FIRST_ROUND:
        for case, with_lists in tpr.reference(name):
            plain = pc.rasterise(case)
            assert set(with_lists) - set(plain) == {"polygons", "fan_drawn", "fan_rejected"}
            for key, value in plain.items():
                same = np.array_equal(value, with_lists[key], equal_nan=True) if isinstance(value, np.ndarray) and value.dtype.kind == "f" else np.array_equal(value, with_lists[key])
                assert same, "%s: %s differs" % (name, key)
            assert with_lists["drawn"] == len(with_lists["fan_drawn"]) and len(with_lists["fan_rejected"]) <= with_lists["rejects"]


def test_matrices_follow_the_pipelines_product():
    a, b = np.arange(16, dtype=F32) * F32(0.37) - F32(2.0), np.cos(np.arange(16, dtype=F32))
    want = (a.reshape(4, 4).T.astype(np.float64) @ b.reshape(4, 4).T.astype(np.float64)).T.reshape(16)
    assert np.allclose(ref.mat_mul(a, b), want, rtol=1e-5, atol=1e-5)
    m = ref.main_pass_matrices(a, b, [pc.IDENTITY], [pc.IDENTITY])
    assert m.shape == (1, 48) and np.array_equal(m[0, :16], pc.IDENTITY) and np.array_equal(m[0, 16:32], ref.mat_mul(a, pc.IDENTITY))


def test_the_mesh_validation_and_packing_run_clean_under_the_sanitizers(tmp_path):
    """packSceneMeshes and packShadowCasters: the packed bytes, every refusal and which defect of several is reported: tools/scene_packing_check.cpp"""
    compiler = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp_path / "scene_packing_check")
    build = subprocess.run([compiler, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "scene_packing_check.cpp"),
                            os.path.join(ROOT, "plainrenderer_amd", "csrc", "frontend", "scene_packing.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "scene_packing_check: ok", run.stdout + run.stderr


def test_the_scene_mesh_entry_points_are_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    for name in ("plrf_set_scene_meshes", "plrf_set_scene_mesh_transforms", "plrf_get_prepass_raster_stats"):
        assert getattr(lib, name) is not None
    from plainrenderer_amd.frame import PlrfPrepassRasterStats, PlrfSceneDraw, PlrfSceneMesh
    assert C.sizeof(PlrfSceneDraw) == 76 and C.sizeof(PlrfPrepassRasterStats) == 32 and C.sizeof(PlrfSceneMesh) == 40


def test_the_shader_is_registered():
    from plainrenderer_amd import supported_shaders
    assert "depthPrepassRaster.comp" in supported_shaders()
