"""The shadow caster entry points at the C boundary and the invariants of the tests' own rasteriser (tests/shadow_raster_reference.py); no GPU."""
import ctypes as C

import numpy as np

import shadow_raster_cases as sc
import shadow_raster_reference as ref


def test_diagonal_through_pixel_centres_covers_every_centre_once():
    """corners on pixel centres, split along the diagonal (2.5, 2.5) -> (10.5, 10.5) that passes through the centres (k + 0.5, k + 0.5): every centre strictly
    inside the square, the ones on the diagonal included, belongs to exactly one of the two triangles"""
    r = sc.rasterise(sc.pixel_case(sc.quad(2.5, 2.5, 10.5, 10.5, 0.25, 0.75), 16))
    assert (r["submitted"], r["drawn"], r["rejects"]) == (2, 2, 0)
    assert (r["coverage"][3:10, 3:10] == 1).all()
    assert r["coverage"].max() == 1
    k = np.arange(3, 10)
    upper, lower = int(np.rint(np.float32(0.25) * np.float32(65535))), int(np.rint(np.float32(0.75) * np.float32(65535)))
    assert (r["map"][k, k] == upper).all(), "edge 2 -> 0 of the upper-right half points up: it is a left edge and owns the diagonal"
    assert (r["map"][5, 6:10] == upper).all() and (r["map"][6:10, 5] == lower).all()


def test_axis_aligned_quad_owns_its_top_row_and_left_column_only():
    r = sc.rasterise(sc.pixel_case(sc.quad(2.5, 3.5, 11.5, 9.5, 0.5, 0.5), 16))
    expect = np.zeros((16, 16), np.int32)
    expect[3:9, 2:11] = 1  # rows 3 .. 8, columns 2 .. 10: the top row y = 3.5 and the left column x = 2.5 are in, the bottom row 9.5 and the right column 11.5 out
    assert np.array_equal(r["coverage"], expect)


def test_closed_box_leaves_the_depth_of_its_far_faces():
    """front faces are culled: of a closed convex mesh every covered texel holds exactly one fragment, the one further from the light (reverse Z: the smaller
    depth). The flipped box covers the same texels with its near side."""
    from plainrenderer_amd import meshes
    s = sc.mesh_scene()
    light = ref.light_matrices(s["info"])[0]
    box = sc.as_arrays(meshes.box((1.0, 1.5, 0.75), subdiv=2))
    out = {}
    for name, mesh in (("far", box), ("near", sc.flipped(box))):
        pos, idx, draws, transforms = ref.merge_meshes([mesh], [(0, s["draws"][0][1])])
        out[name] = ref.rasterise(light, transforms, pos, idx, draws, 200)
    covered = out["far"]["coverage"] > 0
    assert covered.sum() > 300 and out["far"]["coverage"].max() == 1 and out["near"]["coverage"].max() == 1
    assert np.array_equal(out["far"]["coverage"], out["near"]["coverage"])
    assert (out["far"]["map"][covered] < out["near"]["map"][covered]).all()
    assert (out["far"]["map"][~covered] == 0).all()
    assert out["far"]["drawn"] + out["near"]["drawn"] <= out["far"]["submitted"] == 6 * 2 * 2 * 2


def test_vertex_outside_the_guard_band_is_a_counted_reject():
    far = float(2 ** 21)
    r = sc.rasterise(sc.pixel_case([[(far, 2.0, 0.5), (2.0, 2.0, 0.5), (2.0, 12.0, 0.5)], [(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]], 16))
    assert (r["submitted"], r["drawn"], r["rejects"]) == (2, 1, 1)
    alone = sc.rasterise(sc.pixel_case([[(far, 2.0, 0.5), (2.0, 2.0, 0.5), (2.0, 12.0, 0.5)]], 16))
    assert (alone["submitted"], alone["drawn"], alone["rejects"]) == (1, 0, 1) and not alone["map"].any() and not alone["coverage"].any()
    nan = sc.pixel_case([[(2.0, 2.0, np.nan), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)]], 16)
    assert sc.rasterise(nan)["rejects"] == 1


def test_depth_is_clamped_and_rounded_to_nearest_even():
    """z = 1.5 clamps to code 65535, z = -0.5 to 0; 0.5 * 65535 = 32767.5 rounds to the even 32768"""
    tri = lambda z: [(2.0, 2.0, z), (12.0, 2.0, z), (12.0, 12.0, z)]
    assert sc.rasterise(sc.pixel_case([tri(1.5)], 16))["map"].max() == 65535
    low = sc.rasterise(sc.pixel_case([tri(-0.5)], 16))
    assert low["coverage"].any() and not low["map"].any()
    assert sc.rasterise(sc.pixel_case([tri(0.5)], 16))["map"].max() == 32768


def test_depth_clamp_takes_the_number_of_a_nan_and_a_number():
    """the clamp is fmin(fmax(zf, 0), 1) with IEEE maxNum / minNum semantics: a NaN zf stores code 0, +inf stores 65535. z0 = -3e38 and z1 = 3e38 are finite,
    z1 - z0 overflows to +inf, and on edge 2 -> 0 (l1 == 0, a left edge up the pixel centres of column 4) zf = 0 * inf = NaN; beside it zf = +inf"""
    f = np.float32
    assert ref.clamp01(np.array([np.nan, np.inf, -np.inf, -0.5, 0.25, 1.5], f)).tolist() == [0.0, 1.0, 0.0, 0.0, 0.25, 1.0]
    r = sc.rasterise(sc.pixel_case([[(4.5, 2.5, -3e38), (12.5, 6.5, 3e38), (4.5, 10.5, 0.5)]], 16))
    rows = np.arange(3, 10)
    assert (r["submitted"], r["drawn"], r["rejects"]) == (1, 1, 0), "every vertex depth is finite: no reject"
    assert (r["coverage"][rows, 4] == 1).all() and not r["map"][rows, 4].any()
    inner = r["coverage"] > 0
    inner[:, 4] = False
    assert inner.sum() > 10 and (r["map"][inner] == 65535).all()


def test_old_and_new_clamp_agree_on_the_first_four_cases(monkeypatch):
    """np.fmax / np.fmin instead of np.maximum / np.minimum changes no texel where zf is a number: the maps of unit96, mesh200, dense64 and big130 are what they were"""
    import test_shadow_raster as tsr
    new = {name: [r["map"] for _, _, r in tsr.reference(name)] for name in ("unit96", "mesh200", "dense64", "big130")}
    monkeypatch.setattr(ref, "clamp01", lambda zf: np.minimum(np.maximum(zf, np.float32(0.0)), np.float32(1.0)))
    for name, maps in new.items():
        old = [sc.rasterise(case)["map"] for case, _ in tsr.CASES[name]()]
        assert len(old) == len(maps) and all(np.array_equal(a, b) for a, b in zip(old, maps)), name


def test_a_slot_outside_its_buffer_is_a_counted_reject():
    """the contract's clause: a triangle counts as submitted and as a reject, and draws nothing, when its three index slots are not all inside `indices`, when a
    vertex (index + vertexOffset, in 64 bits) is not inside `positions`, or when its draw's transformIndex is not inside `transforms`. Submitted triangles per
    draw stay indexCount // 3."""
    base = sc.pixel_case([[(2.0, 2.0, 0.5), (12.0, 2.0, 0.5), (12.0, 12.0, 0.5)], [(1.0, 3.0, 0.7), (9.0, 3.0, 0.7), (9.0, 14.0, 0.7)]], 16)
    whole = sc.rasterise(base)
    first = sc.rasterise(dict(base, draws=np.array([[0, 3, 0, 0]], np.uint32)))
    assert (whole["submitted"], whole["drawn"], whole["rejects"]) == (2, 2, 0) and (first["submitted"], first["drawn"]) == (1, 1)

    def run(**changed):
        r = sc.rasterise(dict(base, **changed))
        return (r["submitted"], r["drawn"], r["rejects"]), r["map"]

    # the last index slot of the second triangle is one past the end (the buffer holds 5 indices); with 8 of 6 the draw still has two triangles
    counters, out = run(indices=base["indices"][:5])
    assert counters == (2, 1, 1) and np.array_equal(out, first["map"])
    counters, out = run(draws=np.array([[0, 8, 0, 0]], np.uint32))
    assert counters == (2, 2, 0) and np.array_equal(out, whole["map"])
    counters, out = run(draws=np.array([[0, 9, 0, 0]], np.uint32))
    assert counters == (3, 2, 1) and np.array_equal(out, whole["map"])
    counters, _ = run(draws=np.array([[7, 6, 0, 0]], np.uint32))  # a draw that starts behind the buffer
    assert counters == (2, 0, 2)
    # a vertex equal to the vertex count: through the index, through vertexOffset, and not wrapped into the buffer by 32-bit arithmetic
    idx = base["indices"].copy()
    idx[5] = 6
    counters, out = run(indices=idx)
    assert counters == (2, 1, 1) and np.array_equal(out, first["map"])
    counters, out = run(indices=np.array([0, 1, 2, 0, 1, 2], np.uint32), draws=np.array([[0, 3, 0, 0], [3, 3, 4, 0]], np.uint32))
    assert counters == (2, 1, 1) and np.array_equal(out, first["map"])
    idx[5] = 0xFFFFFFFF
    counters, out = run(indices=idx, draws=np.array([[0, 3, 0, 0], [3, 3, 3, 0]], np.uint32))  # 0xFFFFFFFF + 3 is vertex 2 in 32 bits
    assert counters == (2, 1, 1) and np.array_equal(out, first["map"])
    # transformIndex equal to the transform count: the whole draw
    counters, out = run(draws=np.array([[0, 3, 0, 0], [3, 3, 0, 1]], np.uint32))
    assert counters == (2, 1, 1) and np.array_equal(out, first["map"])
    counters, out = run(draws=np.array([[0, 6, 0, 1]], np.uint32))
    assert counters == (2, 0, 2) and not out.any()
    # no buffer at all
    counters, out = run(positions=np.zeros((0, 3), np.float32))
    assert counters == (2, 0, 2) and not out.any()


def test_the_shadow_caster_entry_points_are_exported():
    from plainrenderer_amd import backend
    lib = backend._load()
    for name in ("plrf_set_shadow_casters", "plrf_set_shadow_caster_transforms", "plrf_get_shadow_raster_stats"):
        assert getattr(lib, name) is not None
    from plainrenderer_amd.frame import PlrfShadowDraw, PlrfShadowRasterStats
    assert C.sizeof(PlrfShadowDraw) == 68 and C.sizeof(PlrfShadowRasterStats) == 24


def test_the_shader_is_registered():
    from plainrenderer_amd import supported_shaders
    assert "sunShadowRaster.comp" in supported_shaders()
