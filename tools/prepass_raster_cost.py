"""What the depth prepass costs as a compute pass ("depthPrepassRaster.comp", plrf_set_scene_meshes) in bench.py's 4K frame.

    python tools/prepass_raster_cost.py [--out FILE] [--frames N] [--instances K] [--textured [--bc] | --alpha | --normal-mapped] [--aniso N] [--floor]
                                        [--window tx0,ty0,tx1,ty1]

One process, one build. The scene is the instance set of tools/shadow_raster_cost.py: the three meshes of tests/shadow_raster_cases.py (box, uv_sphere, torus:
1496 triangles) instanced K times (default 202: about 100 k triangles) over the view frustum in front of bench.py's camera, rasterised into the 3840 x 2160
G-buffer. By hipEvent (plr_set_pass_timing), averaged over --frames frames: the set-up kernel and the tile kernel (rasterisation and resolve), with the pass'
counters and, from a host-side projection of the triangles the clip leaves unchanged, how their rectangles spread over the 64 x 64 tiles (the busiest tile
bounds the tile kernel). The same with every instance shrunk to 1 / 20, where the tile kernel's time is its scan of the rectangle list and its resolve.
--textured: the same two scenes with material textures (plrf_set_scene_textures): every draw samples a 256 x 256 albedo and a 256 x 256 specular texture
with full chains (two textures, shared by the draws) by the mesh generators' UVs; compare its tile times with a run without the option.
--textured --bc: the --textured scenes with both textures block-compressed (plrf_set_scene_textures_formatted): the albedo as BC1 and the specular as BC3, 256 x 256
with full chains of random blocks; the store's bytes are reported; compare its tile times with --textured of the same build.
--alpha: the --textured scenes with the alpha test (plrf_set_scene_alpha_cutoffs): every draw has cutoff 128 and the albedo texture's alpha is a 0 / 255
checker in cells of 32 texels, so about half of each draw's fragments are discarded; compare its tile times with --textured of the same build.
--normal-mapped: the --textured scenes with normal maps (plrf_set_scene_normal_maps): every draw names a 256 x 256 normal texture with a full chain; the tile
kernel and the shading-normal kernel behind it are reported separately; compare with --textured of the same build.
--aniso N: on top of any of the textured options, anisotropic filtering with maxAnisotropy N (plrf_set_scene_anisotropy); compare with the same options without it.
--floor: a third scene beside the two - one large ground quad 1.5 units below the camera, spanned by the camera's right and forward vectors, seen at a grazing
angle, with the textures of the option at 2 UV units per world unit. The instance scenes' footprints are mostly near-isotropic; this one's are not. With --aniso its
line is followed by the distribution of N over the covered pixels, from tests/prepass_aniso_reference.py on the same view at 480 x 270 (the ratio of a
footprint's axes, and with it N, does not depend on the resolution).
--window tx0,ty0,tx1,ty1: the pass restricted to that tile window (half-open, 64 x 64 tiles; the 4K frame is 60 x 34). The pipeline is then a partition with
band_raster = 1 and halos of 0 whose owned rectangle is the window less one tile on every side that has a neighbour - the rectangle whose raster window
(plrf_get_raster_window) is the one asked for; no exchange is attached: the other passes' halos are stale, the prepass does not read them. A window that touches
a frame edge without spanning the frame also runs its wrap strips (plrf_raster_wrap_strips_for): up to three more executions of the pass per frame. The times
reported are then the SUM over the frame's executions, and a further line gives the main window's execution and the strips' apart. The counters stay the whole
frame's, `covered` counts the window's pixels only. With the tool's halos of 0 the reach is 17 pixels: 0,0,31,18 is the window of a 4K quadrant (three strips),
0,8,60,18 that of the second of four bands (none).
It also reports that a frame WITHOUT scene meshes records the passes and runs the general kernels it did before a scene was ever set.
The report goes to stdout and to --out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]


def tile_hits(matrices, meshes, draws):
    """(mean, largest, touched) number of unclipped front-facing triangles whose tile rectangle touches a tile"""
    import prepass_raster_reference as ref
    nx, ny = (W + 63) // 64, (H + 63) // 64
    grid = np.zeros((ny + 1, nx + 1), np.int64)
    for d, (mesh, _, _, _) in enumerate(draws):
        pos, _, idx = meshes[mesh]
        clip = ref.transform4(matrices[d, 16:32], pos[idx.astype(np.int64)]).reshape(-1, 3, 4)
        inside = np.isfinite(clip).all(axis=(1, 2))
        for plane in range(5):
            inside &= (ref.plane_distance(plane, clip) >= 0).all(axis=1)
        X, Y, _, ok = ref.project(clip[inside].reshape(-1, 4), W, H)
        X, Y, ok = X.reshape(-1, 3), Y.reshape(-1, 3), ok.reshape(-1, 3).all(axis=1)
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        x0, x1 = np.maximum((X.min(1) + 127) >> 8, 0), np.minimum((X.max(1) - 128) >> 8, W - 1)
        y0, y1 = np.maximum((Y.min(1) + 127) >> 8, 0), np.minimum((Y.max(1) - 128) >> 8, H - 1)
        keep = ok & (area < 0) & (x0 <= x1) & (y0 <= y1)
        tx0, tx1, ty0, ty1 = x0[keep] >> 6, x1[keep] >> 6, y0[keep] >> 6, y1[keep] >> 6
        np.add.at(grid, (ty0, tx0), 1); np.add.at(grid, (ty1 + 1, tx1 + 1), 1)
        np.add.at(grid, (ty0, tx1 + 1), -1); np.add.at(grid, (ty1 + 1, tx0), -1)
    hits = grid.cumsum(0).cumsum(1)[:ny, :nx]
    return float(hits.mean()), int(hits.max()), int((hits > 0).sum())


def scene_textures(draw_count, alpha_checker=False):
    """(textures, mesh_uvs, materials) for the three meshes of the instance set: a 256 x 256 albedo and a 256 x 256 specular texture, the host builds the chains.
    alpha_checker: the albedo's alpha is 0 / 255 in cells of 32 x 32 texels instead of 255"""
    from plainrenderer_amd import meshes
    y, x = np.mgrid[0:256, 0:256].astype(np.uint32)
    albedo = ((x * 7 + y * 3) & 255) | (((x ^ y) & 255) << 8) | (((x * 5 + y * 11) & 255) << 16) | np.uint32(0xFF000000)
    if alpha_checker:
        albedo = (albedo & np.uint32(0x00FFFFFF)) | (np.where(((x >> 5) + (y >> 5)) & 1, 255, 0).astype(np.uint32) << np.uint32(24))
    specular = ((x + y) & 255) | (((x * 13) & 255) << 8) | (((y * 9) & 255) << 16) | np.uint32(0xFF000000)
    # the generators' UVs for the scene's meshes (tests/shadow_raster_cases.py mesh_scene: the same arguments, so the same vertices)
    uvs = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_uvs=True)[2], meshes.uv_sphere(1.25, segments=28, rings=14, with_uvs=True)[2],
           meshes.torus(1.5, 0.5, segments=24, sides=12, with_uvs=True)[2]]
    return [(albedo.reshape(-1), 256, 256, 0), (specular.reshape(-1), 256, 256, 0)], uvs, [(0, 1)] * draw_count


def scene_textures_bc(draw_count):
    """(textures, mesh_uvs, materials) of scene_textures with the albedo as BC1 and the specular as BC3: random blocks, all nine levels given"""
    from plainrenderer_amd import ImageFormat
    _, uvs, materials = scene_textures(draw_count)
    rng = np.random.default_rng(7)
    blocks = sum(((max(1, 256 >> l) + 3) // 4) ** 2 for l in range(9))
    return [(rng.integers(0, 256, blocks * 8, dtype=np.uint8), 256, 256, 9, ImageFormat.BC1), (rng.integers(0, 256, blocks * 16, dtype=np.uint8), 256, 256, 9, ImageFormat.BC3)], uvs, materials


def scene_normal_maps(draw_count):
    """(one more texture, mesh_tangents, mesh_bitangents, normal_textures): a 256 x 256 normal texture (the host builds the chain) named by every draw, the
    generators' tangents; the box came without normals, so its bitangents are given (cross(tangent, area-weighted vertex normal)), the others the host derives"""
    import prepass_raster_cases as pc
    from plainrenderer_amd import meshes
    y, x = np.mgrid[0:256, 0:256].astype(np.float64)
    nx, ny = 0.5 + 0.35 * np.sin(x * (2.0 * np.pi / 32.0)), 0.5 + 0.35 * np.cos(y * (2.0 * np.pi / 16.0))
    texels = np.rint(nx * 255.0).astype(np.uint32) | (np.rint(ny * 255.0).astype(np.uint32) << 8) | np.uint32(0xFFFF0000)
    raw = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_tangents=True), meshes.uv_sphere(1.25, segments=28, rings=14, with_tangents=True),
           meshes.torus(1.5, 0.5, segments=24, sides=12, with_tangents=True)]
    tangents = [np.asarray(m[-1], np.float32) for m in raw]
    c = np.cross(tangents[0].astype(np.float64), pc.vertex_normals(raw[0][0], raw[0][1]).astype(np.float64))
    box_bitangents = (c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-30)).astype(np.float32)
    return (texels.reshape(-1), 256, 256, 0), tangents, [box_bitangents, None, None], [2] * draw_count


def floor_scene(cam):
    """(meshes, draws, mesh_uvs): one quad in the plane 1.5 units below the camera (along -up), 120 units wide and from 5 units behind the camera to 300 ahead,
    both windings, UV = 2 (distance along right, distance along forward)"""
    import prepass_raster_cases as pc
    p, f, u, r = (np.asarray(v, np.float64) for v in (cam.position, cam.forward, cam.up, cam.right))
    corners = [(-60.0, -5.0), (60.0, -5.0), (60.0, 300.0), (-60.0, 300.0)]
    positions = np.array([p - 1.5 * u + a * r + b * f for a, b in corners], np.float32)
    normals = np.tile(u.astype(np.float32), (4, 1))
    indices = np.array([0, 2, 1, 0, 3, 2, 0, 1, 2, 0, 2, 3], np.uint32)
    return [(positions, normals, indices)], [(0, pc.IDENTITY)], [np.array(corners, np.float32) * np.float32(2.0)]


def probe_count_histogram(matrices, positions, indices, uvs, textures, mip_bias, max_anisotropy):
    """N over the covered pixels of the floor at 480 x 270, from the tests' reference: {N: share}"""
    import prepass_aniso_reference as aniso
    import prepass_raster_cases as pc
    import prepass_texture_cases as tc
    import prepass_texture_reference as tref
    case = pc.make_case(480, 270, matrices, positions, indices, [[0, indices.size, 0, 0]])
    chains = [(tref.build_chain(t[0], t[1], t[2]), t[1], t[2], tref.full_mip_count(t[1], t[2])) for t in textures]
    tex = tc.textured(case, uvs, [(0, 1)], chains, mip_bias=mip_bias)[1]
    N = aniso.base_images(case, tex, None, max_anisotropy, diagnostics=True)["diagnostics"]["albedo"]["N"]
    values, counts = np.unique(N[N > 0], return_counts=True)
    return {int(v): float(c) / float(counts.sum()) for v, c in zip(values, counts)}


def pass_times(be, fp, cams, first, frames, parts=None):
    """-> ({pass name: mean us per frame} of the prepass, summed over a frame's executions of the pass - a partition runs one per wrap strip and one for its
    window -, number of timed entries of the last frame). parts (a dict): {pass name: [mean us of the frame's k-th execution]}, in recording order"""
    be.setPassTiming(True)
    acc, entries, each = {}, 0, {}
    for i in range(frames + 1):
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
        be.waitForGPUIdle()
        if i == 0:
            continue
        timings = be.getRenderpassTimings()
        entries = len(timings)
        frame = {}
        for name, ms in timings:
            if name.startswith("Depth prepass"):
                frame.setdefault(name, []).append(ms * 1e3)
        for name, values in frame.items():
            acc.setdefault(name, []).append(sum(values))
            for k, v in enumerate(values):
                each.setdefault(name, {}).setdefault(k, []).append(v)
    be.setPassTiming(False)
    if parts is not None:
        parts.update({name: [float(np.mean(v)) for _, v in sorted(by_k.items())] for name, by_k in each.items()})
    return {k: float(np.mean(v)) for k, v in acc.items()}, entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--instances", type=int, default=202)
    ap.add_argument("--textured", action="store_true")
    ap.add_argument("--bc", action="store_true")
    ap.add_argument("--alpha", action="store_true")
    ap.add_argument("--normal-mapped", action="store_true")
    ap.add_argument("--aniso", type=int, default=0)
    ap.add_argument("--floor", action="store_true")
    ap.add_argument("--window")
    ap.add_argument("--out")
    a = ap.parse_args()
    partition, window = {}, None
    if a.window:
        window = tuple(int(v) for v in a.window.split(","))
        gx, gy = (W + 63) // 64, (H + 63) // 64
        if len(window) != 4 or not (0 <= window[0] < window[2] <= gx and 0 <= window[1] < window[3] <= gy):
            ap.error("--window tx0,ty0,tx1,ty1 must be a non-empty half-open tile rectangle inside the %d x %d grid" % (gx, gy))
        x0, x1 = (0 if window[0] == 0 else (window[0] + 1) * 64), (W if window[2] == gx else (window[2] - 1) * 64)
        y0, y1 = (0 if window[1] == 0 else (window[1] + 1) * 64), (H if window[3] == gy else (window[3] - 1) * 64)
        if x0 >= x1 or y0 >= y1:
            ap.error("--window: too narrow for a partition (the window is the owned rectangle and one more tile per side with a neighbour)")
        partition = dict(band_row_begin=y0, band_row_end=y1, band_raster=1, band_gi_halo=0, band_gi_history_halo=0, band_color_halo=0)
        if (x0, x1) != (0, W):
            partition.update(band_col_begin=x0, band_col_end=x1)
    if a.aniso >= 2 and not (a.textured or a.alpha or a.normal_mapped):
        ap.error("--aniso needs one of --textured, --alpha, --normal-mapped: it is a property of the texture samples")
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    import prepass_raster_cases as pc
    import shadow_raster_cost
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import FramePipeline
    args = argparse.Namespace(steps=a.frames * 6 + 20, warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=2048, scene="default")
    be = RenderBackend(W, H, device=0)
    fp = FramePipeline(be, W, H, shadow_map_res=2048, **partition)
    if window is not None and fp.raster_window() != window:
        raise SystemExit("the partition's raster window is %r, not %r" % (fp.raster_window(), window))
    if window is not None:
        be.setPassFusion(1)  # a partition without an attached exchange: keep every intermediate image in memory
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    lines = ["# python tools/prepass_raster_cost.py%s: bench.py's scene at %d x %d, fast kernel set, %d frames per figure" % ((" --normal-mapped" if a.normal_mapped else " --alpha" if a.alpha else " --textured --bc" if a.textured and a.bc else " --textured" if a.textured else "") + (" --aniso %d" % a.aniso if a.aniso else "") + (" --floor" if a.floor else "") + (" --window " + a.window if a.window else ""), W, H, a.frames)]
    cursor = 1
    for i in range(args.warmup):
        fp.frame(cams[cursor + i], 1.0 / 60.0, 0.5)
    cursor += args.warmup
    _, entries_before = pass_times(be, fp, cams, cursor, 2)
    general_before = be.getGeneralKernelExecutions()
    cursor += 3
    tiles = ((W + 63) // 64) * ((H + 63) // 64)
    lines.append("%-26s %9s %9s %9s %8s %8s %13s %11s %10s" % ("scene", "submitted", "drawn", "clipped", "rejects", "covered", "busiest tile", "set-up us", "tiles us"))
    fp.set_scene_anisotropy(a.aniso)
    for label, shrink in (("meshes at scale", 1.0), ("meshes shrunk to 1 / 20", 0.05)) + ((("floor", None),) if a.floor else ()):
        floor_uvs = None
        if shrink is None:
            meshes, draws, floor_uvs = floor_scene(cams[1])
        else:
            raw, draws = shadow_raster_cost.instances(cams[1], a.instances, shrink)
            meshes = [pc.mesh_arrays(m, k != 0) for k, m in enumerate(raw)]
        scene_draws = [(m, t, *pc.material(d)) for d, (m, t) in enumerate(draws)]
        fp.set_scene_meshes(meshes, scene_draws)
        on_floor = lambda t: (t[0], floor_uvs, t[2]) if floor_uvs is not None else t  # the floor is one mesh with UVs of its own
        if a.normal_mapped:
            textures, uvs, materials = on_floor(scene_textures(len(draws)))
            normal_texture, tangents, bitangents, normal_textures = scene_normal_maps(len(draws))
            fp.set_scene_textures(textures + [normal_texture], uvs, materials)
            if floor_uvs is not None:  # tangent along the camera's right, bitangent along its forward
                tangents = [np.tile(np.asarray(cams[1].right, np.float32), (4, 1))]
                bitangents = [np.tile(np.asarray(cams[1].forward, np.float32), (4, 1))]
            fp.set_scene_normal_maps(tangents, bitangents, normal_textures)
        elif a.textured and a.bc:
            fp.set_scene_textures_formatted(*on_floor(scene_textures_bc(len(draws))))
        elif a.textured or a.alpha:
            fp.set_scene_textures(*on_floor(scene_textures(len(draws), alpha_checker=a.alpha)))
        if a.alpha:
            fp.set_scene_alpha_cutoffs([128] * len(draws))
        parts = {}
        times, _ = pass_times(be, fp, cams, cursor, a.frames, parts)
        cursor += a.frames + 1
        submitted, clipped, drawn, rejects = fp.prepass_raster_stats()
        matrices = be.downloadStorageBuffer(fp.storage_buffer("mainPassMatrices"), 192 * len(draws), dtype=np.float32).reshape(-1, 48)
        covered = max(int((be.downloadImage(fp.image("depth%d" % t), 0, np.float32) > 0).sum()) for t in (0, 1))
        mean_hits, max_hits, touched = tile_hits(matrices, meshes, scene_draws)
        # a normal-mapped execution reports the tile kernel as "(tiles)" and the shading-normal kernel behind it under the pass' name
        lines.append("%-26s %9d %9d %9d %8d %8d %13d %11.2f %10.2f" % (label, submitted, drawn, clipped, rejects, covered, max_hits, times.get("Depth prepass (set-up)", float("nan")),
                                                                 times.get("Depth prepass (tiles)", times.get("Depth prepass", float("nan")))))
        if a.normal_mapped:
            lines.append("  shading-normal kernel: %.2f us" % times.get("Depth prepass", float("nan")))
        if parts and max(len(v) for v in parts.values()) > 1:  # in recording order: the wrap strips, then the window
            lines.append("  per execution (wrap strips first, the window last): " + "; ".join("%s %s us" % (n.replace("Depth prepass", "").strip(" ()") or "last kernel", " + ".join("%.2f" % v for v in vs))
                                                                                                for n, vs in sorted(parts.items())))
        lines.append("  %d draws; %d of %d tiles touched, %.1f rectangles per tile on average" % (len(draws), touched, tiles, mean_hits))
        if floor_uvs is not None and a.aniso >= 2 and a.textured and not a.bc:
            g = np.frombuffer(fp.submitted_globals(), np.float32)
            shares = probe_count_histogram(matrices, meshes[0][0], meshes[0][2], floor_uvs[0], scene_textures(1)[0], float(g[79]), a.aniso)
            lines.append("  N over the covered pixels (reference, 480 x 270): " + ", ".join("%d: %.1f %%" % (n, 100.0 * share) for n, share in sorted(shares.items())))
    if a.textured and not a.alpha and not a.normal_mapped:
        chain = sum(max(1, 256 >> l) ** 2 for l in range(9))
        lines.append("texture store: %d bytes" % (sum(t[0].size for t in scene_textures_bc(1)[0]) if a.bc else 2 * chain * 4))
    if window is not None:
        lines.append("tile window %r: %d of %d tiles" % (window, (window[2] - window[0]) * (window[3] - window[1]), tiles))
    general_with = be.getGeneralKernelExecutions()
    fp.set_scene_meshes([], [])
    _, entries_after = pass_times(be, fp, cams, cursor, 2)
    general_after = be.getGeneralKernelExecutions()
    lines.append("general-kernel executions of the last frame: %d before a scene was set, %d with the scene, %d after it was removed" % (general_before[0], general_with[0], general_after[0]))
    lines.append("timed pass entries of a frame: %d before a scene was set, %d after it was removed" % (entries_before, entries_after))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    fp.destroy()
    be.shutdown()


if __name__ == "__main__":
    main()
