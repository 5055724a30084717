"""What the sun shadow cascades cost as a compute pass ("sunShadowRaster.comp", plrf_set_shadow_casters) in bench.py's 4K frame.

    python tools/shadow_raster_cost.py [--out FILE] [--frames N] [--rounds R] [--instances K] [--alpha | --alpha-bc3]

One process, one build. The casters are the three meshes of tests/shadow_raster_cases.py (box, uv_sphere, torus: 1496 triangles) instanced K times (default 202:
about 100 k triangles) over the view frustum in front of bench.py's camera, rasterised into the frame's three 2048 x 2048 cascades with the uploaded light matrices.
  * per cascade, by hipEvent (plr_set_pass_timing): the set-up kernel and the tile kernel, averaged over --frames frames, with the pass' counters and, from a
    host-side projection of the same triangles (tests/shadow_raster_reference.py), how the drawn triangles' rectangles spread over the 64 x 64 tiles: the tile
    kernel's blocks all run at once, so its time is its busiest tile's;
  * the same with every instance shrunk to 1 / 20: the triangles fall between pixel centres or cover one, so the tile kernel's time is its scan of the
    rectangle list (entries x tiles) and its clear, not fragment work - the two runs together say which of the two bounds the kernel;
  * the frame with and without casters, alternately (--rounds blocks of --frames frames each, host clock around the submits and one wait; the uploaded shadow
    maps are restored in front of every block without casters, so both kinds of block shade the same maps each time).
--alpha: every draw is an alpha-tested cutout (plrf_set_shadow_caster_cutouts): the meshes' own UVs, one 256 x 256 texture whose alpha is a 0 / 255 checker in
cells of 32 texels with its full chain, cutoff 128 - the pass' tested instantiation, against the same scene without the switch.
--alpha-bc3: the --alpha scene with its texture stored as BC3 (plrf_set_shadow_caster_cutouts_formatted): the same chain, every level encoded on the host by
plr_encode_rgba8_to_bc - the pass' format-aware instantiation. The report states the bytes of the texel store either way.
--rounds 0 leaves out the frame with and without casters.
The report goes to stdout and to --out.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, RES = 3840, 2160, 2048


def instances(cam, count, shrink=1.0):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shadow_raster_cases as sc
    s = sc.mesh_scene()
    rng = np.random.default_rng(0x434F5354)
    pos, fwd = np.asarray(cam.position, np.float64), np.asarray(cam.forward, np.float64)
    right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)
    draws = []
    for k in range(count):
        d = rng.uniform(4.0, 45.0)
        at = pos + d * fwd + rng.uniform(-0.45, 0.45) * d * right + rng.uniform(-0.2, 0.2) * d * up
        scale = rng.uniform(0.5, 2.0, 3) * (0.25 + d / 30.0) * shrink
        draws.append((k % 3, sc.affine(scale, rng.uniform(0, 6.28), rng.uniform(-1.0, 1.0), at)))
    return s["meshes"], draws


def checker_cutouts(draw_count):
    """the arguments of set_shadow_caster_cutouts under --alpha: (textures, mesh_uvs, cutouts)"""
    from plainrenderer_amd import meshes
    uvs = [meshes.box((1.0, 1.5, 0.75), subdiv=4, with_uvs=True)[2], meshes.uv_sphere(1.25, segments=28, rings=14, with_uvs=True)[2],
           meshes.torus(1.5, 0.5, segments=24, sides=12, with_uvs=True)[2]]  # (the meshes of tests/shadow_raster_cases.py's mesh scene)
    y, x = np.mgrid[0:256, 0:256]
    alpha = np.where(((x // 32) + (y // 32)) % 2 == 0, 255, 0).astype(np.uint32)
    texels = ((alpha << np.uint32(24)) | np.uint32(0x00808080)).reshape(-1)
    return [(texels, 256, 256, 0)], uvs, [(0, 128)] * draw_count  # mip_count 0: the host builds the full chain


def checker_cutouts_bc3(draw_count):
    """the arguments of set_shadow_caster_cutouts_formatted under --alpha-bc3: checker_cutouts' texture with its chain (the host's rule, as
    tests/prepass_texture_reference.py writes it) as BC3 blocks. -> ((textures, mesh_uvs, cutouts), bytes of the store)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import prepass_texture_reference as tref
    from plainrenderer_amd import image_io
    (texels, w, h, _), = checker_cutouts(draw_count)[0]
    mips = tref.full_mip_count(w, h)
    chain, blocks, at = tref.build_chain(texels, w, h), [], 0
    for l in range(mips):
        lw, lh = tref.level_size(w, h, l)
        blocks.append(image_io.encode_rgba8_to_bc(image_io.ImageFormat.BC3, lw, lh, chain[at:at + lw * lh]))
        at += lw * lh
    data = np.concatenate(blocks)
    _, uvs, cutouts = checker_cutouts(draw_count)
    return ([(data, w, h, mips, int(image_io.ImageFormat.BC3))], uvs, cutouts), int(data.size)


def set_cutouts(fp, a, draw_count):
    """-> the bytes of the casters' texel store"""
    if a.alpha_bc3:
        arguments, stored = checker_cutouts_bc3(draw_count)
        fp.set_shadow_caster_cutouts_formatted(*arguments)
        return stored
    fp.set_shadow_caster_cutouts(*checker_cutouts(draw_count))
    return 4 * sum(max(1, 256 >> l) ** 2 for l in range(9))


def tile_hits(light, meshes, draws, res):
    """(mean, largest) number of drawn triangles whose tile rectangle touches a tile, over the tiles of the map"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shadow_raster_reference as ref
    n = (res + 63) // 64
    grid = np.zeros((n + 1, n + 1), np.int64)
    for mesh, matrix in draws:
        pos, idx = meshes[mesh]
        X, Y, _, inside = ref.project(light, matrix, pos[idx.astype(np.int64)], res)
        X, Y, ok = X.reshape(-1, 3), Y.reshape(-1, 3), inside.reshape(-1, 3).all(axis=1)
        area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
        x0, x1 = np.maximum((X.min(1) + 127) >> 8, 0), np.minimum((X.max(1) - 128) >> 8, res - 1)
        y0, y1 = np.maximum((Y.min(1) + 127) >> 8, 0), np.minimum((Y.max(1) - 128) >> 8, res - 1)
        keep = ok & (area > 0) & (x0 <= x1) & (y0 <= y1)
        tx0, tx1, ty0, ty1 = x0[keep] >> 6, x1[keep] >> 6, y0[keep] >> 6, y1[keep] >> 6
        np.add.at(grid, (ty0, tx0), 1); np.add.at(grid, (ty1 + 1, tx1 + 1), 1)
        np.add.at(grid, (ty0, tx1 + 1), -1); np.add.at(grid, (ty1 + 1, tx0), -1)
    hits = grid.cumsum(0).cumsum(1)[:n, :n]
    return float(hits.mean()), int(hits.max()), int((hits > 0).sum())


def timed_block(be, fp, cams, first, frames):
    be.waitForGPUIdle()
    t0 = time.perf_counter()
    for i in range(frames):
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
    be.waitForGPUIdle()
    return (time.perf_counter() - t0) * 1e3 / frames


def pass_times(be, fp, cams, first, frames):
    """-> {pass name: mean us} of the shadow passes over `frames` frames"""
    be.setPassTiming(True)
    acc = {}
    for i in range(frames + 1):
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
        be.waitForGPUIdle()
        if i == 0:
            continue
        for name, ms in be.getRenderpassTimings():
            if name.startswith("Sun shadow cascade"):
                acc.setdefault(name, []).append(ms * 1e3)
    be.setPassTiming(False)
    return {k: float(np.mean(v)) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--instances", type=int, default=202)
    ap.add_argument("--alpha", action="store_true")
    ap.add_argument("--alpha-bc3", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.alpha and a.alpha_bc3:
        ap.error("--alpha and --alpha-bc3 exclude one another")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import FramePipeline
    args = argparse.Namespace(steps=a.frames * (2 * a.rounds + 4), warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=RES, scene="default")
    be = RenderBackend(W, H, device=0)
    fp = FramePipeline(be, W, H, shadow_map_res=RES)
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    lines = ["# python tools/shadow_raster_cost.py%s: bench.py's scene at %d x %d, cascades %d x %d, fast kernel set, %d frames per block"
             % (" --alpha" if a.alpha else " --alpha-bc3" if a.alpha_bc3 else "", W, H, RES, RES, a.frames)]
    cursor = 1
    for i in range(args.warmup):
        fp.frame(cams[cursor + i], 1.0 / 60.0, 0.5)
    cursor += args.warmup
    tiles = ((RES + 63) // 64) ** 2
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shadow_raster_reference as ref
    lights = ref.light_matrices(inputs.shadow_info)
    for label, shrink in (("meshes at scale", 1.0), ("meshes shrunk to 1 / 20", 0.05)):
        meshes, draws = instances(cams[1], a.instances, shrink)
        fp.set_shadow_casters(meshes, draws)
        if a.alpha or a.alpha_bc3:
            stored = set_cutouts(fp, a, len(draws))
        times = pass_times(be, fp, cams, cursor, a.frames)
        cursor += a.frames + 1
        lines.append("%s: %d draws" % (label, len(draws)) + ("; the casters' texel store holds %d bytes (%s), push constants and storage buffers of a cascade's record: %r"
                                                            % (stored, "BC3" if a.alpha_bc3 else "RGBA8", fp.shadow_raster_record()) if a.alpha or a.alpha_bc3 else ""))
        for c in range(3):
            submitted, drawn, rejects = fp.shadow_raster_stats(c)
            setup = times.get("Sun shadow cascade %d (set-up)" % c, float("nan"))
            tile = times.get("Sun shadow cascade %d" % c, float("nan"))
            covered = int((be.downloadImage(fp.image("shadow%d" % c), 0, np.uint16) > 0).sum())
            mean_hits, max_hits, touched = tile_hits(lights[c], meshes, draws, RES)
            lines.append("  cascade %d: set-up %8.2f us, tiles %8.2f us; %d triangles submitted, %d drawn, %d guard-band rejects, %d texels covered; "
                         "%d of %d tiles touched, %.1f hits per tile on average, %d in the busiest"
                         % (c, setup, tile, submitted, drawn, rejects, covered, touched, tiles, mean_hits, max_hits))
    general = be.getGeneralKernelExecutions()
    lines.append("general-kernel executions of the last frame with casters: %d" % general[0])
    meshes, draws = instances(cams[1], a.instances, 1.0)
    with_ms, without_ms = [], []
    for r in range(a.rounds):
        fp.set_shadow_casters([], [])
        for i in range(4):
            be.uploadImage(fp.image("shadow%d" % i), inputs.shadow_maps[i])
        fp.frame(cams[cursor], 1.0 / 60.0, 0.5)
        without_ms.append(timed_block(be, fp, cams, cursor + 1, a.frames))
        cursor += a.frames + 1
        fp.set_shadow_casters(meshes, draws)
        if a.alpha or a.alpha_bc3:
            set_cutouts(fp, a, len(draws))
        fp.frame(cams[cursor], 1.0 / 60.0, 0.5)
        with_ms.append(timed_block(be, fp, cams, cursor + 1, a.frames))
        cursor += a.frames + 1
    if a.rounds:
        lines.append("frame without casters: " + ", ".join("%.4f" % v for v in without_ms) + " ms per frame (median %.4f)" % float(np.median(without_ms)))
        lines.append("frame with casters:    " + ", ".join("%.4f" % v for v in with_ms) + " ms per frame (median %.4f)" % float(np.median(with_ms)))
        lines.append("difference of the medians: %.1f us per frame for three cascades" % ((float(np.median(with_ms)) - float(np.median(without_ms))) * 1e3))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    fp.destroy()
    be.shutdown()


if __name__ == "__main__":
    main()
