"""What the SDF instances from the scene cost ("sdfInstanceUpdate.comp", "sceneMeanAlbedo.comp"; plrf_set_scene_sdf) in bench.py's 4K frame.

    python tools/scene_sdf_cost.py [--out FILE] [--frames N]

One process, one build, the fast kernel set. The scene is the instance set of tools/shadow_raster_cost.py - the three meshes of tests/shadow_raster_cases.py under
random affine transforms in front of bench.py's camera - with 256 and with 1200 draws (max_sdf_instances' default), every mesh naming one SDF volume of bench.py's
scene, so every draw is an instance and nothing is baked. By hipEvent (plr_set_pass_timing), averaged over --frames frames: "sdfInstanceUpdate.comp" at both
counts, and "sceneMeanAlbedo.comp" (its mark kernel, and the reduction with the three divisions behind it) over the texture store of tools/prepass_raster_cost.py -
a 256 x 256 albedo and a 256 x 256 specular texture with their chains, of which the pass reads level 0 of the albedo - and over one 2048 x 2048 RGBA8 albedo,
where the pass is a read of 16 MiB. The mean albedo pass runs only in a frame after the store changed, so the tool sets the textures again in front of every
timed frame. The report goes to stdout and to --out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]


def timed(be, fp, cams, first, frames, before_frame=None):
    """{pass name: mean us per frame} of the two passes"""
    be.setPassTiming(True)
    acc = {}
    for i in range(frames + 1):
        if before_frame:
            before_frame()
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
        be.waitForGPUIdle()
        if i == 0:
            continue
        for name, ms in be.getRenderpassTimings():
            if name.startswith(("SDF instance update", "Scene mean albedo")):
                acc.setdefault(name, []).append(ms * 1e3)
    be.setPassTiming(False)
    return {k: float(np.mean(v)) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    import prepass_raster_cases as pc
    import prepass_raster_cost
    import shadow_raster_cost
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import FramePipeline
    args = argparse.Namespace(steps=a.frames * 6 + 40, warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=2048, scene="default")
    be = RenderBackend(W, H, device=0)
    fp = FramePipeline(be, W, H, shadow_map_res=2048)
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    volume = inputs.volume_indices[0]
    lines = ["# python tools/scene_sdf_cost.py: bench.py's scene at %d x %d, fast kernel set, %d frames per figure" % (W, H, a.frames)]
    cursor = 1
    for i in range(args.warmup):
        fp.frame(cams[cursor + i], 1.0 / 60.0, 0.5)
    cursor += args.warmup
    for count in (256, 1200):
        raw, draws = shadow_raster_cost.instances(cams[1], count, 1.0)
        meshes = [pc.mesh_arrays(m, k != 0) for k, m in enumerate(raw)]
        fp.set_scene_meshes(meshes, [(m, t, *pc.material(d)) for d, (m, t) in enumerate(draws)])
        fp.set_scene_sdf([volume] * 3)
        times = timed(be, fp, cams, cursor, a.frames)
        cursor += a.frames + 1
        lines.append("sdfInstanceUpdate, %4d instances (%d bytes written): %.2f us" % (fp.scene_sdf_stats()[0], 16 + 128 * count, times.get("SDF instance update", float("nan"))))
    few = min(a.frames, 10)
    stores = [("the cost scene's store (a 256 x 256 albedo named by every draw, 256 KiB read)", prepass_raster_cost.scene_textures(count))]
    rng = np.random.default_rng(11)
    big = rng.integers(0, 1 << 32, 2048 * 2048, dtype=np.uint64).astype(np.uint32)
    uvs = stores[0][1][1]
    stores.append(("one 2048 x 2048 RGBA8 albedo (16 MiB read)", ([(big, 2048, 2048, 1)], uvs, [(0, 0xFFFFFFFF)] * count)))
    for label, (textures, mesh_uvs, materials) in stores:
        times = timed(be, fp, cams, cursor, few, before_frame=lambda: fp.set_scene_textures(textures, mesh_uvs, materials))
        cursor += few + 1
        lines.append("sceneMeanAlbedo over %s, %d draws: mark %.2f us, reduce and finish %.2f us (%d frames)" % (label, count, times.get("Scene mean albedo (mark)", float("nan")),
                                                                                                          times.get("Scene mean albedo", float("nan")), few))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    fp.destroy()
    be.shutdown()


if __name__ == "__main__":
    main()
