"""What generating the frame's noise inputs costs ("blueNoiseVoidAndCluster.comp", "perlinNoise3D.comp"; plrf_generate_noise): one-time work, measured once.

    python tools/noise_cost.py [--out FILE] [--seeds N]

One process, a 256 x 144 pipeline with the froxel passes on (the noise passes do not depend on the frame size), both kernel sets - they run the same kernels. For
each of --seeds seeds, generate_noise(seed) and one frame with plr_set_pass_timing on: the hipEvent time of each of the four blue-noise executions (one per 32 x 32
RG8 texture: two 1024-lane blocks, one per channel, 102 minority pixels, about 1160 selection steps each) and of the Perlin execution (32^3 voxels, 8 cells), with
the swaps the prototype loop took. The report goes to stdout and to --out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
W, H = 256, 144


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    from plainrenderer_amd import RenderBackend, synth
    from plainrenderer_amd.frame import FramePipeline, SyntheticInputs
    from plainrenderer_amd.scene import Camera
    cams = [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=W / H) for i in range(2)]
    be = RenderBackend(W, H, device=0)
    lines = ["# python tools/noise_cost.py: generate_noise(seed) + one frame, hipEvent time per execution, %d seeds per kernel set" % a.seeds]
    try:
        for fast in (False, True):
            be.setMathMode(fast)
            fp = FramePipeline(be, W, H, shadow_map_res=128, brdf_lut_res=16, froxel_depth=8, max_sdf_instances=64, run_volumetrics=1)
            SyntheticInputs(synth.SynthScene(grid=4, cell=8.0, seed_id=973), cams[1], cams[0], W, H, sdf_res=16, shadow_res=128, froxel_depth=8,
                            sun_direction=(0.35, -0.8, 0.45)).upload(fp)
            fp.frame(cams[1], 1.0 / 60.0, 0.5)
            be.setPassTiming(True)
            blue, perlin, swaps = [], [], []
            for seed in range(1, a.seeds + 1):
                fp.generate_noise(seed)
                fp.frame(cams[1], 1.0 / 60.0, 0.5)
                be.waitForGPUIdle()
                for name, ms in be.getRenderpassTimings():
                    if name.startswith("Blue noise"):
                        blue.append(ms * 1e3)
                    elif name.startswith("Perlin noise"):
                        perlin.append(ms * 1e3)
                swaps += [int(v) for v in fp.noise_stats()[:, :, 0].reshape(-1)]
            be.setPassTiming(False)
            fp.destroy()
            label = "fast" if fast else "exact"
            lines.append("%s set, blueNoiseVoidAndCluster, one 32 x 32 RG8 texture (%d executions): mean %.1f us, min %.1f, max %.1f; swaps %d .. %d" %
                         (label, len(blue), np.mean(blue), np.min(blue), np.max(blue), min(swaps), max(swaps)))
            lines.append("%s set, perlinNoise3D, 32^3 with 8 cells (%d executions): mean %.2f us, min %.2f, max %.2f" % (label, len(perlin), np.mean(perlin), np.min(perlin), np.max(perlin)))
    finally:
        be.setMathMode(False)
        be.shutdown()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
