"""What the debug geometry pass ("debugGeometry.comp", plrf_set_debug_geometry) costs in bench.py's 4K frame.

    python tools/debug_lines_cost.py [--out FILE] [--frames N] [--instances K] [--lines L]

One process, one build, times by hipEvent (plr_set_pass_timing) averaged over --frames frames, as tools/draw_culling_cost.py takes them. The scene is the instance
set of tools/prepass_raster_cost.py: the three meshes of tests/shadow_raster_cases.py instanced K times (default 202) over the view frustum in front of bench.py's
camera, each mesh with a baked scene SDF, so that every draw is an SDF instance as well. Settings, one after the other:
  off            flags 0: the frame as it is without the pass (the sum of all its passes is the figure to read the others against)
  draw boxes     PLRF_DEBUG_DRAW_BOXES: 12 K segments
  + SDF boxes    PLRF_DEBUG_DRAW_BOXES | PLRF_DEBUG_SDF_BOXES: 24 K segments
  lines          PLRF_DEBUG_LINES alone with L (default 10 000) seeded segments between random points of the view frustum
Per setting: the pass's time (its three launches and the clears in front of them are one entry), the sum of all passes of the frame, and the pass's counters.
The report goes to stdout and to --out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, RES = 3840, 2160, 2048
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]


def frustum_lines(cam, count):
    """seeded segments between two random points of the view frustum, 4 to 45 units in front of the camera; random colours"""
    rng = np.random.default_rng(0x4C494E53)
    pos, fwd = np.asarray(cam.position, np.float64), np.asarray(cam.forward, np.float64)
    right, up = np.asarray(cam.right, np.float64), np.asarray(cam.up, np.float64)

    def points():
        d = rng.uniform(4.0, 45.0, (count, 1))
        return pos + d * fwd + rng.uniform(-0.45, 0.45, (count, 1)) * d * right + rng.uniform(-0.2, 0.2, (count, 1)) * d * up
    return np.concatenate([points(), points(), rng.uniform(0.0, 4.0, (count, 3))], axis=1).astype(np.float32)


def frame_times(be, fp, cams, first, frames):
    """-> (mean us of the debug geometry pass, mean us of all passes of a frame)"""
    be.setPassTiming(True)
    debug, total = [], []
    for i in range(frames + 1):
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
        be.waitForGPUIdle()
        if i == 0:
            continue
        timings = be.getRenderpassTimings()
        debug.append(sum(ms for name, ms in timings if name.startswith("Debug geometry")) * 1e3)
        total.append(sum(ms for _, ms in timings) * 1e3)
    be.setPassTiming(False)
    return float(np.mean(debug)), float(np.mean(total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--instances", type=int, default=202)
    ap.add_argument("--lines", type=int, default=10000)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    import prepass_raster_cases as pc
    import shadow_raster_cost
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import DEBUG_DRAW_BOXES, DEBUG_LINES, DEBUG_SDF_BOXES, SDF_BAKE, FramePipeline
    args = argparse.Namespace(steps=a.frames * 5 + 20, warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=RES, scene="default")
    be = RenderBackend(W, H, device=0)
    fp = FramePipeline(be, W, H, shadow_map_res=RES)
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    lines = ["# python tools/debug_lines_cost.py: bench.py's scene at %d x %d, fast kernel set, %d frames per figure, %d instances, %d lines" % (W, H, a.frames, a.instances, a.lines)]
    raw, in_view = shadow_raster_cost.instances(cams[1], a.instances, 1.0)
    meshes = [pc.mesh_arrays(m, k != 0) for k, m in enumerate(raw)]
    fp.set_scene_meshes(meshes, [(m, t, *pc.material(d)) for d, (m, t) in enumerate(in_view)])
    fp.set_scene_sdf([SDF_BAKE] * len(meshes))
    lines.append("scene SDF: %d instances, %d volumes baked" % fp.scene_sdf_stats()[:2])
    fp.set_debug_lines(frustum_lines(cams[1], a.lines))
    cursor = 1
    for i in range(args.warmup):
        fp.frame(cams[cursor + i], 1.0 / 60.0, 0.5)
    cursor += args.warmup
    lines.append("  %-12s %12s %14s | %s" % ("setting", "pass us", "all passes us", "submitted, clipped, rejected, drawn, fragments, pixels written"))
    for label, flags in (("off", 0), ("draw boxes", DEBUG_DRAW_BOXES), ("+ SDF boxes", DEBUG_DRAW_BOXES | DEBUG_SDF_BOXES), ("lines", DEBUG_LINES), ("off again", 0)):
        fp.set_debug_geometry(flags)
        debug, total = frame_times(be, fp, cams, cursor, a.frames)
        cursor += a.frames + 1
        s = fp.debug_geometry_stats()
        lines.append("  %-12s %12.2f %14.2f | %d, %d, %d, %d, %d, %d" % (label, debug, total, s["submitted"], s["clipped"], s["rejected"], s["drawn"], s["fragments"], s["pixels_written"]))
    lines.append("general-kernel executions of the last frame: %d" % be.getGeneralKernelExecutions()[0])
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    fp.destroy()
    be.shutdown()


if __name__ == "__main__":
    main()
