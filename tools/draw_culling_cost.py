"""What frustum culling of draws ("drawCulling.comp", plrf_set_draw_culling) costs and saves in bench.py's 4K frame.

    python tools/draw_culling_cost.py [--out FILE] [--frames N] [--instances K]

One process, one build, times by hipEvent (plr_set_pass_timing) averaged over --frames frames, as tools/prepass_raster_cost.py takes them. Two scenes, each both
the scene of the depth prepass and the caster set of the three 2048 x 2048 shadow cascades, each with culling off (flags 0) and on (flags 3):
  (a) in view   the instance set of tools/prepass_raster_cost.py: the three meshes of tests/shadow_raster_cases.py instanced K times (default 202: about 100 k
                triangles) over the view frustum in front of bench.py's camera. Nearly everything is kept: culling can only cost here, its own two executions
  (b) ring      the same instance set eight times, turned about the camera's up axis in steps of 45 degrees: eight times the draws and triangles on a ring
                around the camera, about an eighth of them in view
Per scene and setting: the two cull executions, the prepass's set-up kernel and its tile kernel, and per cascade the set-up and the tile kernel, with the cull's
counters and the rasterisers' `submitted`. The launch grids and the scratch of the rasterisers stay those of the unculled draw list: what culling saves in a
set-up kernel is the transform, clip and snap of the triangles of culled draws, not the lanes that look for a triangle and find none.
The report goes to stdout and to --out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, RES = 3840, 2160, 2048
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
PREFIXES = ("Draw culling", "Depth prepass", "Sun shadow cascade")


def ring(cam, draws, copies=8):
    """the draws `copies` times, copy k turned by k * 360 / copies degrees about the axis through the camera along its up vector"""
    p, up = np.asarray(cam.position, np.float64), np.asarray(cam.up, np.float64)
    up = up / np.linalg.norm(up)
    k_matrix = np.array([[0, -up[2], up[1]], [up[2], 0, -up[0]], [-up[1], up[0], 0]])
    out = []
    for k in range(copies):
        angle = 2.0 * np.pi * k / copies
        r = np.eye(3) + np.sin(angle) * k_matrix + (1.0 - np.cos(angle)) * (k_matrix @ k_matrix)
        turn = np.eye(4)
        turn[:3, :3] = r
        turn[:3, 3] = p - r @ p
        for mesh, t in draws:
            m = np.asarray(t, np.float64).reshape(4, 4).T
            out.append((mesh, (turn @ m).T.astype(np.float32).reshape(16)))
    return out


def pass_times(be, fp, cams, first, frames):
    """-> {pass name: mean us per frame}, a frame's executions of one name summed"""
    be.setPassTiming(True)
    acc = {}
    for i in range(frames + 1):
        fp.frame(cams[first + i], 1.0 / 60.0, 0.5)
        be.waitForGPUIdle()
        if i == 0:
            continue
        frame = {}
        for name, ms in be.getRenderpassTimings():
            if name.startswith(PREFIXES):
                frame[name] = frame.get(name, 0.0) + ms * 1e3
        for name, us in frame.items():
            acc.setdefault(name, []).append(us)
    be.setPassTiming(False)
    return {k: float(np.mean(v)) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--instances", type=int, default=202)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    import prepass_raster_cases as pc
    import shadow_raster_cost
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import CULL_SCENE, CULL_SHADOW_CASTERS, FramePipeline
    args = argparse.Namespace(steps=a.frames * 5 + 20, warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=RES, scene="default")
    be = RenderBackend(W, H, device=0)
    fp = FramePipeline(be, W, H, shadow_map_res=RES)
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    lines = ["# python tools/draw_culling_cost.py: bench.py's scene at %d x %d, cascades %d x %d, fast kernel set, %d frames per figure, %d instances" % (W, H, RES, RES, a.frames, a.instances)]
    cursor = 1
    for i in range(args.warmup):
        fp.frame(cams[cursor + i], 1.0 / 60.0, 0.5)
    cursor += args.warmup
    raw, in_view = shadow_raster_cost.instances(cams[1], a.instances, 1.0)
    meshes = [pc.mesh_arrays(m, k != 0) for k, m in enumerate(raw)]
    for label, draws in (("(a) in view", in_view), ("(b) ring of eight", ring(cams[1], in_view))):
        fp.set_scene_meshes(meshes, [(m, t, *pc.material(d)) for d, (m, t) in enumerate(draws)])
        fp.set_shadow_casters(raw, draws)
        lines.append("%s: %d draws, %d triangles" % (label, len(draws), sum(np.asarray(raw[m][1]).size // 3 for m, _ in draws)))
        lines.append("  %-8s %9s %9s | %9s %11s %10s | %s" % ("culling", "cull main", "cull shd", "submitted", "set-up us", "tiles us", "per cascade: submitted, set-up us, tiles us"))
        for flags in (0, CULL_SCENE | CULL_SHADOW_CASTERS):
            fp.set_draw_culling(flags)
            times = pass_times(be, fp, cams, cursor, a.frames)
            cursor += a.frames + 1
            cascades = []
            for c in range(3):
                cascades.append("%d, %.2f, %.2f" % (fp.shadow_raster_stats(c)[0], times.get("Sun shadow cascade %d (set-up)" % c, float("nan")), times.get("Sun shadow cascade %d" % c, float("nan"))))
            lines.append("  %-8s %9.2f %9.2f | %9d %11.2f %10.2f | %s" % ("on" if flags else "off", times.get("Draw culling, main view", 0.0), times.get("Draw culling, shadow cascades", 0.0),
                                                                  fp.prepass_raster_stats()[0], times.get("Depth prepass (set-up)", float("nan")),
                                                                  times.get("Depth prepass (tiles)", times.get("Depth prepass", float("nan"))), "; ".join(cascades)))
            if flags:
                for v in range(4):
                    s = fp.draw_culling_stats(v)
                    lines.append("    %-10s %d of %d draws and %d of %d triangles kept; culled by near, +x, -x, +y, -y: %r"
                                 % ("main view:" if v == 0 else "cascade %d:" % (v - 1), s["visible_draws"], s["draws"], s["visible_triangles"], s["triangles"], s["culled_by_plane"]))
        fp.set_draw_culling(0)
    lines.append("general-kernel executions of the last frame with culling on: %d" % be.getGeneralKernelExecutions()[0])
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    fp.destroy()
    be.shutdown()


if __name__ == "__main__":
    main()
