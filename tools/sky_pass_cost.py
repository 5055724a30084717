"""What the sky pass (plrf_settings.run_sky, "skyAndSunSprite.comp") costs in bench.py's 4K frame.

    python tools/sky_pass_cost.py [--out FILE] [--baseline-lib PATH/libplr.so]

Runs bench.py's scene at 3840 x 2160 in CHILD processes (a fresh process per run: each has its own HIP context, and the tracer wraps the child only):
run_sky = 0 and run_sky = 1 once plain (frame time over --frames frames, host clock around the submits + one wait) and once under
`rocprofv3 --kernel-trace --stats` (per-kernel calls and time). With --baseline-lib a third traced run loads that library (PLR_LIB: a build of another
commit) with the setting left alone, and the report says whether the run_sky = 0 kernel list - names and calls - equals that build's.
The report goes to stdout and to --out.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 3840, 2160


def child(run_sky, frames):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import torch  # noqa: F401  (first: it brings its own HIP runtime)
    import bench
    from plainrenderer_amd import RenderBackend
    from plainrenderer_amd.frame import FramePipeline
    args = argparse.Namespace(steps=frames, warmup=5, profile_frames=0, grid=16, sdf_res=64, shadow_res=2048, scene="default")
    be = RenderBackend(W, H, device=0)
    extra = {} if run_sky < 0 else dict(run_sky=run_sky)  # < 0: a library that does not know the setting
    fp = FramePipeline(be, W, H, shadow_map_res=args.shadow_res, **extra)
    _, cams, inputs = bench.build_scene(args, "cuda:0", W, H, None)
    inputs.upload(fp)
    for i in range(args.warmup):
        fp.frame(cams[i + 1], 1.0 / 60.0, 0.5)
    be.waitForGPUIdle()
    t0 = time.perf_counter()
    for i in range(frames):
        fp.frame(cams[args.warmup + i + 1], 1.0 / 60.0, 0.5)
    be.waitForGPUIdle()
    ms = (time.perf_counter() - t0) * 1e3 / frames
    general = be.getGeneralKernelExecutions()
    sky_share = float((inputs.gb["depth"] == 0).mean())
    print("SKY_PASS_COST " + json.dumps(dict(run_sky=run_sky, frame_ms=ms, frames=frames, general_kernel_executions=general[0], sky_pixel_share=sky_share)), flush=True)
    fp.destroy()
    be.shutdown()


def run_child(run_sky, frames, traced, lib=None):
    """-> (the child's JSON record, {kernel name: (calls, total ns)} or None)"""
    env = dict(os.environ)
    if lib:
        env["PLR_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(run_sky), "--frames", str(frames)]
    with tempfile.TemporaryDirectory() as tmp:
        if traced:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "kt", "--output-format", "csv", "--"] + cmd
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SKY_PASS_COST ")][-1][len("SKY_PASS_COST "):])
        kernels = None
        if traced:
            kernels = {}
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                with open(path) as fh:
                    for row in csv.DictReader(fh):
                        if "plr::" in row["Name"]:
                            kernels[row["Name"]] = (int(row["Calls"]), int(float(row["TotalDurationNs"])))
    return rec, kernels


def short(name):
    return name.split("(")[0].replace("plr::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out")
    ap.add_argument("--baseline-lib")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.frames)
    lines = ["# python tools/sky_pass_cost.py: bench.py's scene at %d x %d, %d frames per run, fast kernel set; a fresh process per run" % (W, H, a.frames)]
    plain = {s: run_child(s, a.frames, False)[0] for s in (0, 1)}
    traced = {s: run_child(s, a.frames, True) for s in (0, 1)}
    for s in (0, 1):
        lines.append("run_sky = %d: %.4f ms per frame (%.4f under the tracer), general-kernel executions %d" % (s, plain[s]["frame_ms"], traced[s][0]["frame_ms"], plain[s]["general_kernel_executions"]))
    lines.append("sky pixels (depth == 0) of the frame: %.1f %%" % (100.0 * plain[1]["sky_pixel_share"]))
    k0, k1 = traced[0][1], traced[1][1]
    sky = {n: v for n, v in k1.items() if "skyAndSunSprite" in n}
    for n, (calls, ns) in sky.items():
        lines.append("sky kernel %s: %d calls, %.2f us per call" % (short(n), calls, ns / calls / 1e3))
    lines.append("kernels of run_sky = 1 without the sky kernel equal those of run_sky = 0 (names and calls): %s"
                 % ({n: c for n, (c, _) in k1.items() if n not in sky} == {n: c for n, (c, _) in k0.items()}))
    lines.append("no sky kernel with run_sky = 0: %s" % (not any("skyAndSunSprite" in n for n in k0)))
    if a.baseline_lib:
        rec_b, kb = run_child(-1, a.frames, True, lib=os.path.abspath(a.baseline_lib))
        same = {n: c for n, (c, _) in kb.items()} == {n: c for n, (c, _) in k0.items()}
        lines.append("baseline library: %.4f ms per frame under the tracer; kernel list of run_sky = 0 equals the baseline's (names and calls): %s" % (rec_b["frame_ms"], same))
        if not same:
            for n in sorted(set(kb) | set(k0)):
                if kb.get(n, (0, 0))[0] != k0.get(n, (0, 0))[0]:
                    lines.append("  %s: baseline %d calls, run_sky = 0 %d calls" % (short(n), kb.get(n, (0, 0))[0], k0.get(n, (0, 0))[0]))
    lines.append("kernels of run_sky = 0 (calls, us per call):")
    for n in sorted(k0):
        lines.append("  %-70s %6d %9.2f" % (short(n)[:70], k0[n][0], k0[n][1] / k0[n][0] / 1e3))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
