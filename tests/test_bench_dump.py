"""bench.py --dump-outputs: after the timed steps the benchmark writes what its last timed frame computed (float arrays, at most 64 MB, a seeded pixel
sample of the 4K frame). Two runs with the same arguments get the same inputs, so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--profile-frames", "0", "--no-cpu-baseline"]
NAMES = ["histogram.npy", "light.npy", "pixel_index.npy", "post1_rgb.npy", "swapchain.npy"]


def _bench(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_frame_the_same_way_every_run(tmp_path):
    runs = []
    for name in ("a", "b"):
        line = _bench(tmp_path / name)
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert sorted(os.listdir(tmp_path / name)) == NAMES
        assert sum(os.path.getsize(tmp_path / name / f) for f in NAMES) <= 64 << 20
        runs.append({f[:-4]: np.load(tmp_path / name / f) for f in NAMES})
    a, b = runs
    w, h = line["config"]["resolution"]
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
    idx = a["pixel_index"]
    assert idx.size == 1 << 20 and np.array_equal(idx, np.unique(idx)) and idx[0] >= 0 and idx[-1] < w * h
    assert a["swapchain"].shape == (idx.size, 4) and a["post1_rgb"].shape == (idx.size, 3)
    assert int(a["histogram"].sum()) == w * h
    assert np.isfinite(a["post1_rgb"]).all() and a["post1_rgb"].max() > 0 and a["swapchain"][:, :3].max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s differs between two runs with the same arguments" % k
