"""A backend shut down and set up again inside one process, on one thread (plr_shutdown followed by plr_setup is supported): what a pass's launcher remembers about
its scratch memory must go with the backend that owned the memory. The new backend's passes and their scratch may come back at the addresses just freed, with the
same sizes; a launcher that still took its derived tables (the shade's PCF tap table, the spatial filter's sample tables, the histogram's thresholds) for built
would render from zero-filled memory. The restart happens in a child process (tests/backend_restart_child.py): the suite's own backend is one per session."""
import os
import re
import subprocess
import sys

import pytest

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "backend_restart_child.py")
OUTPUTS = 11  # ten images and the histogram buffer
FRAMES = 5


def run(sizes):
    """-> per round: (the lines of its five frames, its content line)"""
    p = subprocess.run([sys.executable, CHILD] + sizes, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rounds = []
    for r in range(len(sizes)):
        frames = [l.split(" ", 2)[2] for l in p.stdout.splitlines() if l.startswith("round %d frame " % r)]
        content = [l for l in p.stdout.splitlines() if l.startswith("round %d content " % r)]
        assert len(frames) == FRAMES * (OUTPUTS + 1) and len(content) == 1, p.stdout
        rounds.append((frames, content[0]))
    return rounds


@pytest.mark.gpu
def test_gpu_restarted_backend_renders_what_a_fresh_one_renders():
    first, second, third = run(["256x144", "323x183", "256x144"])
    (fresh,) = run(["323x183"])
    for frames, content in (first, second, third, fresh):
        # the fast kernel set rendered every frame, and the frames are not trivial: a colour buffer of many values, sky and geometry, and among the geometry
        # pixels fully lit ones, fully shadowed ones and a penumbra (taps that all sit on the pixel - a zeroed tap table - give 0 or 12 lit taps, never between)
        assert all(l.endswith(" 0") for l in frames if "general-kernel-executions" in l), frames
        assert not any("unwritten" in l for l in frames if re.match(r"frame \d (color|post1|swapchain|histogram)", l)), frames  # (only a GI intermediate may be)
        n = dict(zip(content.split()[3::2], (int(v) for v in content.split()[4::2])))
        assert n["distinct-colours"] > 16 and n["sky"] > 0 and n["lit"] > 0 and n["shadowed"] > 0 and n["penumbra"] > 0, content
    assert third[0] == first[0], "the third backend of the process (same size as the first) renders something else than the first"
    assert third[1].split(" ", 2)[2] == first[1].split(" ", 2)[2]
    assert second[0] == fresh[0], "the second backend of a process renders something else than the first backend of a fresh process at the same size"
    assert second[1].split(" ", 2)[2] == fresh[1].split(" ", 2)[2]
