"""Child process of tests/test_backend_restart.py: for every size on the command line (WxH), one after the other on the main thread, a backend is set up, switched
to the fast kernel set (pass fusion at its default), renders five frames of test_live_resize.py's synthetic scene - five: each of the four rotating noise textures
comes round again - and is shut down. Prints a SHA-256 of every output after every frame, and what the shade's decision-signature words of one more frame say."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from plainrenderer_amd import RenderBackend, synth  # noqa: E402
from plainrenderer_amd.backend import PlrError  # noqa: E402
from plainrenderer_amd.frame import FramePipeline, SyntheticInputs  # noqa: E402
from plainrenderer_amd.scene import Camera  # noqa: E402

OPTS = dict(shadow_map_res=256, brdf_lut_res=32, froxel_depth=16, max_sdf_instances=64)
IMAGES = ("color0", "color1", "post1", "swapchain", "giHistoryYSH0", "giHistoryYSH1", "giHistoryCoCg0", "giHistoryCoCg1", "giFullResYSH", "giFullResCoCg")
FRAMES = 5


def camera(f, w, h):
    return Camera.look((15.0 + 0.03 * f, -7.0, -6.0 + 0.05 * f), (0.0, 0.16, 1.0), aspect=w / h)


def frame(fp, f, w, h):
    fp.frame(camera(f + 1, w, h), 1.0 / 60.0, 0.5 + f / 60.0)


def digest(be, fp, name):
    """an intermediate a fused launch kept in registers (pass fusion level 2) cannot be read"""
    try:
        return hashlib.sha256(be.downloadImage(fp.image(name), 0, np.uint8).tobytes()).hexdigest()
    except PlrError as e:
        if "was not written in the last frame" not in str(e):
            raise
        return "unwritten"


scene = synth.SynthScene(grid=4, cell=8.0, seed_id=702)
for rnd, size in enumerate(sys.argv[1:]):
    w, h = (int(v) for v in size.split("x"))
    be = RenderBackend(w, h, device=0)
    be.setMathMode(True)
    fp = FramePipeline(be, w, h, **OPTS)
    SyntheticInputs(scene, camera(1, w, h), camera(0, w, h), w, h, sdf_res=16, shadow_res=256, froxel_depth=16, sun_direction=(0.35, -0.8, 0.45)).upload(fp)
    for f in range(FRAMES):
        frame(fp, f, w, h)
        general = be.getGeneralKernelExecutions()[0]
        for name in IMAGES:
            print("round %d frame %d %s %s" % (rnd, f, name, digest(be, fp, name)))
        hist = be.downloadStorageBuffer(fp.storage_buffer("histogram"), 512)
        print("round %d frame %d histogram %s" % (rnd, f, hashlib.sha256(hist.tobytes()).hexdigest()))
        print("round %d frame %d general-kernel-executions %d" % (rnd, f, general))
    colours = [np.unique(be.downloadImage(fp.image(n), 0, np.uint32)).size for n in ("color0", "color1")]
    # one more frame with the decision signatures on: the shade is the last pass that writes them, one word per pixel (bit 7 sky, bit 6 geometry, bits 2..5 the
    # number of lit PCF taps of 12)
    be.setDecisionSignature(w * h)
    frame(fp, FRAMES, w, h)
    words = be.readDecisionSignature(w * h) & 0xff
    be.setDecisionSignature(0)
    lit = (words[(words & 64) != 0] >> 2) & 15
    print("round %d content distinct-colours %d sky %d lit %d shadowed %d penumbra %d" % (rnd, min(colours), int(((words & 128) != 0).sum()), int((lit == 12).sum()),
                                                                                        int((lit == 0).sum()), int(((lit > 0) & (lit < 12)).sum())))
    fp.destroy()
    be.shutdown()
