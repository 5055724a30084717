"""The fused upscale + deferred shade (kernels_fast/shading_fast.hip upscaleAndShadeKernel) leaves out work no output depends on: a wave without a geometry
pixel writes its sky colours and never resolves the GI upscale - only where the upscaled texels are neither stored (pass fusion level 2) nor signed (no
decision-signature run). Behind a switch, PLR_SHADE_SKY_EXIT (include/plr.h); it may not change a byte: every image the launch delivers is
compared with the switch on against off.

CPU: the switch parses. GPU: byte equality on crafted G-buffers, and the count of waves that took the exit against the count numpy expects - none where the
upscaled texels are stored or signed.

The frames are single launches of the pass pair (tests/passes.py gpu_upscale_and_shade), which has no temporal feedback of its own: "two frames" are two frame
indices, that is two noise textures and two by-position tap tables.

The albedo ramp among the G-buffers was made for the second change of the same work, the albedo's sRGB -> linear from a 256-entry table in LDS: bit-identical here
too, but not measurably faster and therefore not in the tree (profiles/r08_shade_sky_srgb.txt). The ramp stays: it costs nothing and holds any later decode to
every code."""
import numpy as np
import pytest

import passes
from plainrenderer_amd import backend as plr_backend
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.scene import Camera, GlobalShaderInfo
from util import light_buffer_bytes

LUT_RES = 32
SHADOW_RES = 256
SIZES = [(128, 64), (200, 70)]  # aligned; ragged: 200 % 64 = 8, 70 % 4 = 2 (both even, as the half-res chain requires)
KINDS = ["all_sky", "no_sky", "horizon", "checkerboard", "albedo_ramp"]
SPECIAL_CODES = [0, 1, 2, 10, 11, 255]  # both sides of the decode's `c <= 0.004045f` select (codes 1 | 2), 10 | 11, and the two ends
FRAME_INDICES = (3, 4)


# ------------------------------------------------------------------------------------------------------------------------ CPU: bookkeeping
def test_switch_parses(monkeypatch):
    monkeypatch.delenv("PLR_SHADE_SKY_EXIT", raising=False)
    assert plr_backend.shade_sky_exit_switch() is True, "on by default"
    monkeypatch.setenv("PLR_SHADE_SKY_EXIT", "0")
    assert plr_backend.shade_sky_exit_switch() is False
    for value in ("1", "", "00", "0 ", "off"):  # as PLR_SHADE_SKIP_UNLIT: only the string "0" is "off"
        monkeypatch.setenv("PLR_SHADE_SKY_EXIT", value)
        assert plr_backend.shade_sky_exit_switch() is True, repr(value)


# ------------------------------------------------------------------------------------------------------------------------ GPU: byte equality
def _depth_of(linear, cam):
    return ((cam.near * cam.far / np.asarray(linear, np.float64) - cam.near) / (cam.far - cam.near)).astype(np.float32)


class Frame:
    """one synthetic G-buffer of `kind` at w x h and everything else the pass pair reads"""

    def __init__(self, w, h, kind):
        self.w, self.h, self.kind = w, h, kind
        r = np.random.default_rng(1000 * w + h)
        self.cam = cam = Camera.look((16.0, -6.0, -5.0), (0.05, 0.2, 1.0), aspect=w / h)
        sun = np.array([0.35, -0.8, 0.45])
        self.sun = sun = sun / np.linalg.norm(sun)
        ys, xs = np.mgrid[0:h, 0:w]
        depth = _depth_of(6.0 + 0.15 * xs + 0.3 * ys + r.uniform(0.0, 3.0, (h, w)), cam)  # rough: the upscale's edge test goes both ways
        if kind == "all_sky":
            depth[:] = 0.0
        elif kind == "horizon":
            # rows 0 .. 9 of columns 0 .. 95 and rows 0 .. 29 of the rest: the edge at x = 96 cuts the segment 64 .. 127 in its middle, the one at y = 10 the block
            # of rows 8 .. 11, the one at y = 30 the block of rows 28 .. 31 - all-sky, mixed and all-geometry waves inside one block
            depth[(ys < 10) | ((xs >= 96) & (ys < 30))] = 0.0
        elif kind == "checkerboard":
            depth[((xs + ys) & 1) == 0] = 0.0
        albedo = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if kind == "albedo_ramp":
            for ch in range(3):  # every code in every channel, each channel with a phase of its own
                albedo[..., ch] = (xs * 7 + ys * 29 + ch * 85) % 256
            n = len(SPECIAL_CODES)
            albedo[0, 0:n, :3] = np.asarray(SPECIAL_CODES, np.uint8)[:, None]            # side by side in one wave, the same code in all channels
            for ch in range(3):
                albedo[1, 0:n, ch] = np.roll(np.asarray(SPECIAL_CODES, np.uint8), ch + 1)  # ... and a different one in each channel
        normal = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        normal[::2, :, :3] = np.array([172, 26, 185], np.uint8)  # every other row faces the sun: the albedo reaches the sun's lobes, not only the indirect term
        specular = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        self.gb = {"depth": depth, "normal": normal, "albedo": albedo, "specular": specular}
        sc = synth.SynthScene(grid=4, cell=8.0, seed_id=400)
        self.shadow_info = sc.shadow_cascades(cam, sun, 2.0, 60.0, 8, cascade_count=3)[0]
        my, mx = np.mgrid[0:SHADOW_RES, 0:SHADOW_RES]
        block = ((mx // 32) + (my // 32)) % 3
        self.shadow_maps = []
        for _ in range(4):
            noise = np.where(r.integers(0, 2, (SHADOW_RES, SHADOW_RES)) == 1, 0xffff, 0)
            self.shadow_maps.append(np.where(block == 0, 0xffff, np.where(block == 1, noise, 0)).astype(np.uint16))
        self.noise = synth.blue_noise_standins()
        self.sky = synth.sky_lut()
        self.froxel, self.froxel_dims = synth.froxel_volume(w, h, 16)
        self.vol_settings = synth.volumetric_settings_bytes(30.0)
        tw, th = w // 2, h // 2
        ysh = r.uniform(-0.2, 0.6, (th, tw, 4)).astype(np.float32) * 0.02
        ysh[..., 0] = np.abs(ysh[..., 0]) + 0.01
        self.half_ysh = pixfmt.pack_half(ysh)
        self.half_cocg = pixfmt.pack_half(r.uniform(-0.004, 0.004, (th, tw, 2)).astype(np.float32))
        self.half_depth = passes.orc_depth_downscale(depth, w, h)
        self.light = light_buffer_bytes(sun_color=(1.0, 0.92, 0.8), prev_exposure=8e-5, sun_strength_exposed=128000 * 8e-5)
        self.lut = passes.orc_brdf_lut(LUT_RES, 2)

    def sky_waves(self):
        """waves (64 x 1 pixel segments, the covered lanes of the last one) without a geometry pixel"""
        sky = self.gb["depth"] == 0
        return int(sum(sky[:, x0:x0 + 64].all(axis=1).sum() for x0 in range(0, self.w, 64)))

    def global_bytes(self, frame_index, noise_idx):
        g = GlobalShaderInfo(frameIndex=frame_index, sunDirection=(*self.sun.tolist(), 0.0))
        self.cam.fill_global(g, self.w, self.h)
        g.noiseTextureIndices = tuple(noise_idx)
        return g.pack()


_frames = {}


def _frame(w, h, kind):
    if (w, h, kind) not in _frames:
        _frames[(w, h, kind)] = Frame(w, h, kind)
    return _frames[(w, h, kind)]


def test_gbuffers_hold_what_they_are_for():
    for w, h in SIZES:
        waves_per_row = -(-w // 64)
        assert _frame(w, h, "all_sky").sky_waves() == waves_per_row * h
        assert _frame(w, h, "no_sky").sky_waves() == 0 and _frame(w, h, "checkerboard").sky_waves() == 0 and _frame(w, h, "albedo_ramp").sky_waves() == 0
        hz = _frame(w, h, "horizon")
        sky = hz.gb["depth"] == 0
        assert 0 < hz.sky_waves() < waves_per_row * h
        assert sky[8:10, 0:64].all() and not sky[10:12, 0:64].any(), "all-sky and all-geometry waves in the block of rows 8 .. 11"
        seg = sky[12, 64:128]
        assert seg.any() and not seg.all(), "a mixed wave"
        ramp = _frame(w, h, "albedo_ramp")
        geometry = ramp.gb["depth"] != 0
        assert geometry.all()
        for ch in range(3):
            assert set(np.unique(ramp.gb["albedo"][..., ch]).tolist()) == set(range(256)), "every code in channel %d" % ch
        assert ramp.gb["albedo"][0, 0:len(SPECIAL_CODES), 0].tolist() == SPECIAL_CODES
    assert 200 % 64 != 0 and 70 % 4 != 0


def _run(be, f, frame_index, noise_idx, mode):
    """one launch of the pair -> {image name: array}; mode: 'level2' | 'level1' | 'signature'"""
    args = (be, f.half_ysh, f.half_cocg, f.w // 2, f.h // 2, f.half_depth, f.gb, f.w, f.h, f.lut, LUT_RES, f.light, f.shadow_info, f.shadow_maps, SHADOW_RES, f.froxel,
            f.froxel_dims, f.vol_settings, f.sky, f.global_bytes(frame_index, noise_idx), 2, 0, True, 3)
    out = {}
    if mode == "level1":
        out["colour"], out["upscaled Y_SH"], out["upscaled CoCg"] = passes.gpu_upscale_and_shade(*args, download_upscaled=True)
    elif mode == "signature":
        with passes.gpu_signature(be, f.w * f.h) as sg:
            out["colour"] = passes.gpu_upscale_and_shade(*args)
        out["decision signature"] = sg.words.copy()
    else:
        out["colour"] = passes.gpu_upscale_and_shade(*args)
    assert be.getGeneralKernelExecutions()[0] == 0, be.getGeneralKernelExecutions()
    assert be.getPassFusion()[1] == 2, "one fused launch"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_sky_exit_changes_no_byte(backend, monkeypatch, w, h, kind):
    f = _frame(w, h, kind)
    _, noise_idx = passes.make_bindless(backend, [], 1, f.noise)
    monkeypatch.delenv("PLR_SHADE_SKY_EXIT", raising=False)
    backend.setMathMode(True)
    early = backend.getEarlyParts()[0]
    backend.setEarlyParts(0)
    backend.debugShadeSkyExitWaves(True)
    try:
        for mode in ("level2", "level1", "signature"):
            backend.setPassFusion(1 if mode == "level1" else 2)
            exits_expected = f.sky_waves() if mode == "level2" else 0  # stored or signed upscaled texels: the exit must not be taken
            for frame_index in FRAME_INDICES:
                results = {}
                for setting in ("on", "off"):
                    if setting == "off":
                        monkeypatch.setenv("PLR_SHADE_SKY_EXIT", "0")
                    results[setting] = _run(backend, f, frame_index, noise_idx, mode)
                    monkeypatch.delenv("PLR_SHADE_SKY_EXIT", raising=False)
                    waves = backend.debugShadeSkyExitWaves(True)  # reads, then zeroes
                    want = exits_expected if setting == "on" else 0
                    print("SKY_EXIT %dx%d %-12s %-9s frame %d switch %-3s: %d waves took the sky exit (expected %d)" % (w, h, kind, mode, frame_index, setting, waves, want), flush=True)
                    assert waves == want, "%s, switch %s: %d waves took the sky exit, %d have no geometry pixel and may" % (mode, setting, waves, want)
                on, off = results["on"], results["off"]
                assert on["colour"].dtype == np.uint32 and on["colour"].size == w * h
                assert set(on) == set(off) and len(on) == {"level2": 1, "level1": 3, "signature": 2}[mode]
                for name, image in on.items():
                    differing = int((image != off[name]).sum())
                    assert differing == 0, "%s, frame index %d: %s differs in %d words between PLR_SHADE_SKY_EXIT=0 and the default" % (mode, frame_index, name, differing)
    finally:
        backend.debugShadeSkyExitWaves(False)
        backend.setPassFusion(2)
        backend.setEarlyParts(early)
        backend.setMathMode(False)
