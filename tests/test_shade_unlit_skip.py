"""The deferred shade skips what the sun cannot light (kernels_fast/shading_fast.hip shadeDirect, "unlit pixels"): the PCF of a pixel whose
normal faces away from the sun, and the sun's lobes of a pixel that is back-facing or has all twelve taps shadowed. The skip multiplies nothing new by
zero - it leaves out products whose other factor is an exact zero - so the colour image is the same uint32 array with the skip, without it
(PLR_SHADE_SKIP_UNLIT=0) and in a decision-signature run (which always takes the full path).

CPU: the premise, in the oracle - the shadow maps cannot reach a back-facing pixel. GPU: bit identity of the three runs on a crafted frame."""
import numpy as np
import pytest

import passes
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.scene import Camera, GlobalShaderInfo
from util import light_buffer_bytes

VARIANTS = [(2, 0, True, 0, 3), (0, 1, False, 0, 3), (1, 2, True, 1, 4), (3, 3, True, 0, 1), (2, 0, False, 1, 2)]  # tests/test_shading.py's (brdf, multi, aa, tech, cascades)
LUT_RES = 32
SUN = np.array([0.35, -0.8, 0.45])


def _ndotl(normal_rgba8, sun):
    """dot(normalize(decoded 8-bit normal), normalize(sun)) in float64; the all-zero decode (no 8-bit texel has it) would be NaN"""
    raw = normal_rgba8[..., :3].astype(np.float64) / 255.0 * 2.0 - 1.0
    n = raw / np.linalg.norm(raw, axis=-1, keepdims=True)
    return n @ (np.asarray(sun, np.float64) / np.linalg.norm(sun))


def _view_vectors(cam, w, h):
    """surface -> camera unit vectors of the pixel centres (screenToWorld.inc)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (xs + 0.5) / w * 2 - 1, (ys + 0.5) / h * 2 - 1
    t = cam.tan_fov_half()
    d = np.asarray(cam.forward, np.float64) - t * ny[..., None] * np.asarray(cam.up, np.float64) + t * cam.aspect * nx[..., None] * np.asarray(cam.right, np.float64)
    return -d / np.linalg.norm(d, axis=-1, keepdims=True)


def _orc_bindless(noise, idx):
    import pyoracle as orc
    arr = (orc.OrcImage * (max(idx) + 1))()
    keep = []
    for nz, i in zip(noise, idx):
        im = orc.Img(np.ascontiguousarray(nz), 32, 32, passes.F.RG8)
        keep.append(im)
        arr[i] = im.c
    return arr, max(idx) + 1, keep


# ------------------------------------------------------------------------------------------------------------------------ CPU: the premise
def test_oracle_shadow_maps_cannot_reach_back_facing_pixels():
    w, h, res = 96, 40, 64
    sc = synth.SynthScene(grid=4, cell=8.0, seed_id=400)
    cam = Camera.look((16.0, -6.0, -5.0), (0.05, 0.2, 1.0), aspect=w / h)
    gb = sc.gbuffer(cam, w, h)
    sun = SUN / np.linalg.norm(SUN)
    shadow_info, _ = sc.shadow_cascades(cam, sun, 2.0, 60.0, 8)  # the matrices; the maps are replaced below
    g = GlobalShaderInfo(frameIndex=3, sunDirection=(*sun.tolist(), 0.0))
    cam.fill_global(g, w, h)
    noise = synth.blue_noise_standins()
    g.noiseTextureIndices = (0, 1, 2, 3)
    arr, n, keep = _orc_bindless(noise, [0, 1, 2, 3])
    r = np.random.default_rng(11)
    ysh = r.uniform(-0.2, 0.6, (h, w, 4)).astype(np.float32) * 0.02
    ysh[..., 0] = np.abs(ysh[..., 0]) + 0.01
    cocg = r.uniform(-0.004, 0.004, (h, w, 2)).astype(np.float32)
    froxel, froxel_dims = synth.froxel_volume(w, h, 16)
    lut = passes.orc_brdf_lut(LUT_RES, 2)
    light = light_buffer_bytes(sun_color=(1.0, 0.92, 0.8), prev_exposure=8e-5, sun_strength_exposed=128000 * 8e-5)

    def shade(texel):
        maps = [np.full((res, res), texel, np.uint16) for _ in range(4)]
        return passes.orc_deferred_shading(gb, w, h, lut, LUT_RES, light, shadow_info, maps, res, pixfmt.pack_half(ysh), pixfmt.pack_half(cocg), froxel, froxel_dims,
                                           synth.volumetric_settings_bytes(30.0), synth.sky_lut(), g.pack(), arr, n).reshape(h, w)
    lit, shadowed = shade(0), shade(0xffff)  # "actualDepth >= texel": every tap lit / every tap of a pixel inside a cascade shadowed
    geometry = gb["depth"] != 0
    ndotl = _ndotl(gb["normal"], sun)
    back, facing = geometry & (ndotl <= -1e-3), geometry & (ndotl >= 1e-3)
    assert back.sum() > 100 and facing.sum() > 100
    assert np.array_equal(lit[back], shadowed[back]), "a back-facing pixel does not depend on the shadow maps"
    # (a facing pixel outside every cascade reads the black border - lit - from either set of maps: a difference anywhere among the facing pixels is
    #  a difference at a pixel in range of a cascade)
    assert (lit[facing] != shadowed[facing]).any(), "the two sets of maps do differ where the sun can reach"
    assert np.array_equal(lit[~geometry], shadowed[~geometry])


# ------------------------------------------------------------------------------------------------------------------------ GPU: bit identity
W, H = 200, 70        # 3 whole 64-pixel waves and one of 8 per row; 17 whole block rows and one of 2
TW, TH = W // 2, H // 2
SHADOW_RES = 512
NEAR_PERPENDICULAR = 4e-7  # |NdotL| of the "perpendicular" rows: a few ulp of 1
ROWS_SEGMENTS, ROWS_CHECKER, ROWS_PERP, ROWS_RANDOM = slice(0, 16), slice(16, 32), slice(32, 44), slice(44, 70)


def _depth_of(linear, cam):
    return ((cam.near * cam.far / np.asarray(linear, np.float64) - cam.near) / (cam.far - cam.near)).astype(np.float32)


class Crafted:
    """A frame that is no scene: every class of pixel the skip distinguishes, side by side in the waves of a 200 x 70 launch.
    The sun (eps, t, t) is perpendicular to every normal (x, +1/255, -1/255): their NdotL is x * eps and some float32 rounding, either sign."""

    def __init__(self):
        r = np.random.default_rng(77)
        self.cam = cam = Camera.look((16.0, -6.0, -5.0), (0.05, 0.2, 1.0), aspect=W / H)
        self.sun = sun = np.array([1e-7, 0.5 ** 0.5, 0.5 ** 0.5])
        ys, xs = np.mgrid[0:H, 0:W]
        # ---- normals
        toward, away = np.array([128, 218, 218], np.uint8), np.array([127, 37, 37], np.uint8)
        nrm = np.zeros((H, W, 4), np.uint8)
        nrm[..., 3] = 255
        nrm[ROWS_SEGMENTS, :, :3] = away                       # whole 64-pixel segments facing away (and the partial wave of columns 192 ..)
        nrm[ROWS_SEGMENTS, 64:128, :3] = toward                # ... next to a whole segment that faces the sun
        chk = ((xs + ys) & 1).astype(bool)
        nrm[ROWS_CHECKER, :, :3] = np.where(chk[ROWS_CHECKER, :, None], toward, away)  # lane by lane
        perp = np.stack([(xs * 5 + ys * 37) % 256, np.where(xs & 1, 128, 127), np.where(xs & 1, 127, 128)], -1).astype(np.uint8)
        nrm[ROWS_PERP, :, :3] = perp[ROWS_PERP]
        nrm[ROWS_RANDOM, :, :3] = r.integers(0, 256, (H, W, 3), dtype=np.uint8)[ROWS_RANDOM]  # grazing view angles among them
        # ---- depth: a smooth surface; in the checkerboard rows every lane at a depth of its own - every cascade in one wave, and beyond the last split
        lin = 8.0 + 0.1 * xs + 0.2 * ys
        lin[ROWS_CHECKER] = r.choice([2.5, 9.0, 18.0, 25.0, 33.0, 42.0, 50.0, 58.0, 75.0, 140.0], (H, W))[ROWS_CHECKER]
        depth = _depth_of(lin, cam)
        depth[((xs * 7 + ys * 13) % 23 == 0) & (ys >= 16)] = 0.0  # sky holes
        depth[60:, 120:] = 0.0                                  # and whole waves of sky
        # ---- materials: 0 and 255 among random texels
        def texels():
            t = r.integers(0, 256, (H, W, 4), dtype=np.uint8)
            pick = r.integers(0, 4, (H, W, 4))
            t[pick == 0] = 0
            t[pick == 1] = 255
            return t
        self.gb = {"depth": depth, "normal": nrm, "albedo": texels(), "specular": texels()}
        # ---- shadow cascades: the matrices of a real fit, maps in 32 x 32 texel blocks: every tap shadowed | texel noise (penumbra) | every tap lit
        sc = synth.SynthScene(grid=4, cell=8.0, seed_id=400)
        self.shadow_info = {n: sc.shadow_cascades(cam, sun / np.linalg.norm(sun), 2.0, 60.0, 8, cascade_count=n)[0] for n in (1, 2, 3, 4)}
        my, mx = np.mgrid[0:SHADOW_RES, 0:SHADOW_RES]
        kind = ((mx // 32) + (my // 32)) % 3
        self.shadow_maps = []
        for _ in range(4):
            noise = np.where(r.integers(0, 2, (SHADOW_RES, SHADOW_RES)) == 1, 0xffff, 0)
            self.shadow_maps.append(np.where(kind == 0, 0xffff, np.where(kind == 1, noise, 0)).astype(np.uint16))
        g = GlobalShaderInfo(frameIndex=3, sunDirection=(*sun.tolist(), 0.0))
        cam.fill_global(g, W, H)
        self.g = g
        self.noise = synth.blue_noise_standins()
        self.sky = synth.sky_lut()
        self.froxel, self.froxel_dims = synth.froxel_volume(W, H, 16)
        self.vol_settings = synth.volumetric_settings_bytes(30.0)
        ysh = r.uniform(-0.2, 0.6, (H, W, 4)).astype(np.float32) * 0.02
        ysh[..., 0] = np.abs(ysh[..., 0]) + 0.01
        self.ysh = pixfmt.pack_half(ysh)
        self.cocg = pixfmt.pack_half(r.uniform(-0.004, 0.004, (H, W, 2)).astype(np.float32))
        self.half_ysh = pixfmt.pack_half(ysh[::2, ::2])
        self.half_cocg = pixfmt.pack_half(r.uniform(-0.004, 0.004, (TH, TW, 2)).astype(np.float32))
        self.half_depth = passes.orc_depth_downscale(depth, W, H)
        self.light = light_buffer_bytes(sun_color=(1.0, 0.92, 0.8), prev_exposure=8e-5, sun_strength_exposed=128000 * 8e-5)
        self.luts = {}
        # ---- what numpy knows about the pixels
        self.geometry = depth != 0
        self.ndotl = _ndotl(nrm, sun)
        self.nov = np.abs(np.einsum("ijk,ijk->ij", self._unit_normals(nrm), _view_vectors(cam, W, H)))
        self.linear = lin

    @staticmethod
    def _unit_normals(nrm):
        raw = nrm[..., :3].astype(np.float64) / 255.0 * 2.0 - 1.0
        return raw / np.linalg.norm(raw, axis=-1, keepdims=True)

    def lut(self, brdf):
        """the oracle's LUT with zero-energy texels: a block and a scatter (multiscattering 2 divides by the texel's .y)"""
        if brdf not in self.luts:
            t = passes.orc_brdf_lut(LUT_RES, brdf).reshape(LUT_RES, LUT_RES, 4).copy()
            t[:6, :10] = 0
            t[::5, ::3] = 0
            t[20:, 25:, 1] = 0
            self.luts[brdf] = t.reshape(-1)
        return self.luts[brdf]


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


def test_crafted_frame_has_every_pixel_class(crafted):
    """what does not depend on a GPU run (the lit-tap classes are asserted from the signature words, per run)"""
    c = crafted
    back, facing = c.geometry & (c.ndotl < 0), c.geometry & (c.ndotl > 0)
    assert W % 64 != 0 and H % 4 != 0
    assert back[ROWS_SEGMENTS, 0:64].all() and back[ROWS_SEGMENTS, 128:].all() and facing[ROWS_SEGMENTS, 64:128].all(), "whole segments, the partial wave among them"
    chk = c.ndotl[ROWS_CHECKER] > 0
    assert (chk[:, 1:] != chk[:, :-1]).all() and (np.abs(c.ndotl[ROWS_CHECKER]) > 0.9).all(), "per-lane checkerboard"
    near = c.geometry & (np.abs(c.ndotl) <= NEAR_PERPENDICULAR)
    assert (near & (c.ndotl > 0)).sum() > 50 and (near & (c.ndotl < 0)).sum() > 50 and near[ROWS_PERP][c.geometry[ROWS_PERP]].all(), "perpendicular on both sides"
    assert (~c.geometry).sum() > 500 and (~c.geometry)[60:, 128:192].all(), "sky holes and a wave of sky"
    for name, channels in (("albedo", (0, 1, 2)), ("specular", (1, 2))):
        for ch in channels:
            t = c.gb[name][..., ch][c.geometry]
            assert (t == 0).any() and (t == 255).any(), (name, ch)
    assert (c.geometry & (c.nov < 0.02)).sum() >= 5, "grazing view angles"
    assert (c.linear[ROWS_CHECKER] > 60.0).any(), "beyond the far end of the last cascade's fit"


def _assert_coverage(c, words, cascades):
    words = words.reshape(H, W) & 0xff
    assert np.array_equal((words & 128) != 0, ~c.geometry) and ((words & 64) != 0)[c.geometry].all()
    lit = (words >> 2) & 15
    facing, back = c.geometry & (c.ndotl > 1e-3), c.geometry & (c.ndotl < -1e-3)
    for name, mask in (("facing", facing), ("back-facing", back)):
        assert (lit[mask] == 0).any() and (lit[mask] == 12).any() and ((lit[mask] > 0) & (lit[mask] < 12)).any(), "%s pixels: all shadowed, all lit, penumbra" % name
    seg = (words & 3)[ROWS_CHECKER, 0:64]
    ok = c.geometry[ROWS_CHECKER, 0:64]
    assert any(set(np.unique(row[m]).tolist()) == set(range(cascades)) for row, m in zip(seg, ok)), "every cascade inside one wave"
    assert ((words & 3)[c.geometry & (c.linear > 60.0)] == cascades - 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("brdf,multi,aa,tech,cascades", VARIANTS)
def test_gpu_unlit_skip_is_bit_identical(backend, crafted, monkeypatch, brdf, multi, aa, tech, cascades):
    c = crafted
    _, noise_idx = passes.make_bindless(backend, [], 1, c.noise)
    c.g.noiseTextureIndices = tuple(noise_idx)
    common = (c.gb, W, H, c.lut(brdf), LUT_RES, c.light, c.shadow_info[cascades], c.shadow_maps, SHADOW_RES)
    tail = (c.froxel, c.froxel_dims, c.vol_settings, c.sky, c.g.pack())

    def shade():
        out = passes.gpu_deferred_shading(backend, *common, c.ysh, c.cocg, *tail, brdf, multi, aa, tech, cascades)
        assert backend.getGeneralKernelExecutions()[0] == 0, backend.getGeneralKernelExecutions()
        return out

    def fused():
        out = passes.gpu_upscale_and_shade(backend, c.half_ysh, c.half_cocg, TW, TH, c.half_depth, *common, *tail, brdf, multi, aa, cascades)
        assert backend.getGeneralKernelExecutions()[0] == 0, backend.getGeneralKernelExecutions()
        assert backend.getPassFusion() == (2, 2), "one fused launch"
        return out

    backend.setMathMode(True)
    early = backend.getEarlyParts()[0]
    try:
        for name, run in (("deferred shade", shade), ("upscale + shade", fused)):
            monkeypatch.setenv("PLR_SHADE_SKIP_UNLIT", "0")
            full = run()
            monkeypatch.delenv("PLR_SHADE_SKIP_UNLIT")
            skipping = run()
            with passes.gpu_signature(backend, W * H) as sg:
                signed = run()
            _assert_coverage(c, sg.words, cascades)
            assert full.dtype == np.uint32 and full.size == W * H
            differing = int((full != skipping).sum())
            print("UNLIT_SKIP %-16s brdf %d multi %d aa %d tech %d cascades %d: %d of %d words differ between PLR_SHADE_SKIP_UNLIT=0 and the default, %d between the "
                  "signature run and the default" % (name, brdf, multi, aa, tech, cascades, differing, full.size, int((signed != skipping).sum())), flush=True)
            assert np.array_equal(full, skipping), "%s: the skip changes the colour image" % name
            assert np.array_equal(signed, skipping), "%s: the decision-signature run's colour image differs" % name
        # the pair as two launches (the direct lighting as the early part: shadeDirectKernel), with and without the skip
        backend.setEarlyParts(2)
        monkeypatch.setenv("PLR_SHADE_SKIP_UNLIT", "0")
        full = fused()
        assert backend.getEarlyParts() == (2, 1), "direct lighting launched as the early part"
        monkeypatch.delenv("PLR_SHADE_SKIP_UNLIT")
        skipping = fused()
        assert backend.getEarlyParts() == (2, 1)
        assert np.array_equal(full, skipping), "two launches: the skip changes the colour image"
    finally:
        backend.setEarlyParts(early)
        backend.setMathMode(False)
