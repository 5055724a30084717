"""Inputs of the deferred shade's reference tests (tests/test_shade_reference_cpu.py, tests/test_shade_reference.py): named G-buffers of a few thousand pixels, the
smallest at which the shade can still go wrong, each with a check, on the reference alone (tests/shade_reference.py), that it is what it is for. Sizes are
256 x 8n or 128 x 8n: whole 64 x 4 shade blocks and 128 x 8 quad blocks, even, so the upscale + shade pair fuses.

Every case: a `Camera.look` camera, a depth plane or ramp, the real 32 x 32 BRDF LUT of the variant's diffuse model (passes.orc_brdf_lut), synth.froxel_volume,
the four noise stand-ins, 1 to 4 cascades. Nothing is out of range, no input is non-finite, no case exists to provoke a fault.

  material_lattice        256 x 48: columns = roughness codes 0 .. 255 (0 .. 17 decode onto the max(r * r, 0.0045) floor), rows = metalness codes {0, 1, 127, 128,
                          254, 255} x albedo codes {0, 1, 2, 10, 11, 128, 254, 255} (1 | 2: the two sides of the shader's `<= 0.004045` select; 10 | 11: the two
                          sides of the textbook knee 0.04045, which the shader does not have). Per pixel a normal between camera and sun, 15 degrees off the half vector.
  mirror_highlight        256 x 16: per pixel the 8-bit normal closest to normalize(V + L), so NoH -> 1; column groups = roughness codes 0 .. 20, 32, 64, 128, row
                          groups = metalness 0 | 255. (Geometric AA on and off: the variants.) A dimmer sun: D reaches 1 / (pi r^2) = 15 719 here.
  grazing_and_terminator  128 x 40, a metal with roughness code 0 | 128. Rows 0-7: columns step |N.V| from 0.05 through the 1e-4 floor; rows 8-23: rows step N.L across 0
                          and back, never within 1e-3 of it; rows 24-39: sun-facing and back-facing normals alternate per pixel, per row and per 64 x 4 block.
  cascades_and_taps       128 x 32, an axis-aligned camera with near 1, far 257: a depth ramp over the rows crosses the splits 8, 16, 32 with 3 % to spare - and two
                          pixels whose depth 249 / 2048 linearises to the split 8 in exact arithmetic (every operation on the way is exact in fp32 and float64), so
                          `>=` and `>` differ there. Cascade 0 reads a map with a straight edge (lit | shadowed), 1 an all-shadowed map under a matrix whose depth
                          runs past 1 (clamped onto the texel's 1.0: lit by `>=` alone), 2 an all-lit map, 3 an all-shadowed map most pixels project outside of
                          (the black border: lit). A pixel with a tap closer than TAP_TEXEL_MARGIN texels to a texel boundary behind which the map differs, or with
                          an unclamped depth within TAP_DEPTH_MARGIN of its texel, is made a sky pixel: the lit-tap count of every other is unambiguous.
  fog_and_indirect        128 x 96 (the noise moves the froxel UV by at most 0.0065: with fewer than 77 rows that is less than half a pixel): pixelDepth from a sixth of the fog's maxDistance to twice it, one row group at it; noise offsets that carry the froxel UV across all
                          four borders; column groups = SH texels with a dominant direction of length 0, 0.005, 0.5, 1.5; CoCg of both signs; sky pixels inside quads.
                          (Indirect technique 0 and 1: the variants.)

NOT_FINITE lists the (case, variant) pairs that are not run because the reference is not finite there, with the reason.
"""
import struct

import numpy as np

import passes
import shade_reference as sr
from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.scene import Camera, GlobalShaderInfo
from util import light_buffer_bytes

LUT_RES = 32
SHADOW_RES = 64
SUN = np.array([0.35, -0.8, -0.45])
SPLIT_MARGIN = 1e-3        # relative distance of every pixelDepth to every split (but the two exact ties of cascades_and_taps)
TAP_TEXEL_MARGIN = 1e-3    # texels
TAP_DEPTH_MARGIN = 1e-2
NDOTL_MARGIN = 1e-3
ROUGHNESS_FLOOR_CODES = 18  # (17 / 255)^2 = 0.00444 < 0.0045 <= (18 / 255)^2
MIRROR_ROUGHNESS = list(range(21)) + [32, 64, 128]
LATTICE_METAL = (0, 1, 127, 128, 254, 255)
LATTICE_ALBEDO = (0, 1, 2, 10, 11, 128, 254, 255)
NOT_FINITE = {}            # (case name, variant) -> reason. Empty: every reference value of every case x variant is finite (asserted by the CPU test)

_luts = {}


def lut(brdf):
    if brdf not in _luts:
        _luts[brdf] = passes.orc_brdf_lut(LUT_RES, brdf)
    return _luts[brdf]


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def view_vectors(cam, w, h):
    """surface -> camera unit vectors of the pixel centres (screenToWorld.inc)"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (xs + 0.5) / w * 2 - 1, (ys + 0.5) / h * 2 - 1
    t = cam.tan_fov_half()
    f, u, r = (np.asarray(a, np.float64) for a in (cam.forward, cam.up, cam.right))
    return unit(-f + t * ny[..., None] * u - t * cam.aspect * nx[..., None] * r)


def depth_of(linear, cam):
    return ((cam.near * cam.far / np.asarray(linear, np.float64) - cam.near) / (cam.far - cam.near)).astype(np.float32)


def decode_normals(codes):
    return unit(codes.astype(np.float64) / 255.0 * 2.0 - 1.0)


def search_codes(target, cost, radius=2):
    """per pixel the 8-bit normal texel, among those within `radius` codes of the rounded target, whose decoded unit normal has the smallest cost(N [..., k, 3])"""
    base = np.rint((unit(target) * 0.5 + 0.5) * 255.0).astype(np.int64)
    o = np.arange(-radius, radius + 1)
    offsets = np.stack(np.meshgrid(o, o, o, indexing="ij"), -1).reshape(-1, 3)
    cand = np.clip(base[..., None, :] + offsets, 0, 255)
    best = np.argmin(cost(decode_normals(cand)), axis=-1)
    return np.take_along_axis(cand, best[..., None, None], axis=-2)[..., 0, :].astype(np.uint8)


def ortho_light(rows):
    """ShadowCascadeInfo's matrix from the three rows (a, b, c, d): light-space x, y, z = a X + b Y + c Z + d of the world position; [column][row] as glm stores it"""
    m = np.zeros((4, 4))
    m[:3] = np.asarray(rows, np.float64)
    m[3, 3] = 1.0
    return np.ascontiguousarray(m.T.astype(np.float32))


def shadow_info_bytes(splits, matrices, scales):
    b = struct.pack("<4f", *splits)
    for m in matrices:
        b += np.asarray(m, np.float32).tobytes()
    for s in scales:
        b += struct.pack("<2f", *s)
    assert len(b) == 304
    return b


class Case:
    """One G-buffer with everything the shade reads. `args(brdf, noise_idx)` are the arguments of passes.*_deferred_shading up to the global block."""

    def __init__(self, name, w, h, cam, sun=SUN, splits=(10.0, 25.0, 45.0, 0.0), sun_strength_exposed=10.24, max_distance=30.0):
        self.name, self.w, self.h, self.cam = name, w, h, cam
        self.sun = unit(sun)
        self.V = view_vectors(cam, w, h)
        self.ys, self.xs = np.mgrid[0:h, 0:w]
        r = np.random.default_rng(1200 + sum(name.encode()))
        self.rng = r
        self.gb = {"depth": depth_of(np.full((h, w), 12.0), cam), "normal": np.zeros((h, w, 4), np.uint8), "albedo": np.full((h, w, 4), 180, np.uint8),
                   "specular": np.full((h, w, 4), 255, np.uint8)}
        self.gb["specular"][..., 1], self.gb["specular"][..., 2] = 128, 0
        self.gb["normal"][..., 3] = 255
        # one light matrix for every cascade that keeps every pixel inside an all-lit map, mid depth
        m = ortho_light([(0.004, 0, 0, 0), (0, 0.004, 0, 0), (0, 0, 0, 0.5)])
        self.shadow_info = shadow_info_bytes(splits, [m] * 4, [(1.0, 1.0)] * 4)
        self.shadow_maps = [np.zeros((SHADOW_RES, SHADOW_RES), np.uint16) for _ in range(4)]
        ysh = np.zeros((h, w, 4), np.float32)
        ysh[..., 0] = 0.02 + 0.01 * r.random((h, w))
        ysh[..., 1:] = r.uniform(-0.004, 0.004, (h, w, 3))
        self.ysh = pixfmt.pack_half(ysh)
        self.cocg = pixfmt.pack_half(r.uniform(-0.001, 0.001, (h, w, 2)).astype(np.float32))
        self.froxel, self.froxel_dims = synth.froxel_volume(w, h, 16)
        self.vol_settings = synth.volumetric_settings_bytes(max_distance)
        self.light = light_buffer_bytes(sun_color=(1.0, 0.92, 0.8), prev_exposure=8e-5, sun_strength_exposed=sun_strength_exposed)
        self.noise = synth.blue_noise_standins()
        self.sky = synth.sky_lut()
        self.g = GlobalShaderInfo(frameIndex=3, sunDirection=(*self.sun.tolist(), 0.0))
        cam.fill_global(self.g, w, h)

    def global_packed(self, noise_idx=(0, 1, 2, 3)):
        self.g.noiseTextureIndices = tuple(noise_idx)
        return self.g.pack()

    def args(self, brdf, noise_idx=(0, 1, 2, 3)):
        return (self.gb, self.w, self.h, lut(brdf), LUT_RES, self.light, self.shadow_info, self.shadow_maps, SHADOW_RES, self.ysh, self.cocg, self.froxel, self.froxel_dims,
                self.vol_settings, self.sky, self.global_packed(noise_idx))

    def noise_by_index(self, noise_idx=(0, 1, 2, 3)):
        return {i: t for i, t in zip(noise_idx, self.noise)}

    def reference(self, variant, noise_idx=(0, 1, 2, 3), **kw):
        return sr.shade(*self.args(variant[0], noise_idx), self.noise_by_index(noise_idx), *variant, **kw)

    def common_check(self, ref, variant):
        """what every case promises: finite reference values, no ambiguous discrete decision"""
        geo = ~ref.sky
        assert geo.sum() >= 0.8 * geo.size
        assert np.isfinite(ref.rgb[geo]).all() and np.isfinite(ref.slack[geo]).all(), self.name
        d = ref.diag
        ties = getattr(self, "split_ties", np.zeros_like(geo))
        assert (d["split_margin"][geo & ~ties] >= SPLIT_MARGIN).all(), "a pixelDepth too close to a split"
        assert (d["tap_texel_margin"][geo] >= TAP_TEXEL_MARGIN).all() and (d["tap_depth_margin"][geo] >= TAP_DEPTH_MARGIN).all(), "an ambiguous PCF tap"
        assert (np.abs(d["NdotL"][geo]) >= NDOTL_MARGIN).all(), "a normal too close to the terminator"


def _default_cam(w, h):
    """tests/test_shading.py's camera; the aspect ratio is the global block's, not the image's: the strips stay inside a 60 degree field of view"""
    return Camera.look((16.0, -6.0, -5.0), (0.05, 0.2, 1.0), aspect=16.0 / 9.0)


# ------------------------------------------------------------------------------------------------------------------------ material_lattice
def _material_lattice():
    w, h = 256, 48
    c = Case("material_lattice", w, h, _default_cam(w, h))
    half = unit(c.V + c.sun)
    side = unit(np.cross(half, c.sun))
    n = unit(np.cos(np.radians(15.0)) * half + np.sin(np.radians(15.0)) * side)
    c.gb["normal"][..., :3] = np.rint((n * 0.5 + 0.5) * 255.0).astype(np.uint8)
    c.gb["specular"][..., 1] = c.xs
    c.gb["specular"][..., 2] = np.asarray(LATTICE_METAL, np.uint8)[c.ys // len(LATTICE_ALBEDO)]
    c.gb["albedo"][..., :3] = np.asarray(LATTICE_ALBEDO, np.uint8)[c.ys % len(LATTICE_ALBEDO)][..., None]

    def check(ref, variant):
        c.common_check(ref, variant)
        aa_off = ref if not variant[2] else c.reference((*variant[:2], False, *variant[3:]), want_slack=False)
        r = aa_off.diag["r"]
        assert (r[:, :ROUGHNESS_FLOOR_CODES] == np.float64(np.float32(0.0045))).all() and (r[:, ROUGHNESS_FLOOR_CODES:] > 0.0045).all(), "codes 0 .. 17 sit on the floor"
        assert np.allclose(r[:, ROUGHNESS_FLOOR_CODES:], (np.arange(ROUGHNESS_FLOOR_CODES, 256) / 255.0) ** 2, rtol=1e-12)
        assert sorted(set(np.rint(ref.diag["metalic"] * 255).astype(int).reshape(-1).tolist())) == sorted(LATTICE_METAL)
        lo = ref.diag["albedo"][..., 0]
        assert np.allclose(lo[c.gb["albedo"][..., 0] == 1], 1 / 255.0 / np.float64(np.float32(12.92))) and (lo[c.gb["albedo"][..., 0] == 2] > 2 / 255.0 / 12.0).all(), "1 | 2: the select"
        assert len(np.unique(c.gb["albedo"][..., 0])) == len(LATTICE_ALBEDO)
        assert (ref.diag["NdotL"] > 0.3).all() and (np.abs(ref.diag["NdotV"]) > 0.3).all() and (ref.diag["NdotH"] > 0.9).all() and (ref.diag["NdotH"] < 0.985).all()
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------------------------------ mirror_highlight
def _mirror_highlight():
    w, h = 256, 16
    c = Case("mirror_highlight", w, h, _default_cam(w, h), sun_strength_exposed=1.0)
    half = unit(c.V + c.sun)
    c.gb["normal"][..., :3] = search_codes(half, lambda n: -(n * half[..., None, :]).sum(-1), radius=1)
    group = c.xs * len(MIRROR_ROUGHNESS) // w
    c.gb["specular"][..., 1] = np.asarray(MIRROR_ROUGHNESS, np.uint8)[group]
    c.gb["specular"][..., 2] = np.where((c.ys // 4) % 2 == 0, 0, 255)
    c.floor_columns = np.asarray(MIRROR_ROUGHNESS)[group] < ROUGHNESS_FLOOR_CODES
    c.well_columns = np.asarray(MIRROR_ROUGHNESS)[group] >= 64

    def check(ref, variant):
        c.common_check(ref, variant)
        aa_off = ref if not variant[2] else c.reference((*variant[:2], False, *variant[3:]), want_slack=False)
        r, noh = aa_off.diag["r"], aa_off.diag["NdotH"]
        assert sorted(set(c.gb["specular"][..., 1].reshape(-1).tolist())) == MIRROR_ROUGHNESS
        assert (r[c.floor_columns] == np.float64(np.float32(0.0045))).all()
        peak = noh[c.floor_columns] > 1.0 - 2.0 * r[c.floor_columns] ** 2
        assert peak.mean() >= 0.1, "NoH exceeds 1 - 2 r^2 on %.3f of the floor columns' pixels" % peak.mean()
        assert set(np.unique(c.gb["specular"][..., 2]).tolist()) == {0, 255}
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------------------------------ grazing_and_terminator
GRAZING_ROWS, TERMINATOR_ROWS, PER_PIXEL_ROWS, PER_ROW_ROWS, PER_BLOCK_ROWS = slice(0, 8), slice(8, 24), slice(24, 28), slice(28, 32), slice(32, 40)
TERMINATOR_STEPS = (0.05, 0.003, -0.003, -0.05, -0.05, -0.003, 0.003, 0.05)   # per quad row


def _per_pixel(codes):
    return np.repeat(np.repeat(codes, 2, axis=0), 2, axis=1)


def _grazing_and_terminator():
    w, h = 128, 40
    c = Case("grazing_and_terminator", w, h, _default_cam(w, h))
    V, L = c.V, c.sun
    c.gb["specular"][..., 1] = np.where((c.ys // 2) % 2 == 0, 0, 128)
    c.gb["specular"][..., 2] = 255
    c.gb["albedo"][..., :3] = 200
    qx = c.xs[::2, ::2] / 2
    qy = c.ys[::2, ::2] // 2
    # rows 0-7, a normal texel per pixel: N = a V + sqrt(1 - a^2) T, T the unit vector perpendicular to V in the plane of V and L (so the sun lights the pixel).
    # The texel is searched within ONE code of the rounded target: a wider search reaches the floor more often, but neighbours then differ by several codes, the
    # geometric AA lifts the roughness of code 0 to ~0.045 - between the LUT's first two columns, its steepest - and a 1 / 256 weight step is whole codes there
    T = unit(L - (V @ L)[..., None] * V)
    a = (0.05 * (2e-5 / 0.05) ** (c.xs / (w - 1.0)))[..., None]
    target = a * V + np.sqrt(1.0 - a * a) * T
    cost = lambda n: np.abs((n * V[..., None, :]).sum(-1) - a) + 10.0 * ((n @ L) < 0.2)
    c.gb["normal"][GRAZING_ROWS, :, :3] = search_codes(target, cost, radius=1)[GRAZING_ROWS]
    # rows 8-23, a normal texel per quad (the geometric AA's differences are zero there: the roughness stays the texel's):
    # N = b L + sqrt(1 - b^2) U, U perpendicular to L and turned about it from column to column
    u0 = unit(np.cross(L, [0.0, 1.0, 0.0]))
    u1 = np.cross(L, u0)
    phi = (qx / (w / 2) * 2.0 * np.pi)[..., None]
    U = np.cos(phi) * u0 + np.sin(phi) * u1
    b = np.asarray(TERMINATOR_STEPS)[np.clip(qy - 4, 0, 7)][..., None]
    target = b * L + np.sqrt(1.0 - b * b) * U
    cost = lambda n: np.abs((n @ L) - b) + 10.0 * ((np.abs(n @ L) < 1.5 * NDOTL_MARGIN) | (np.sign(n @ L) != np.sign(b)))
    c.gb["normal"][TERMINATOR_ROWS, :, :3] = _per_pixel(search_codes(target, cost, radius=3))[TERMINATOR_ROWS]
    # rows 24-39: lit | back-facing per pixel, per row, per 64 x 4 block
    toward = np.rint((unit(L + 0.3 * V[h // 2, w // 2]) * 0.5 + 0.5) * 255.0).astype(np.uint8)
    away = (255 - toward.astype(np.int64)).astype(np.uint8)
    lit = np.zeros((h, w), bool)
    lit[PER_PIXEL_ROWS] = ((c.xs + c.ys) % 2 == 0)[PER_PIXEL_ROWS]
    lit[PER_ROW_ROWS] = (c.ys % 2 == 0)[PER_ROW_ROWS]
    lit[PER_BLOCK_ROWS] = ((c.xs // 64 + c.ys // 4) % 2 == 0)[PER_BLOCK_ROWS]
    c.gb["normal"][24:, :, :3] = np.where(lit[24:, :, None], toward, away)
    c.lit_pattern = lit

    def check(ref, variant):
        c.common_check(ref, variant)
        nov = np.abs(ref.diag["NdotV"][GRAZING_ROWS])
        for lo, hi in ((1e-2, 0.06), (1e-3, 1e-2), (1e-4, 1e-3), (0.0, 1e-4)):
            assert ((nov >= lo) & (nov < hi)).sum() >= 24, "|N.V| in [%g, %g): %d pixels" % (lo, hi, ((nov >= lo) & (nov < hi)).sum())
        assert (ref.diag["NdotL"][GRAZING_ROWS] > 0.2).all()
        ndl = ref.diag["NdotL"][TERMINATOR_ROWS]
        steps = np.repeat(np.asarray(TERMINATOR_STEPS), 2)
        assert (np.sign(ndl) == np.sign(steps)[:, None]).all() and (np.abs(ndl) >= NDOTL_MARGIN).all()
        assert (np.abs(ndl[np.abs(steps) < 0.01]) < 6e-3).all(), "the rows next to the terminator are within 6e-3 of it"
        ndl = ref.diag["NdotL"][24:]
        assert ((ndl > 0.5) == c.lit_pattern[24:]).all() and (np.abs(ndl) > 0.5).all()
        p = c.lit_pattern
        assert (p[PER_PIXEL_ROWS][:, 1:] != p[PER_PIXEL_ROWS][:, :-1]).all(), "mixed waves"
        assert (p[PER_ROW_ROWS] == p[PER_ROW_ROWS][:, :1]).all() and (p[28] != p[29]).all(), "uniform waves, mixed blocks"
        assert all(len(np.unique(p[y:y + 4, x:x + 64])) == 1 for y in (32, 36) for x in (0, 64)) and p[32, 0] != p[32, 64] and p[32, 0] != p[36, 0], "uniform blocks"
        assert set(np.unique(c.gb["specular"][..., 1]).tolist()) == {0, 128}
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------------------------------ cascades_and_taps
CASCADE_SPLITS = (8.0, 16.0, 32.0, 0.0)
TIE_DEPTH = 249.0 / 2048.0   # near 1, far 257: 1 - depth = 1799 / 2048, * -256 = -224.875, + 257 = 32.125, 257 / 32.125 = 8: every step exact
TIE_PIXELS = ((9, 5), (9, 70))
EDGE_TEXEL = SHADOW_RES // 2


def _cascades_and_taps():
    w, h = 128, 32
    cam = Camera.look((16.0, -6.0, 0.0), (0.0, 0.0, 1.0), aspect=16.0 / 9.0, near=1.0, far=257.0)
    c = Case("cascades_and_taps", w, h, cam, sun=(0.3, -0.8, -0.5), splits=CASCADE_SPLITS)
    linear = 4.12 * 2.0 ** (c.ys / 8.0)
    depth = depth_of(linear, cam)
    c.split_ties = np.zeros((h, w), bool)
    for y, x in TIE_PIXELS:
        depth[y, x] = TIE_DEPTH
        c.split_ties[y, x] = True
    c.gb["depth"] = depth
    n = unit(c.sun + c.V[h // 2, w // 2])
    c.gb["normal"][..., :3] = np.rint((n * 0.5 + 0.5) * 255.0).astype(np.uint8)
    # light space: x follows world x (the columns), y world y, z is a constant or runs with x; fitted per cascade at the middle of its depth range
    half_width = cam.tan_fov_half() * cam.aspect   # world x = 16 +- half_width * linear depth at the image's edges
    mats = []
    for ci, (mid, reach, z) in enumerate(((5.8, 1.2, (0.0, 0.5)), (11.6, 1.2, (0.67, 0.6)), (23.0, 1.2, (0.0, 0.5)), (46.0, 2.5, (0.0, 0.5)))):
        sx = reach / (half_width * mid)
        mats.append(ortho_light([(sx, 0, 0, -16.0 * sx), (0, 0.3 * sx, 0, 6.0 * 0.3 * sx), (z[0] * sx, 0, 0, z[1] - 16.0 * z[0] * sx)]))
    c.shadow_info = shadow_info_bytes(CASCADE_SPLITS, mats, [(3.0, 3.0)] * 4)
    edge = np.zeros((SHADOW_RES, SHADOW_RES), np.uint16)
    edge[:, EDGE_TEXEL:] = 0xffff
    full = np.full((SHADOW_RES, SHADOW_RES), 0xffff, np.uint16)
    c.shadow_maps = [edge, full, np.zeros((SHADOW_RES, SHADOW_RES), np.uint16), full.copy()]
    # pixels whose lit-tap count would hang on a rounding become sky (in any variant: the cascade counts select different maps for a pixel)
    for cascades in (1, 2, 3, 4):
        d = c.reference((2, 3, False, 1, cascades), want_slack=False).diag
        c.gb["depth"][(d["tap_texel_margin"] < 2 * TAP_TEXEL_MARGIN) | (d["tap_depth_margin"] < 2 * TAP_DEPTH_MARGIN)] = 0.0
    for y, x in TIE_PIXELS:
        assert c.gb["depth"][y, x] == np.float32(TIE_DEPTH)

    def check(ref, variant):
        c.common_check(ref, variant)
        cascades = variant[4]
        geo, d = ~ref.sky, ref.diag
        assert set(np.unique(d["cascade"][geo]).tolist()) == set(range(cascades)), "the ramp crosses every split"
        if cascades > 1:
            assert all(d["pixel_depth"][y, x] == CASCADE_SPLITS[0] and d["cascade"][y, x] >= 1 for y, x in TIE_PIXELS), "pixelDepth == split, exactly"
        in0 = geo & (d["cascade"] == 0)
        assert set(range(0, 13)) <= set(np.unique(d["lit"][in0]).tolist()), "the edge: every tap count 0 .. 12, %s" % np.unique(d["lit"][in0])
        if cascades >= 2:
            in1 = geo & (d["cascade"] == 1)
            assert ((d["lit"][in1] == 0).sum() > 50) and ((d["clamped_ties"][in1] == 12).sum() > 20), "all shadowed; depth clamped onto the texel"
            assert (d["lit"][in1 & (d["clamped_ties"] == 12) & (d["border_taps"] == 0)] == 12).all()
        if cascades >= 3:
            in2 = geo & (d["cascade"] == 2)
            assert (d["lit"][in2] == 12).all() and in2.sum() > 500, "all lit"
        if cascades == 4:
            in3 = geo & (d["cascade"] == 3)
            assert (d["border_taps"][in3] == 12).sum() > 100 and (d["lit"][in3 & (d["border_taps"] == 0)] == 0).all() and (in3 & (d["border_taps"] == 0)).sum() > 100
        assert (d["border_taps"][geo] > 0).any(), "the black border"
    c.check = check
    return c


# ------------------------------------------------------------------------------------------------------------------------ fog_and_indirect
FOG_MAX_DISTANCE = 30.0
SH_LENGTHS = (0.0, 0.005, 0.5, 1.5)


def _fog_and_indirect():
    w, h = 128, 96
    rows = 5.0 * 12.0 ** (np.arange(h) / (h - 1.0))
    rows[64:68] = FOG_MAX_DISTANCE
    splits = [float(np.sqrt(rows[y] * rows[y + 1])) for y in (11, 43, 79)]   # half way between two rows of the ramp
    c = Case("fog_and_indirect", w, h, _default_cam(w, h), splits=(*splits, 0.0), max_distance=FOG_MAX_DISTANCE)
    linear = np.repeat(rows[:, None], w, axis=1)
    depth = depth_of(linear, c.cam)
    depth[(c.xs * 7 + c.ys * 13) % 23 == 0] = 0.0
    c.gb["depth"] = depth
    n = unit(c.sun + 0.6 * c.V[h // 2, w // 2])
    c.gb["normal"][..., :3] = np.rint((n * 0.5 + 0.5) * 255.0).astype(np.uint8)
    length = np.asarray(SH_LENGTHS)[c.xs * len(SH_LENGTHS) // w]
    dominant = unit([0.2, -0.7, -0.6]) * length[..., None]
    ysh = np.zeros((h, w, 4), np.float32)
    ysh[..., 0] = 0.02 + 3.0 * length
    ysh[..., 3], ysh[..., 1], ysh[..., 2] = -dominant[..., 0], -dominant[..., 1], dominant[..., 2]   # dominantDirectionFromSH_L1: (-w, -y, z)
    c.ysh = pixfmt.pack_half(ysh)
    cocg = np.zeros((h, w, 2), np.float32)
    cocg[..., 0] = np.where(c.ys % 2 == 0, 0.05, -0.05) * ysh[..., 0]
    cocg[..., 1] = np.where((c.xs // 2) % 2 == 0, 0.04, -0.04) * ysh[..., 0]
    c.cocg = pixfmt.pack_half(cocg)
    c.sh_length = length

    def check(ref, variant):
        c.common_check(ref, variant)
        geo, d = ~ref.sky, ref.diag
        lin = d["froxel_linear"][geo]
        assert (lin < 0.2).any() and (lin > 1.9).any() and (np.abs(lin - 1.0) < 1e-5).sum() > 100, "below, at and beyond maxDistance"
        uv = d["fog_uv"]
        assert (uv[..., 0] < 0).any() and (uv[..., 0] > 1).any() and (uv[..., 1] < 0).any() and (uv[..., 1] > 1).any(), "all four borders"
        got = d["dominant_length"]
        assert (got[c.sh_length == 0.0] == 0.0).all() and (got[c.sh_length == 0.005] < 0.01).all() and (got[c.sh_length == 0.005] > 0.004).all()
        assert (np.abs(got[c.sh_length == 0.5] - 0.5) < 1e-3).all() and (got[c.sh_length == 1.5] > 1.4).all()
        co = pixfmt.unpack_half(c.cocg).reshape(c.h, c.w, 2)
        assert all(((co[..., k] > 0) & geo).any() and ((co[..., k] < 0) & geo).any() for k in (0, 1)), "CoCg of both signs"
        if variant[3] == 0:
            assert (d["irradiance"][geo] > 0).all()
        sky_in_quads = ref.sky[0::2, 0::2] | ref.sky[1::2, 0::2] | ref.sky[0::2, 1::2] | ref.sky[1::2, 1::2]
        assert ref.sky.sum() >= 100 and (sky_in_quads & ~(ref.sky[0::2, 0::2] & ref.sky[1::2, 0::2] & ref.sky[0::2, 1::2] & ref.sky[1::2, 1::2])).sum() >= 100
    c.check = check
    return c


_BUILDERS = {"material_lattice": _material_lattice, "mirror_highlight": _mirror_highlight, "grazing_and_terminator": _grazing_and_terminator,
             "cascades_and_taps": _cascades_and_taps, "fog_and_indirect": _fog_and_indirect}
NAMES = tuple(_BUILDERS)
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]
