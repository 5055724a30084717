"""The deferred shade in float64 numpy: the reference of tests/test_shade_reference_cpu.py and tests/test_shade_reference.py.

Written from the reference shader - triangle.frag (main, calcShadow, computeSpecularMultiscatteringLobe, applyVolumetricLighting), brdf.inc, GeometricAA.inc,
sunShadowCascades.inc, volumetricFroxelLighting.inc, SphericalHarmonics.inc, colorConversion.inc, linearDepth.inc, screenToWorld.inc - fed from the G-buffer the
way "deferredShading.comp" is: gl_FragCoord = pixel + 0.5, passPos rebuilt from depth like sdfDiffuseTrace.comp:120-126, N = normalize(normal texel * 2 - 1),
dFdxFine / dFdyFine(N) = the differences inside the pixel's 2 x 2 quad, a pixel with depth == 0 is sky. It shares no code and no routine with the oracle:
`pow`, `log2`, `exp`, `log`, `sin`, `cos`, `sqrt` are numpy's, in float64.

Every input is decoded exactly (an 8-bit, half, Depth16, D32 or fp32 value IS a float64 value; the shader's float literals are their fp32 values) and every step
after the decode is float64. Discrete steps follow DESIGN.md's sampler contract: nearest fetches are floor(u * size) with clamp / repeat / black border, linear
fetches (BRDF LUT: 2D clamp, froxel volume: 3D clamp) use 8 fractional weight bits, t = floor((u * size - 0.5) * 256 + 0.5), taken from the float64 coordinate.

`shade()` returns, per pixel: the unquantised RGB, the decision word in the oracle's layout (cascade | lit taps << 2 | 64; a sky pixel is only marked: 128) and

`slack`, per channel: the first-order forward error of an fp32 evaluation of the same pixel, by finite differences in the reference itself. The pixel is
re-evaluated with one scalar at a time moved by +- K_ULPS fp32 ulps - the dot products N.H, N.L, N.V, V.H, L.V of the sun's lobes, N.H, N.L, V.H of the indirect
lobe, the SH irradiance dot product, pixelDepth and the roughness after geometric AA - and with each linear fetch moved by +- one weight step (1 / 256 texel) per
axis; per scalar the larger of the two changes counts, and the changes are summed. A dot product of unit vectors is moved by ulps of 1.0 (its error is absolute:
it comes from the components, which are of order one, however small the sum), the irradiance by ulps of the sum of its terms' magnitudes, pixelDepth and the
roughness by ulps of their own value. The dot products are moved BEFORE the shader's clamps (max(., 0), abs, the 1e-4 floor), so a back-facing pixel stays unlit.

K_ULPS = 8, one constant for every implementation and every case. It is the count of roundings on the exact kernel set's longest path to a dot product, N.H, in
half-ulps of a component of order one: decode of the normal texel (c / 255, * 2 - 1: 2), normalise N (the squared length's five roundings reach a component
halved by the square root: 1.25, the square root 1, the division 1: 3.25), normalise V (3.25), V + L (1), normalise H (3.25), the dot product's products and
two additions (3): 15.75 half-ulps if every rounding pushes the same way - 16 half-ulps = 8 ulps. (The reconstruction of passPos in front of V is not counted.)
Nothing was run to choose it.

`mistake=` seeds one error at a time (MISTAKES): the tests show that each makes the comparison with the oracle fail, so the reference can fail. One of them,
pi in place of the shader's 3.1415 in multiscattering mode 0, moves the lobe by 2.9e-5 of itself - a three-hundredth of a storage code, which no colour image
can show; `specular_multiscattering_lobe` is a function of its own so that the oracle's lobe (its KAT entry point) can be held to it directly.
"""
import math
import struct

import numpy as np


def _c(x):
    """a float literal of the shader: its fp32 value"""
    return float(np.float32(x))


PI = _c(3.1415926535)  # global.inc:44
K_ULPS = 8
ULP1 = 2.0 ** -23      # fp32 ulp of 1.0
MISTAKES = ("roughness_floor", "schlick_exponent", "srgb_knee", "multiscatter_pi", "nov_floor", "pcf_compare", "cascade_compare", "froxel_linear_z")
SCALARS = ("NdotH", "NdotL", "NdotV", "VdotH", "LdotV", "NdotH_i", "NdotL_i", "VdotH_i", "irradiance_Y", "pixelDepth", "r")
FETCHES = (("lut_view", 2), ("lut_sun", 2), ("lut_indirect", 2), ("froxel", 3))
R11G11B10_MAX = np.array([65024.0, 65024.0, 64512.0])


# ------------------------------------------------------------------------------------------------------------------------ formats
def code_step(v):
    """one R11G11B10 code at the value v [..., 3]: 6 mantissa bits for R and G, 5 for B, denormals below 2^-14"""
    v = np.minimum(np.abs(np.asarray(v, np.float64)), R11G11B10_MAX)
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return 2.0 ** (e - np.array([6.0, 6.0, 5.0]))


def half_steps(got, ref):
    """|got - ref| in half-float steps at the reference value (the helper of tests/test_fast_kernels.py test_fast_brdf_lut_within_a_half_float_step)"""
    ref = np.asarray(ref, np.float64)
    step = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -14))) - 10)
    return np.abs(np.asarray(got, np.float64) - ref) / step


def _half(u16):
    return np.asarray(u16, np.uint16).view(np.float16).astype(np.float64)


def _unorm8(u8):
    return np.asarray(u8, np.uint8).astype(np.float64) / 255.0


class Global:
    """the fields of GlobalShaderInfo (global.inc:4-33, std140, 340 bytes) the shade reads"""

    def __init__(self, packed):
        b = bytes(packed)
        f4 = lambda off: np.array(struct.unpack_from("<3f", b, off), np.float64)
        self.sun_direction, self.camera_position = f4(128), f4(144)
        self.camera_right, self.camera_up, self.camera_forward = f4(176), f4(192), f4(208)
        self.noise_texture_indices = struct.unpack_from("<4i", b, 240)
        self.screen_resolution = struct.unpack_from("<2i", b, 272)
        self.tan_fov_half, self.aspect, self.near, self.far = (float(v) for v in struct.unpack_from("<4f", b, 280))
        self.frame_index_mod4 = struct.unpack_from("<I", b, 336)[0]


# ------------------------------------------------------------------------------------------------------------------------ linear fetches
def _axis(coord, size, shift):
    """-> (i0, i1, a): the two texels of one axis of a clamp-to-edge linear fetch and the weight of the second, 8 fractional bits"""
    t = np.floor((coord * size - 0.5) * 256.0 + 0.5).astype(np.int64) + int(shift)
    i0 = t >> 8
    a = (t & 255) / 256.0
    return np.clip(i0, 0, size - 1), np.clip(i0 + 1, 0, size - 1), a


def sample_linear_2d(tex, u, v, shift=(0, 0)):
    """tex [h, w, c] float64, clamp to edge; `shift` moves the fetch by whole weight steps per axis"""
    h, w, _ = tex.shape
    i0, i1, a = _axis(u, w, shift[0])
    j0, j1, b = _axis(v, h, shift[1])
    a, b = a[:, None], b[:, None]
    return (1 - a) * (1 - b) * tex[j0, i0] + a * (1 - b) * tex[j0, i1] + (1 - a) * b * tex[j1, i0] + a * b * tex[j1, i1]


def sample_linear_3d(tex, u, v, s, shift=(0, 0, 0)):
    """tests/test_kat.py _np_sample in three dimensions: tex [d, h, w, c] float64, clamp to edge on every axis"""
    d, h, w, _ = tex.shape
    i0, i1, a = _axis(u, w, shift[0])
    j0, j1, b = _axis(v, h, shift[1])
    k0, k1, c = _axis(s, d, shift[2])
    a, b, c = a[:, None], b[:, None], c[:, None]
    lo = (1 - a) * (1 - b) * tex[k0, j0, i0] + a * (1 - b) * tex[k0, j0, i1] + (1 - a) * b * tex[k0, j1, i0] + a * b * tex[k0, j1, i1]
    hi = (1 - a) * (1 - b) * tex[k1, j0, i0] + a * (1 - b) * tex[k1, j0, i1] + (1 - a) * b * tex[k1, j1, i0] + a * b * tex[k1, j1, i1]
    return (1 - c) * lo + c * hi


# ------------------------------------------------------------------------------------------------------------------------ brdf.inc
def _pow_nonneg(base, e):
    """GLSL leaves pow of a negative base undefined; the project's contract treats the base as 0"""
    return np.maximum(base, 0.0) ** e


def d_ggx(NoH, r):
    a = NoH * r
    k = r / (1.0 - NoH * NoH + a * a)
    return k * k * (1.0 / PI)


def visibility(NoV, NoL, r):
    r_2 = r * r
    v1 = NoL * np.sqrt(NoV * NoV * (1.0 - r_2) + r_2)
    v2 = NoV * np.sqrt(NoL * NoL * (1.0 - r_2) + r_2)
    return 0.5 / (v1 + v2)


def f_schlick(f0, f90, x, exponent=5.0):
    return f0 + (f90 - f0) * _pow_nonneg(1.0 - x, exponent)


def disney_diffuse(NoL, VoH, NoV, r, exponent=5.0):
    """DisneyDiffuse / diffuseColor"""
    energy_bias = 0.5 * r
    energy_factor = 1.0 * (1.0 - r) + (_c(1.0) / _c(1.51)) * r
    f90 = energy_bias + 2.0 * VoH * VoH * r
    return 1.0 / PI * f_schlick(1.0, f90, NoL, exponent) * f_schlick(1.0, f90, NoV, exponent) * energy_factor


def cod_wwii_diffuse(NoL, VoH, NoV, NoH, r):
    """CoDWWIIDiffuse / diffuseColor (its powers of five are not Schlick's)"""
    f0 = VoH + _pow_nonneg(1.0 - VoH, 5.0)
    f1 = (1.0 - 0.75 * _pow_nonneg(1.0 - NoL, 5.0)) * (1.0 - 0.75 * _pow_nonneg(1.0 - NoV, 5.0))
    g = np.log2(2.0 / (r * r) - 1.0) / 18.0
    t = np.clip(_c(2.2) * g - 0.5, 0.0, 1.0)
    fd = f0 + (f1 - f0) * t
    fb = (34.5 * g * g - 59.0 * g + 24.5) * VoH * 2.0 ** (-np.maximum(_c(73.2) * g - _c(21.2), _c(8.9)) * np.sqrt(NoH))
    return 1.0 / PI * (fd + fb)


def titanfall2_single(NoL, LoV, NoV, NoH, r):
    facing = 0.5 + 0.5 * LoV
    rough = facing * (_c(0.9) - _c(0.4) * facing) * (0.5 + NoH) / np.maximum(NoH, _c(0.03))
    smooth = _c(1.05) * (1.0 - _pow_nonneg(1.0 - NoL, 5.0)) * (1.0 - _pow_nonneg(1.0 - NoV, 5.0))
    return 1.0 / PI * (smooth * (1.0 - r) + rough * r)


def reflected_energy_average(roughness):
    smoothness = 1.0 - np.sqrt(roughness)
    r = _c(-0.0761947) - _c(0.383026) * smoothness
    r = _c(1.04997) + smoothness * r
    r = _c(0.409255) + smoothness * r
    return np.minimum(_c(0.999), r)


def specular_multiscattering_lobe(mode, lut, r, NoL, f0, single_lobe, lut_texel, shift=(0, 0), pi_of_mode_0=_c(3.1415)):
    """triangle.frag computeSpecularMultiscatteringLobe: r, NoL [n]; f0, single_lobe, lut_texel (the LUT at (r, NoV)) [n, 3]; lut [res, res, 4] -> [n, 3].
    Mode 0 divides by the shader's own 3.1415, not by pi."""
    energy_outgoing = lut_texel[:, 1:2]
    fresnel_average = f0 + (1.0 - f0) / 21.0
    if mode == 0:
        energy_average = reflected_energy_average(r)[:, None]
        energy_incoming = sample_linear_2d(lut, r, NoL, shift)[:, 1:2]
        unscaled = (1.0 - energy_incoming) * (1.0 - energy_outgoing) / (pi_of_mode_0 * (1.0 - energy_average))
        scaling = (fresnel_average * fresnel_average * energy_average) / (1.0 - fresnel_average * (1.0 - energy_average))
        return unscaled * scaling
    if mode == 1:
        scaling = (fresnel_average * fresnel_average * energy_outgoing) / (1.0 - fresnel_average * (1.0 - energy_outgoing))
        return (1.0 - energy_outgoing) / PI * scaling
    if mode == 2:
        return f0 * (1.0 / energy_outgoing - 1.0) * single_lobe
    return np.zeros_like(f0)


# ------------------------------------------------------------------------------------------------------------------------ the BRDF LUT (brdfLut.comp)
def _radical_inverse(i):
    bits = np.asarray(i, np.uint64)
    out = np.zeros(bits.shape, np.uint64)
    for b in range(32):
        out |= ((bits >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return out.astype(np.float64) * _c(2.3283064365386963e-10)


def brdf_lut(res, diffuse_model):
    """brdfLut.comp in float64 with its 1024 Hammersley points: [res, res, 4] (x: Fresnel-weighted, y: directional albedo, z: diffuse integral, w: 0).
    N = (0, 0, 1): the tangent frame of sampling.inc is tangent (0, -1, 0), bitangent (1, 0, 0), a hemisphere sample (x, y, z) lands on (y, -x, z)"""
    samples = 1024
    i = np.arange(samples)
    xi_x, xi_y = i / float(samples), _radical_inverse(i)
    ux = np.arange(res, dtype=np.float64)[None, :, None]
    uy = np.arange(res, dtype=np.float64)[:, None, None]
    r = np.maximum(ux / res, _c(0.0001))
    NoV = np.maximum(uy, _c(0.1)) / res
    Vx, Vz = np.sqrt(1.0 - NoV * NoV), NoV
    out = np.zeros((res, res, 4))
    # specular: importanceSampleGGX
    r_2 = r * r
    cos_t = np.sqrt((1.0 - xi_y) / (1.0 + (r_2 * r_2 - 1.0) * xi_y))
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    phi = 2.0 * PI * xi_x
    Hx, Hy, Hz = np.sin(phi) * sin_t, -np.cos(phi) * sin_t, cos_t
    VdotH = Vx * Hx + Vz * Hz
    Lz = 2.0 * VdotH * Hz - Vz
    VoH, NoH, NoL = np.maximum(VdotH, 0.0), np.maximum(Hz, 0.0), np.maximum(Lz, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(NoL > 0.0, visibility(NoV, NoL, r) * VoH * NoL / NoH, 0.0)
    out[..., 0] = (_pow_nonneg(1.0 - VoH, 5.0) * k).sum(-1)
    out[..., 1] = k.sum(-1)
    # diffuse: importanceSampleCosine
    phi = 2.0 * PI * xi_y
    cos_t, sin_t = np.sqrt(xi_x), np.sqrt(1.0 - xi_x)
    Lx, Ly, Lz = np.sin(phi) * sin_t, -np.cos(phi) * sin_t, cos_t
    hx, hy, hz = Vx + Lx, Ly + 0.0 * Vx, Vz + Lz
    hl = np.sqrt(hx * hx + hy * hy + hz * hz)
    hx, hz = hx / hl, hz / hl
    VoH = np.clip(Vx * hx + Vz * hz, 0.0, 1.0)
    NoL, NoH = np.maximum(Lz, 0.0), np.maximum(hz, 0.0)
    f0d = _c(0.04)
    in_out = (1.0 - f_schlick(f0d, 1.0, NoV)) * (1.0 - f_schlick(f0d, 1.0, NoL))
    if diffuse_model == 0:
        z = (1.0 / PI) * in_out
    elif diffuse_model == 1:
        z = disney_diffuse(NoL, VoH, NoV, r) * in_out
    elif diffuse_model == 2:
        z = cod_wwii_diffuse(NoL, VoH, NoV, NoH, r) * in_out
    else:
        LoV = np.clip(Lx * Vx + Lz * Vz, 0.0, 1.0)
        z = titanfall2_single(NoL, LoV, NoV, NoH, r) * in_out
    out[..., 2] = np.broadcast_to(z, (res, res, samples)).sum(-1)
    out /= float(samples)
    out[..., :2] *= 4.0
    return out


# ------------------------------------------------------------------------------------------------------------------------ the shade
class Result:
    """rgb [h, w, 3], words [h, w] uint32, slack [h, w, 3] (None if not asked for), terms: name -> [h, w, ...] (if asked for), diag: what the cases' self-checks read"""


def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _dot(a, b):
    return (a * b).sum(-1)


def _normals(normal_rgba8):
    raw = _unorm8(normal_rgba8[..., :3]) * 2.0 - 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = _normalize(raw)
    bad = np.isnan(n).any(-1)
    n[bad] = raw[bad]
    return n


def _srgb_to_linear(x, knee):
    lo = x / _c(12.92)
    hi = (np.abs(x + _c(0.055)) / _c(1.055)) ** _c(2.4)
    return np.where(x <= knee, lo, hi)


def _ycocg_to_linear(y, co, cg):
    return np.stack([y + co - cg, y + cg, y - co - cg], -1)


def shade(gb, w, h, brdf_lut_u16, lut_res, light_bytes, shadow_info, shadow_maps, shadow_res, ysh_u16, cocg_u16, froxel_u16, froxel_dims, vol_settings, sky_packed,
          global_packed, noise_textures, diffuse_brdf=2, multiscatter=0, geometric_aa=True, indirect_tech=0, cascades=3, mistake=None, want_slack=True, want_terms=False):
    """The arguments of passes.orc_deferred_shading with the noise textures as arrays (`noise_textures[bindless index]`: [32, 32, 2] uint8) in place of the
    bindless set. `sky_packed` is not read: a sky pixel is only marked."""
    assert mistake is None or mistake in MISTAKES, mistake
    g = Global(global_packed)
    n = w * h
    # ---- decode
    depth = np.asarray(gb["depth"], np.float32).astype(np.float64).reshape(n)
    albedo_texel = _unorm8(np.asarray(gb["albedo"]).reshape(n, 4)[:, :3])
    specular_texel = _unorm8(np.asarray(gb["specular"]).reshape(n, 4)[:, :3])
    normals = _normals(np.asarray(gb["normal"]).reshape(h, w, 4))
    lut = _half(brdf_lut_u16).reshape(lut_res, lut_res, 4)
    sun_color = np.array(struct.unpack_from("<3f", light_bytes, 0), np.float64)
    sun_strength = float(struct.unpack_from("<f", light_bytes, 16)[0])
    info = np.frombuffer(bytes(shadow_info), np.float32).astype(np.float64)
    splits, matrices, light_space_scale = info[0:4], info[4:68].reshape(4, 4, 4), info[68:76].reshape(4, 2)  # matrices[c][column][row]
    maps = [np.asarray(m, np.uint16).astype(np.float64).reshape(shadow_res, shadow_res) / 65535.0 for m in shadow_maps]
    ysh = _half(ysh_u16).reshape(n, 4)
    cocg = _half(cocg_u16).reshape(n, 2)
    fw, fh, fd = froxel_dims
    froxel = _half(froxel_u16).reshape(fd, fh, fw, 4)
    max_distance = float(struct.unpack_from("<f", vol_settings, 28)[0])
    noise_tex = np.asarray(noise_textures[g.noise_texture_indices[g.frame_index_mod4]])
    nh, nw = noise_tex.shape[:2]

    ys, xs = np.mgrid[0:h, 0:w]
    px, py = xs.reshape(n), ys.reshape(n)
    frag = np.stack([px + 0.5, py + 0.5], -1)
    screen_uv = frag / np.array(g.screen_resolution, np.float64)
    # ---- the interpolants, from the G-buffer (screenToWorld.inc, linearDepth.inc)
    ndc = screen_uv * 2.0 - 1.0
    view = -g.camera_forward + g.tan_fov_half * ndc[:, 1:2] * g.camera_up - g.tan_fov_half * g.aspect * ndc[:, 0:1] * g.camera_right
    v_cam = -_normalize(view)
    depth_linear = g.near * g.far / (g.far + (-depth + 1.0) * (g.near - g.far))
    pass_pos = g.camera_position + v_cam / _dot(v_cam, g.camera_forward)[:, None] * depth_linear[:, None]
    sky = depth == 0.0

    # ---- triangle.frag main()
    metalic = specular_texel[:, 2]
    r = specular_texel[:, 1]
    r = np.maximum(r * r, _c(0.005) if mistake == "roughness_floor" else _c(0.0045))
    albedo = _srgb_to_linear(albedo_texel, _c(0.04045) if mistake == "srgb_knee" else _c(0.004045))
    diffuse_color = (1.0 - metalic)[:, None] * albedo
    N = normals.reshape(n, 3)
    L = _normalize(g.sun_direction)
    V = g.camera_position - pass_pos
    pixel_depth = _dot(V, -g.camera_forward)
    V = _normalize(V)
    H = _normalize(V + L)
    if geometric_aa:  # GeometricAA.inc with the quad's differences
        xl, yl = px & ~1, py & ~1
        at = lambda x, y: normals[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        n_u = at(xl + 1, py) - at(xl, py)
        n_v = at(px, yl + 1) - at(px, yl)
        variance = 0.25 * (_dot(n_v, n_v) + _dot(n_u, n_u))
        kernel_roughness2 = np.minimum(2.0 * variance, _c(0.18))
        r = np.clip(np.sqrt(r * r + kernel_roughness2), 0.0, 1.0)
    f0 = _c(0.04) * (1.0 - metalic)[:, None] + albedo * metalic[:, None]

    # ---- cascade and PCF (triangle.frag:84-120, 222-239)
    cascade = np.zeros(n, np.int64)
    for c in range(cascades - 1):
        cascade += (pixel_depth > splits[c]) if mistake == "cascade_compare" else (pixel_depth >= splits[c])
    with np.errstate(divide="ignore", invalid="ignore"):
        split_margin = np.min(np.abs(pixel_depth[:, None] - splits[None, :max(cascades - 1, 0)]) / pixel_depth[:, None], axis=1, initial=np.inf)
    noise_rg = _unorm8(noise_tex[py % nh, px % nw, :2])  # nearest, repeat, at gl_FragCoord / textureSize: the texel (x mod w, y mod h)
    noise = noise_rg[:, 0]
    lit = np.zeros(n, np.int64)
    tap_depth_margin = np.full(n, np.inf)   # smallest |actualDepth - texel| over the taps whose depth is not clamped onto the texel's value
    tap_texel_margin = np.full(n, np.inf)   # smallest distance, in texels, of a tap to a texel boundary behind which the map holds another value
    clamped_ties = np.zeros(n, np.int64)
    border_taps = np.zeros(n, np.int64)
    for c in range(cascades):
        sel = np.nonzero(cascade == c)[0]
        if sel.size == 0:
            continue
        M = matrices[c]
        p = (M[None, :, :] * np.concatenate([pass_pos[sel], np.ones((sel.size, 1))], 1)[:, :, None]).sum(1)  # p[row] = sum over columns M[column][row] * v[column]
        p = p / p[:, 3:4]
        xy = p[:, :2] * 0.5 + 0.5
        actual = np.clip(p[:, 2], 0.0, 1.0)
        was_clamped = (p[:, 2] <= 0.0) | (p[:, 2] >= 1.0)
        offset_scale = _c(0.03) * light_space_scale[c]
        padded = np.zeros((shadow_res + 2, shadow_res + 2))  # black border
        padded[1:-1, 1:-1] = maps[c]
        for i in range(12):
            d = np.sqrt((i + 0.5 * noise[sel]) / 12.0)
            angle = noise[sel] * 2.0 * PI + 2.0 * PI * i / 12.0
            pos = xy + np.stack([np.cos(angle), np.sin(angle)], -1) * offset_scale * d[:, None]
            t = pos * shadow_res
            tf = np.floor(t)
            ti = np.clip(tf, -1, shadow_res).astype(np.int64)
            texel = padded[ti[:, 1] + 1, ti[:, 0] + 1]
            lit[sel] += (actual > texel) if mistake == "pcf_compare" else (actual >= texel)
            tie = was_clamped & (actual == texel)
            clamped_ties[sel] += tie
            border_taps[sel] += (ti[:, 0] < 0) | (ti[:, 1] < 0) | (ti[:, 0] >= shadow_res) | (ti[:, 1] >= shadow_res)
            tap_depth_margin[sel] = np.minimum(tap_depth_margin[sel], np.where(tie, np.inf, np.abs(actual - texel)))
            fr = t - tf
            for axis, step in ((0, -1), (0, 1), (1, -1), (1, 1)):
                nb = ti.copy()
                nb[:, axis] = np.clip(nb[:, axis] + step, -1, shadow_res)
                adjacent = (tf[:, axis] >= -1) & (tf[:, axis] <= shadow_res)  # further out, the neighbour along this axis is border as well
                other = adjacent & (padded[nb[:, 1] + 1, nb[:, 0] + 1] != texel)
                tap_texel_margin[sel] = np.minimum(tap_texel_margin[sel], np.where(other, fr[:, axis] if step < 0 else 1.0 - fr[:, axis], np.inf))
    sun_shadow = lit / 12.0
    words = np.where(sky, 128, cascade | (lit << 2) | 64).astype(np.uint32)

    # ---- the indirect lobe's vectors (triangle.frag:297-315, SphericalHarmonics.inc)
    k0, k1 = 1.0 / (2.0 * math.sqrt(PI)), math.sqrt(3.0) / (2.0 * math.sqrt(PI))
    sh = _normalize(np.stack([np.full(n, k0), -k1 * N[:, 1], k1 * N[:, 2], -k1 * N[:, 0]], -1))
    dominant = np.stack([-ysh[:, 3], -ysh[:, 1], ysh[:, 2]], -1)
    dominant_length = np.clip(np.sqrt(_dot(dominant, dominant)), _c(0.01), 1.0)
    L_i = dominant / dominant_length[:, None]
    H_i = _normalize(L_i + V)
    L_i_scale = np.maximum(1.0, np.sqrt(_dot(L_i, L_i)))

    # ---- the fog's coordinates (applyVolumetricLighting)
    fog_uv = screen_uv + (noise_rg - 0.5) * _c(0.013)

    scalars = {"NdotH": _dot(N, H), "NdotL": N @ L, "NdotV": _dot(N, V), "VdotH": _dot(V, H), "LdotV": V @ L, "NdotH_i": _dot(N, H_i), "NdotL_i": _dot(N, L_i),
               "VdotH_i": _dot(V, H_i), "irradiance_Y": _dot(ysh, sh), "pixelDepth": pixel_depth, "r": r}
    unit = K_ULPS * ULP1
    deltas = {"NdotH": unit, "NdotL": unit, "NdotV": unit, "VdotH": unit, "LdotV": unit, "NdotH_i": unit, "NdotL_i": unit * L_i_scale, "VdotH_i": unit,
              "irradiance_Y": unit * np.abs(ysh * sh).sum(-1), "pixelDepth": K_ULPS * np.spacing(pixel_depth.astype(np.float32)).astype(np.float64),
              "r": K_ULPS * np.spacing(r.astype(np.float32)).astype(np.float64)}
    exponent = 4.0 if mistake == "schlick_exponent" else 5.0
    nov_floor = _c(0.001) if mistake == "nov_floor" else _c(0.0001)
    ms_pi = PI if mistake == "multiscatter_pi" else _c(3.1415)

    def multiscattering_lobe(rr, NoL, single, lut_texel, fetch, shift):
        return specular_multiscattering_lobe(multiscatter, lut, rr, NoL, f0, single, lut_texel, shift[fetch], ms_pi)

    def evaluate(s, shift, terms=None):
        rr = s["r"]
        NoH = np.maximum(s["NdotH"], 0.0)
        NoL = np.clip(s["NdotL"], 0.0, 1.0)
        VoH = np.abs(s["VdotH"])
        LoV = np.maximum(s["LdotV"], 0.0)
        NoV = np.maximum(np.abs(s["NdotV"]), nov_floor)
        direct_lighting = (np.maximum(s["NdotL"], 0.0) * sun_shadow)[:, None] * sun_color
        lut_texel = sample_linear_2d(lut, rr, NoV, shift["lut_view"])
        integral = lut_texel[:, 2:3] * np.ones((1, 3))
        if diffuse_brdf == 0:
            lobe = diffuse_color / PI
        elif diffuse_brdf == 1:
            lobe = diffuse_color * disney_diffuse(NoL, VoH, NoV, rr, exponent)[:, None]
        elif diffuse_brdf == 2:
            lobe = diffuse_color * cod_wwii_diffuse(NoL, VoH, NoV, NoH, rr)[:, None]
        else:
            single = titanfall2_single(NoL, LoV, NoV, NoH, rr)
            lobe = diffuse_color * (single[:, None] + diffuse_color * (_c(0.1159) * rr)[:, None])
            multi_integral = _c(0.1159) * rr * PI * 2.0 * (1.0 - f_schlick(_c(0.04), 1.0, NoV, exponent)) * _c(0.94291)
            integral = np.minimum(lut_texel[:, 2:3] + diffuse_color * multi_integral[:, None], 1.0)
        fresnel_in_out = (1.0 - f_schlick(f0, 1.0, NoV[:, None], exponent)) * (1.0 - f_schlick(f0, 1.0, NoL[:, None], exponent))
        diffuse_direct = lobe * direct_lighting * fresnel_in_out
        D, Vis, F = d_ggx(NoH, rr), visibility(NoV, NoL, rr), f_schlick(f0, 1.0, VoH[:, None], exponent)
        single_lobe = (D * Vis)[:, None] * F
        multi_lobe = multiscattering_lobe(rr, NoL, single_lobe, lut_texel, "lut_sun", shift)
        specular_direct = direct_lighting * (single_lobe + multi_lobe)
        if indirect_tech == 0:
            irradiance = _ycocg_to_linear(s["irradiance_Y"], cocg[:, 0], cocg[:, 1])
            diffuse_indirect = irradiance * diffuse_color * integral
            r_i = 1.0 * (1.0 - np.sqrt(dominant_length)) + rr * np.sqrt(dominant_length)
            NoH_i, NoL_i, VoH_i = np.maximum(s["NdotH_i"], 0.0), np.maximum(s["NdotL_i"], 0.0), np.maximum(s["VdotH_i"], 0.0)
            single_i = (d_ggx(NoH_i, r_i) * visibility(NoV, NoL_i, r_i))[:, None] * f_schlick(f0, 1.0, VoH_i[:, None], exponent)
            multi_i = multiscattering_lobe(r_i, NoL_i, single_i, lut_texel, "lut_indirect", shift)
            specular_indirect = (single_i + multi_i) * _ycocg_to_linear(ysh[:, 0], cocg[:, 0], cocg[:, 1])
        else:
            ambient = _c(0.003) * sun_strength
            single_i, multi_i = np.zeros((n, 3)), np.zeros((n, 3))
            diffuse_indirect = ambient * diffuse_color * integral
            specular_indirect = (lut_texel[:, 0:1] * (1.0 - f0) + lut_texel[:, 1:2] * f0) * ambient
        color = (diffuse_direct + specular_direct) * sun_strength + diffuse_indirect + specular_indirect
        # applyVolumetricLighting (volumetricFroxelLighting.inc: exponential depth distribution, k = 3)
        linear = s["pixelDepth"] / max_distance
        z = linear if mistake == "froxel_linear_z" else np.log(linear * (math.exp(3.0) - 1.0) + 1.0) / 3.0
        fog = sample_linear_3d(froxel, fog_uv[:, 0], fog_uv[:, 1], z, shift["froxel"])
        if terms is not None:
            terms.update(D=D, Vis=Vis, F=F, diffuse_lobe=lobe * fresnel_in_out, multiscatter_lobe=multi_lobe, direct_lighting=direct_lighting,
                         single_indirect=single_i, multiscatter_indirect=multi_i, diffuse_indirect=diffuse_indirect, specular_indirect=specular_indirect, fog=fog,
                         unfogged=color, NoH=NoH, NoL=NoL, NoV=NoV, VoH=VoH, LoV=LoV, r=rr, froxel_z=z, lut_texel=lut_texel)
        return color * fog[:, 3:4] + fog[:, :3]

    no_shift = {name: (0,) * axes for name, axes in FETCHES}
    out = Result()
    terms = {} if want_terms else None
    with np.errstate(all="ignore"):
        rgb = evaluate(scalars, no_shift, terms)
        slack, parts = None, {}
        if want_slack:
            slack = np.zeros((n, 3))
            for name in SCALARS:
                worst = np.zeros((n, 3))
                for sign in (-1.0, 1.0):
                    moved = dict(scalars)
                    moved[name] = scalars[name] + sign * deltas[name]
                    worst = np.fmax(worst, np.abs(evaluate(moved, no_shift) - rgb))
                slack += worst
                parts[name] = worst
            for name, axes in FETCHES:
                if (name == "lut_sun" and multiscatter != 0) or (name == "lut_indirect" and (multiscatter != 0 or indirect_tech != 0)):
                    continue  # the fetch is not made
                for axis in range(axes):
                    worst = np.zeros((n, 3))
                    for step in (-1, 1):
                        moved = dict(no_shift)
                        moved[name] = tuple(step if a == axis else 0 for a in range(axes))
                        worst = np.fmax(worst, np.abs(evaluate(scalars, moved) - rgb))
                    slack += worst
                    parts["%s[%d]" % (name, axis)] = worst
            slack = slack.reshape(h, w, 3)
    out.rgb, out.words, out.slack, out.sky = rgb.reshape(h, w, 3), words.reshape(h, w), slack, sky.reshape(h, w)
    out.slack_parts = {k: v.reshape(h, w, 3) for k, v in parts.items()}  # slack, by the scalar or fetch axis that was moved
    out.terms = None if terms is None else {k: v.reshape((h, w) + v.shape[1:]) for k, v in terms.items()}
    shape = lambda a: a.reshape(h, w)
    out.diag = dict(r=shape(r), NdotH=shape(scalars["NdotH"]), NdotL=shape(scalars["NdotL"]), NdotV=shape(scalars["NdotV"]), pixel_depth=shape(pixel_depth),
                    cascade=shape(cascade), lit=shape(lit), split_margin=shape(split_margin), tap_depth_margin=shape(tap_depth_margin),
                    tap_texel_margin=shape(tap_texel_margin), clamped_ties=shape(clamped_ties), border_taps=shape(border_taps), fog_uv=fog_uv.reshape(h, w, 2),
                    dominant_length=shape(np.sqrt(_dot(dominant, dominant))), metalic=shape(metalic), albedo=albedo.reshape(h, w, 3),
                    irradiance=_ycocg_to_linear(scalars["irradiance_Y"], cocg[:, 0], cocg[:, 1]).reshape(h, w, 3), froxel_linear=shape(pixel_depth / max_distance))
    return out


# ------------------------------------------------------------------------------------------------------------------------ the comparison
def compare(packed_u32, ref, extra=None):
    """An implementation's R11G11B10 image against the reference: -> dict with
    excess [h, w, 3]: (|unpack(got) - ref| - slack) in codes at the reference value - the statement is excess <= 1 on every geometry pixel;
    slack_codes [h, w, 3]; well [h, w]: slack below a quarter of a code in every channel. The reference value is clamped to the format's largest finite
    value, as the format's encoder clamps (DESIGN.md's format contract)."""
    from plainrenderer_amd import pixfmt
    h, w = ref.words.shape
    got = pixfmt.unpack_r11g11b10(np.asarray(packed_u32, np.uint32).reshape(-1)).reshape(h, w, 3).astype(np.float64)
    want = np.minimum(np.maximum(ref.rgb, 0.0), R11G11B10_MAX)
    step = code_step(want)
    slack_codes = ref.slack / step
    excess = np.abs(got - want) / step - slack_codes
    return dict(excess=excess, slack_codes=slack_codes, well=(slack_codes < 0.25).all(-1), got=got, finite=np.isfinite(got).all(-1))
