"""The sky pass' setting at the C boundary and the invariants of the tests' own reference (tests/sky_reference.py); no GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

from plainrenderer_amd import pixfmt, synth
from plainrenderer_amd.scene import Camera, GlobalShaderInfo

W, H = 48, 32


def _lib():
    from plainrenderer_amd import backend
    return backend._load()


def _globals(sun, time=0.75, fov=4.0, w=W, h=H):
    cam = Camera.look((1.0, 2.0, 3.0), (0.3, -0.5, 0.8), fov=fov, aspect=w / h)
    g = cam.fill_global(GlobalShaderInfo(), w, h)
    g.sunDirection = (*[float(x) for x in sun], 0.0)
    g.time = time
    return cam, g.pack()


def test_default_settings_leave_the_sky_pass_off_and_the_struct_sizes_agree():
    from plainrenderer_amd.frame import PlrfSettings
    lib = _lib()
    size = C.sizeof(PlrfSettings)
    buf = (C.c_uint8 * (size + 64))(*([0xA5] * (size + 64)))  # plrf_default_settings clears sizeof(plrf_settings) bytes: the guard behind must survive
    assert lib.plrf_default_settings(buf, C.c_uint32(640), C.c_uint32(360)) == 0
    s = PlrfSettings.from_buffer_copy(bytes(buf)[:size])
    assert s.run_sky == 0 and s.run_shading == 1 and (s.width, s.height) == (640, 360)
    assert PlrfSettings.run_sky.offset + 4 == size, "run_sky is the last field"
    assert all(b == 0xA5 for b in bytes(buf)[size:]), "the C struct is larger than the ctypes mirror"
    assert bytes(buf)[size - 4:size] == bytes(4), "the C struct is smaller than the ctypes mirror: its last field was not written"


def test_the_sky_pass_without_the_shade_is_refused():
    """validated before anything touches the GPU: PLR_ERR_INVALID_ARGUMENT with a message that names both settings"""
    from plainrenderer_amd.frame import PlrfSettings
    lib = _lib()
    lib.plrf_last_error.restype = C.c_char_p
    s = PlrfSettings()
    assert lib.plrf_default_settings(C.byref(s), C.c_uint32(64), C.c_uint32(64)) == 0
    s.run_sky, s.run_shading = 1, 0
    handle = C.c_void_p()
    assert lib.plrf_create(C.byref(s), C.byref(handle)) == -1  # PLR_ERR_INVALID_ARGUMENT
    assert not handle.value
    msg = lib.plrf_last_error().decode()
    assert "run_sky" in msg and "run_shading" in msg


def test_the_shader_is_registered_for_both_math_modes():
    from plainrenderer_amd import supported_shaders
    assert "skyAndSunSprite.comp" in supported_shaders()


def test_reference_constant_sky_stays_within_the_dither(oracle):
    """constant LUT, identity froxel volume (in-scattering 0, transmittance 1), no sun in view: the sky is the constant +- 1/255"""
    import sky_reference as sr
    cam, g = _globals(-np.asarray(Camera.look((0, 0, 0), (0.3, -0.5, 0.8)).forward))
    const = np.array([0.25, 0.5, 0.125], np.float32)
    lut = (np.full(200 * 100, pixfmt.pack_r11g11b10(const[None, :])[0], np.uint32), 200, 100)
    vol = np.zeros((4, (H + 7) // 8, (W + 7) // 8, 4), np.float32)
    vol[..., 3] = 1.0
    ref = sr.sky_pass(g, W, H, lut, (synth.transmission_lut(), 128, 128), (pixfmt.pack_half(vol), (W + 7) // 8, (H + 7) // 8, 4), 70.0,
                      struct.pack("<5f", 1, 1, 1, 1, 12.8))
    assert not ref["in_disc"].any()
    assert np.abs(ref["sky"] - const).max() <= 1.0 / 255.0 + 1e-7
    assert np.abs(ref["sky"] - const).max() > 0, "no dither at all"
    stored = pixfmt.unpack_r11g11b10(ref["stored"].reshape(-1))
    assert np.abs(stored - const).max() <= 1.0 / 255.0 + const.max() / 64.0  # + half an R11G11B10 step (5 mantissa bits in blue)


def test_reference_disc_is_symmetric_about_its_centre(oracle):
    import sky_reference as sr
    rng = np.random.default_rng(5)
    S = np.asarray(Camera.look((0, 0, 0), (0.2, -0.7, 0.4)).forward, np.float64)
    a = np.cross(S, [0.0, 1.0, 0.0]); a /= np.linalg.norm(a)
    b = np.cross(S, a)
    r = rng.uniform(0.0, 1.5, 64) * float(sr.SUN_SPRITE_SCALE)
    t = rng.uniform(0.0, 2 * np.pi, 64)
    off = r[:, None] * (np.cos(t)[:, None] * a + np.sin(t)[:, None] * b)
    def d2(sign):
        v = S + sign * off
        v /= np.linalg.norm(v, axis=1)[:, None]
        return sr.sun_disc(v.astype(np.float32), S.astype(np.float32))[1].astype(np.float64)
    plus, minus = d2(1.0), d2(-1.0)
    expect = (r / float(sr.SUN_SPRITE_SCALE)) ** 2
    # float32 rays carry ~6e-8 of error against offsets of ~5e-3: 1e-4 relative on the squared distance
    assert np.abs(plus - minus).max() <= 2e-4 * (1.0 + expect.max())
    assert np.abs(plus - expect).max() <= 2e-4 * (1.0 + expect.max())


@pytest.mark.parametrize("longitude,latitude", [(0.0, 30.0), (90.0, 45.0), (200.0, 10.0), (-73.0, 80.0), (10.0, 120.0)])
def test_reference_sprite_centre_is_the_sun_direction(longitude, latitude):
    """the quad's centre under Sky::issueSkyDrawcalls' model matrix is directionToVector(sunDirection) = g_sunDirection"""
    import sky_reference as sr
    assert np.abs(sr.sprite_centre(longitude, latitude) - sr.direction_to_vector(longitude, latitude)).max() < 1e-6
