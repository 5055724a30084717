"""The per-pass parity checks of tests/pass_parity.py (the statement tests/test_parity_fullsize.py holds the benchmarked kernel set to at 3840 x 2160)
at frame sizes no kernel geometry divides: bench.py's scene, PLR_MATH_FAST, two frames with the oracle frame beside them, every pass fed what the
oracle pass consumed. Every check also asserts that the pass ran the fast kernels (no general-kernel execution) and holds the pixels of the last,
partial, block column / row of the kernel's launch (plus a 2-pixel border) to the flip caps on their own. Measured numbers:
profiles/r07_parity_ragged.txt.

What each size makes ragged (trace image = half resolution, W // 2 x H // 2):
  322 x 182    even frame, odd trace image 161 x 91: the upscale's quad kernel and the fused upscale + shade end in a half quad column / row;
               trace 8 x 8 groups and 32-pixel culling tiles partial; TAA strips 322 = 5 * 62 + 12 columns, 182 = 11 * 16 + 6 rows
  323 x 183    odd frame: indirectLightUpscaleFastKernel (not 2x the trace image) and no upscale + shade fusion (separate fast launches)
  1000 x 563   TAA 1000 = 16 * 62 + 8, 563 = 35 * 16 + 3 (three rows in the strip kernel's last block); the spatial filter's one-column walk
               with a partial last chunk (500 x 281)
  3074 x 1730  trace image 1537 x 865: the spatial filter's two-XCD-column walk (widths from 1536), odd texel counts both ways
  72 x 40      trace image 36 x 20, narrower than one 64-texel filter tile; one TAA strip, one culling tile
"Narrower than 64" is asked of the trace image (72 x 40 traces 36 x 20): a full-resolution frame narrower than 64 is not in the list.
"""
import pytest

import pass_parity as pp

SIZES = [(322, 182), (323, 183), (1000, 563), (3074, 1730), (72, 40)]
TAA_SIZES = [(322, 182), (1000, 563)]
SPATIAL_FULL_RES_SIZES = [(323, 183), (1000, 563)]
# (clip, dilate, history sampler, tonemap): every sampler x clip / clamp; samplers 0 and 4 run the strip kernel, 1 - 3 the 64 x 4 kernel
TAA_VARIANTS = [(clip, True, tech, True) for tech in range(5) for clip in (True, False)]

_ids = ["%dx%d" % wh for wh in SIZES]


def test_the_size_list_keeps_every_geometry_ragged():
    """each kernel geometry the module exists for is ragged at one size of the list at least (a later edit of SIZES cannot drop one silently)"""
    def some(cond):
        return any(cond(w, h, w // 2, h // 2) for w, h in SIZES)
    assert some(lambda w, h, tw, th: w % 2 == 1), "an odd frame width: indirectLightUpscaleFastKernel, no upscale + shade fusion"
    assert some(lambda w, h, tw, th: h % 2 == 1), "an odd frame height"
    assert some(lambda w, h, tw, th: w % 2 == 0 and tw % 2 == 1), "an even frame with an odd trace width: a half quad in the quad upscale / fused shade"
    assert some(lambda w, h, tw, th: tw % 8 != 0 and th % 8 != 0), "partial 8 x 8 trace groups"
    assert some(lambda w, h, tw, th: tw % 32 != 0 and th % 32 != 0), "partial 32-pixel culling tiles"
    assert some(lambda w, h, tw, th: tw % 64 != 0 and tw > 64), "a partial last 64-texel spatial filter tile behind whole ones"
    assert some(lambda w, h, tw, th: w % 62 != 0), "a partial last TAA strip"
    assert some(lambda w, h, tw, th: h % 16 != 0), "a partial last block of TAA strip rows"
    assert some(lambda w, h, tw, th: h % 4 != 0), "a partial last row of the 64 x 4 kernels"
    assert some(lambda w, h, tw, th: tw > 1536), "a trace image from 1536 texels wide: the spatial filter's two-XCD-column walk"
    assert some(lambda w, h, tw, th: tw < 64), "a trace image narrower than one 64-texel tile"
    assert all(wh in SIZES for wh in TAA_SIZES + SPATIAL_FULL_RES_SIZES)
    assert any(w % 62 != 0 and h % 16 != 0 for w, h in TAA_SIZES) and any(w % 64 != 0 and h % 4 != 0 for w, h in TAA_SIZES)
    assert any(w % 2 == 1 for w, h in SPATIAL_FULL_RES_SIZES) and any(w % 64 != 0 and h % 4 != 0 for w, h in SPATIAL_FULL_RES_SIZES)


@pytest.fixture(scope="module", params=SIZES, ids=_ids)
def rs(request, backend):
    w, h = request.param
    s = pp.build_state(backend, w, h)
    s.W, s.H, s.TW, s.TH = w, h, w // 2, h // 2
    yield s
    s.fp.destroy()
    backend.setMathMode(False)


def _size(s):
    return s.W, s.H, s.TW, s.TH


@pytest.mark.gpu
def test_gpu_ragged_trace(backend, rs):
    pp.check_trace(backend, rs, *_size(rs))


@pytest.mark.gpu
@pytest.mark.parametrize("which,filter_index", [("spatial0", 0), ("spatial1", 1)])
def test_gpu_ragged_spatial_filter(backend, rs, which, filter_index):
    pp.check_spatial_filter(backend, rs, *_size(rs), which, filter_index)


@pytest.mark.gpu
def test_gpu_ragged_temporal_filter(backend, rs):
    pp.check_temporal_filter(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_upscale(backend, rs):
    pp.check_upscale(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_deferred_shading(backend, rs):
    pp.check_deferred_shading(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_upscale_and_shade(backend, rs):
    pp.check_fused_upscale_and_shade(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_taa(backend, rs):
    pp.check_taa(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_bloom(backend, rs):
    pp.check_bloom(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_tonemap_and_exposure(backend, rs):
    pp.check_tonemap_and_exposure(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_hiz_and_depth_downscale_bit_exact(backend, rs):
    pp.check_hiz_and_depth_downscale(backend, rs, *_size(rs))


@pytest.mark.gpu
def test_gpu_ragged_frame_end_to_end(backend, rs):
    pp.check_frame_end_to_end(backend, rs, *_size(rs))


@pytest.mark.gpu
@pytest.mark.parametrize("rs", TAA_SIZES, ids=["%dx%d" % wh for wh in TAA_SIZES], indirect=True)
@pytest.mark.parametrize("clip,dilate,tech,tonemap", TAA_VARIANTS)
def test_gpu_ragged_taa_every_history_sampler(backend, rs, clip, dilate, tech, tonemap):
    pp.check_taa(backend, rs, *_size(rs), clip, dilate, tech, tonemap, name="taa %d/%d/%d/%d" % (clip, dilate, tech, tonemap))


@pytest.mark.gpu
@pytest.mark.parametrize("rs", SPATIAL_FULL_RES_SIZES, ids=["%dx%d" % wh for wh in SPATIAL_FULL_RES_SIZES], indirect=True)
@pytest.mark.parametrize("filter_index", [0, 1])
def test_gpu_ragged_spatial_filter_on_a_full_resolution_grid(backend, rs, filter_index):
    pp.check_spatial_filter_full_res(backend, rs, *_size(rs), filter_index)


def test_count_caps_are_the_rate_caps_at_the_benchmarked_size():
    """at 3840 x 2160 every count cap allows exactly the counts the rate cap `count / n <= rate` it replaced allowed"""
    W, H = 3840, 2160
    for rate, n in [(1e-5, W * H // 4), (5e-4, 32 * W * H // 4), (3e-3, W * H), (2e-3, W * H), (1e-4, W * H), (5e-3, W * H), (5e-4, W * H), (1e-4, 4 * W * H),
                    (1e-3, 32 * W * H)]:
        cap = pp.count_cap(rate, n)
        assert cap / n <= rate and (cap + 1) / n > rate, (rate, n, cap)
    assert pp.count_cap(1e-5, 161 * 91) == pp.FLIP_FLOOR


def test_edge_mask_holds_the_last_partial_blocks_and_the_border():
    m = pp.edge_mask(322, 182, *pp.TAA_STRIP_BLOCK)
    assert m[:, 310:].all() and m[176:, :].all() and m[:2].all() and m[:, :2].all()
    assert not m[2:176, 2:310].any()
    assert pp.histogram_counts_every_pixel(3840, 2160, 128) and not pp.histogram_counts_every_pixel(322, 182, 128)


def test_expected_histogram_total_is_the_oracles_at_ragged_sizes(oracle):
    """the partial-tile rule (pass_parity.expected_histogram_total) against the oracle's histogram of random colours at sizes the 32 x 32 tiles do not divide"""
    import struct

    import numpy as np

    import passes
    from plainrenderer_amd import pixfmt
    rng = np.random.default_rng(7)
    light = struct.pack("<5f", 1.0, 1.0, 1.0, 0.7, 1.0)
    for w, h in [(322, 182), (72, 40), (1000, 563)]:
        packed = pixfmt.pack_r11g11b10(np.exp(rng.uniform(-8.0, 8.0, (w * h, 3))).astype(np.float32))
        _, hist = passes.orc_histogram(packed, w, h, light)
        expected, ambiguous = pp.expected_histogram_total(packed, w, h, light, hist.size)
        assert int(hist.sum()) < w * h and abs(int(hist.sum()) - expected) <= ambiguous
