"""The per-pass checks of the PLR_MATH_FAST kernel set against the oracle (the tolerance statement of tests/parity.py), as functions of the state
`build_state(backend, W, H)` returns: tests/test_parity_fullsize.py runs them at the benchmarked 3840 x 2160, tests/test_parity_ragged.py at sizes no
kernel geometry divides, tests/test_variants_parity.py reuses the TAA and full-resolution spatial filter checks. Nothing here reads a module global of
a test: every check takes W, H and the trace size TW x TH (W // 2, H // 2: the half-resolution trace, frame_pipeline.cpp).

Caps on flipped decisions are COUNTS: `count_cap(rate, n)` = max(floor(rate * n), FLIP_FLOOR). floor(rate * n) is the integer form of the rate cap
`count / n <= rate` the full-size tests always had (the same number at 3840 x 2160); FLIP_FLOOR keeps one honest flip on a 161 x 91 image from
failing a test whose rate cap allows one in 100 000.

Edge regions: every pass whose kernel takes discrete decisions is also held to its cap on the pixels of the last (partial) block column and block row
of its launch geometry plus a 2-pixel image border (`edge_mask`), with the cap computed on the region's own pixel count. Clean pixels must meet the
bound everywhere already; this catches a kernel that is systematically wrong along one edge while the image-wide rate stays under its cap.
"""
import math
import struct

import numpy as np

import parity
import passes
from plainrenderer_amd import pixfmt
from util import F

U = pixfmt.unpack_half
FLIP_FLOOR = 2   # k of count_cap: flips a cap allows on any image, however small
EDGE_BORDER = 2  # pixels of every image border inside the edge region

# launch geometries (block width, block height in pixels of the output image) that edge regions follow
TRACE_BLOCK = (32, 32)          # the trace image's 32-pixel culling tiles (each holds whole 8 x 8 groups of sdfDiffuseTraceFastKernel)
SPATIAL_BLOCK = (64, 4)         # spatialFilterFastKernel tiles (gi_spatial_fast.hip PLR_SPATIAL_TX)
UPSCALE_QUAD_BLOCK = (128, 8)   # indirectLightUpscaleQuadKernel: 64 x 4 quads of 2 x 2 pixels
UPSCALE_BLOCK = (64, 4)         # indirectLightUpscaleFastKernel (sizes that are not exactly 2x the trace)
SHADE_BLOCK = (64, 4)           # the deferred shade and the fused upscale + shade
TAA_STRIP_BLOCK = (62, 16)      # temporalFilterStripKernel: 62 output columns, 4 waves x kStripRows rows (history samplers 0 and 4)
TAA_BLOCK = (64, 4)             # the 64 x 4 TAA kernel (history samplers 1 - 3)


class State:
    pass


def build_state(backend, W, H):
    """bench.py's scene; two frames of the C++ FramePipeline in PLR_MATH_FAST with the oracle frame run beside it on what the pipeline submitted"""
    import bench
    from oracle_frame import OracleFrame
    from plainrenderer_amd.frame import FramePipeline

    class A:
        grid, sdf_res, shadow_res, steps, warmup, profile_frames = 16, 64, 2048, 4, 0, 0
    s = State()
    backend.setMathMode(True)
    fp = FramePipeline(backend, W, H, shadow_map_res=2048)
    scene, cams, inputs = bench.build_scene(A, "cuda:0", W, H)
    inputs.upload(fp)
    ora = OracleFrame(inputs, W, H, 512, fp.settings)
    for f in range(2):
        fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
        s.general = backend.getGeneralKernelExecutions()
        frustum = backend.downloadUniformBuffer(fp.uniform_buffer("sdfCameraFrustum"), 192).tobytes()
        ora.capture = f == 1
        ora.frame(fp.submitted_globals(), fp.resolve_weights(), frustum, 5.0)
    s.fp, s.ora, s.inputs, s.cap, s.gp, s.gb, s.settings = fp, ora, inputs, ora.cap, ora.cap["global"], inputs.gb, fp.settings
    s.post_gpu = backend.downloadImage(fp.image("post1"), 0, np.uint32).copy()
    s.swap_gpu = backend.downloadImage(fp.image("swapchain"), 0, np.uint8).copy()
    s.hist_gpu = backend.downloadStorageBuffer(fp.storage_buffer("histogram"), 512, dtype=np.uint32).copy()
    return s


def report(name, **kv):
    print("PARITY %-14s %s" % (name, " ".join("%s=%s" % (k, ("%.6g" % v) if isinstance(v, float) else v) for k, v in kv.items())), flush=True)


def count_cap(rate, n, k=FLIP_FLOOR):
    """the largest count a rate cap `count / n <= rate` allows, and never fewer than k"""
    return max(int(math.floor(rate * n + 1e-9)), k)


def edge_mask(w, h, block_w, block_h, border=EDGE_BORDER):
    """bool [h, w]: the last block column and the last block row of a launch of block_w x block_h pixel blocks (the partial ones where the size is no
    multiple of the block), plus a border-pixel frame around the image"""
    m = np.zeros((h, w), bool)
    m[:, (w - 1) // block_w * block_w:] = True
    m[(h - 1) // block_h * block_h:, :] = True
    m[:border, :] = True
    m[h - border:, :] = True
    m[:, :border] = True
    m[:, w - border:] = True
    return m


def histogram_counts_every_pixel(W, H, n_bins):
    """histogramPerTile.comp:37-39 returns for an invocation outside the image before the shared bins are zeroed (:43-46) and written back (:61-64):
    bin b of a 32 x 32 tile reaches the histogram only if the tile's invocation (b % 32, b // 32) is inside the image (the oracle restates it,
    exposure_tonemap.cpp orc_histogram_per_tile). The histogram totals W * H only if every partial tile keeps all those invocations"""
    rw, rh = W % 32 or 32, H % 32 or 32
    return all(b % 32 < rw and b // 32 < rh for b in range(n_bins))


def expected_histogram_total(color_packed, W, H, light_bytes, n_bins):
    """-> (pixels, ambiguous): how many pixels the histogram counts under the rule of histogram_counts_every_pixel, from each pixel's own bin
    (histogramPerTile.comp:48-54) evaluated in float64; `ambiguous` pixels lie within 1e-3 of a bin boundary, where float32 may choose the other bin"""
    rgb = pixfmt.unpack_r11g11b10(np.asarray(color_packed, np.uint32).reshape(-1)).reshape(H, W, 3).astype(np.float64)
    exposure = struct.unpack_from("<f", light_bytes, 12)[0]  # LightBuffer.previousFrameExposure
    lum = rgb @ np.array([0.2126, 0.7152, 0.0722]) / exposure
    lo, hi = math.log(passes.MIN_LUM), math.log(passes.MAX_LUM)
    with np.errstate(divide="ignore"):
        x = (n_bins - 1) * np.clip((np.log(lum) - lo) / (hi - lo), 0.0, 1.0)
    bins = np.floor(x).astype(np.int64)
    ambiguous = (np.abs(x - np.rint(x)) < 1e-3) & (x > 0.0) & (x < n_bins - 1)
    yy, xx = np.mgrid[0:H, 0:W]
    kept = ((xx // 32) * 32 + bins % 32 < W) & ((yy // 32) * 32 + bins // 32 < H)  # the tile's invocation that writes this bin back is inside the image
    return int(kept.sum()), int(ambiguous.sum())


def fast_only(backend, what):
    """the pass just launched ran the PLR_MATH_FAST kernels: a launcher that hands a size to the general kernel would make a check vacuous"""
    n, names = backend.getGeneralKernelExecutions()
    assert n == 0, "%s: %d general-kernel executions (%s)" % (what, n, names)


def upscale_is_regular(W, H):
    """launchUpscale's quad kernel (and the fusion with the shade) needs the target to be exactly twice the half-resolution images"""
    return W % 2 == 0 and H % 2 == 0 and W // 2 >= 4


# ------------------------------------------------------------------ config 4: trace + denoise
def check_trace(backend, s, W, H, TW, TH):
    c = s.cap["trace"]
    args = (s.gb["depth"], s.gb["normal"], W, H, TW, TH, s.inputs.sky, 200, 100, c["light"], s.inputs.instance_bytes_patched, c["tiles"], 5.0, s.inputs.shadow_info,
            s.inputs.shadow_maps[c["cascade"]], s.inputs.shadow_res, s.gp)
    with passes.gpu_signature(backend, TW * TH) as sg:
        yg, cg = passes.gpu_sdf_trace(backend, *args, strict=True, cascade=c["cascade"])
    fast_only(backend, "trace")
    arr, n = s.ora._bindless(passes.orc.global_from_bytes(s.gp))
    with passes.orc_signature(TW * TH) as so:
        yo, co = passes.orc_sdf_trace(*args, arr, n, strict=True, cascade=c["cascade"])
    assert np.array_equal(yo, c["out"][0]) and np.array_equal(co, c["out"][1])  # the oracle reproduces its own frame (and the signature run changes nothing)
    counts = c["tiles"].reshape(-1, passes.TILE_UINTS)[:, 0]
    ray_flip = ((sg.words ^ so.words) & ~np.uint32(0x7F8)).reshape(TH, TW) != 0     # hit / shadow / zeroed / closest instance of the pixel's own ray
    take_flip = ((sg.words ^ so.words) & np.uint32(0x7F8)).reshape(TH, TW) != 0      # the resolve accepted different neighbours
    touched = (parity.dilate3x3(ray_flip) | take_flip).reshape(-1)                    # a flipped ray reaches its 8 neighbours through the 3x3 resolve
    got = np.concatenate([U(yg).reshape(-1, 4), U(cg).reshape(-1, 2)], axis=1)
    ref = np.concatenate([U(yo).reshape(-1, 4), U(co).reshape(-1, 2)], axis=1)
    bad = parity.half_violations(got, ref, floor_frac=2.0 ** -10)
    edge = edge_mask(TW, TH, *TRACE_BLOCK)
    n_edge = int(edge.sum())
    edge_flips = int((ray_flip | take_flip)[edge].sum())
    report("trace", rays_flipped=float(ray_flip.mean()), take_flipped=float(take_flip.mean()), pixels_touched=float(touched.mean()),
           clean_violations=int((bad & ~touched).sum()), touched_violations=float((bad & touched).mean()), max_tile_count=int(counts.max()), edge_flipped=edge_flips,
           edge_pixels=n_edge)
    assert not (bad & ~touched).any(), "pixels with identical ray decisions must agree to max(2^-7 |x|, 2^-10 max|x|)"
    assert ray_flip.sum() <= count_cap(1e-5, TW * TH), "hard cap (measured 4.8e-7 = one ray in two million): rays that resolve differently (hit / miss, owner, shadow bit)"
    assert take_flip.sum() <= count_cap(1e-5, TW * TH), "hard cap (measured 0): 3x3 neighbour masks that differ"
    assert ray_flip[edge].sum() <= count_cap(1e-5, n_edge) and take_flip[edge].sum() <= count_cap(1e-5, n_edge), "edge region: %d flips" % edge_flips
    assert np.isfinite(got).all() and np.abs(got - ref)[touched].max(initial=0.0) <= 2.0 * np.abs(ref).max()


def _flipped_samples(words_gpu, words_ora):
    xw = (words_gpu ^ words_ora).reshape(-1, 2)
    x = xw[:, 0] | xw[:, 1]                                      # bit i: sample i reads another texel than the oracle's sample i
    flipped = np.zeros(x.size, np.int32)
    for b in range(32):
        flipped += ((x >> np.uint32(b)) & np.uint32(1)).astype(np.int32)
    return flipped


def check_spatial_filter(backend, s, W, H, TW, TH, which, filter_index):
    c = s.cap[which]
    dsrc, dfmt, dw, dh = c["depth"]
    args = (c["inp"][0], c["inp"][1], TW, TH, dsrc, dfmt, dw, dh, s.gb["normal"], W, H, s.gp, filter_index)
    with passes.gpu_signature(backend, 2 * TW * TH) as sg:   # two words per pixel: x parities, y parities of the 32 samples' texels
        yg, cg = passes.gpu_gi_spatial(backend, *args)
    fast_only(backend, which)
    with passes.orc_signature(2 * TW * TH) as so:
        yo, co = passes.orc_gi_spatial(*args)
    assert np.array_equal(yo, c["out"][0])
    flipped_samples = _flipped_samples(sg.words, so.words)
    clean = flipped_samples == 0
    got = np.concatenate([U(yg).reshape(-1, 4), U(cg).reshape(-1, 2)], axis=1)
    ref = np.concatenate([U(yo).reshape(-1, 4), U(co).reshape(-1, 2)], axis=1)
    bad = parity.half_violations(got, ref, floor_frac=2.0 ** -10)
    # a pixel with k of its 32 samples on another texel: each sample carries at most weight 1 of a total >= (32 - k) * (smallest weight) - bounded
    # here by the spread of the input around the pixel: |delta| <= k / 32 * (max - min of the input image) is far too loose to be useful, so the
    # statement for flipped pixels is statistical: their error stays below 1/4 of the image's range and shrinks with k
    err = np.abs(got - ref).max(axis=1)
    edge = edge_mask(TW, TH, *SPATIAL_BLOCK).reshape(-1)
    edge_flips = int(flipped_samples[edge].sum())
    report(which, sample_flip_rate=float(flipped_samples.sum() / (32.0 * clean.size)), pixels_with_flip=float((~clean).mean()), clean_violations=int((bad & clean).sum()),
           flipped_pixel_violations=float((bad & ~clean).mean()), max_err_clean=float(err[clean].max()), max_err_flipped=float(err[~clean].max(initial=0.0)),
           scale=float(np.abs(ref).max()), edge_flipped_samples=edge_flips, edge_pixels=int(edge.sum()))
    assert not (bad & clean).any(), "pixels whose 32 samples read the same texels as the oracle's must agree to max(2^-7 |x|, 2^-10 max|x|)"
    assert flipped_samples.sum() <= count_cap(5e-4, 32 * clean.size), "hard cap (measured 1.2e-4): disc samples that land on a neighbouring texel"
    assert edge_flips <= count_cap(5e-4, 32 * int(edge.sum())), "edge region"
    assert err[~clean].max(initial=0.0) <= 0.5 * np.abs(ref).max()


def check_spatial_filter_full_res(backend, s, W, H, TW, TH, filter_index, tag=""):
    """the trace at full resolution (SDFTraceSettings::halfResTrace = false) filters on the D32 depth buffer: the unpacked three-gather kernel. Its W x H inputs
    are the captured half-resolution images upsampled by nearest texel (index clamped to the last texel: odd sizes have one full-res column / row more)"""
    c = s.cap["spatial%d" % filter_index]
    iy = np.minimum(np.arange(H) // 2, TH - 1)
    ix = np.minimum(np.arange(W) // 2, TW - 1)
    yf = np.ascontiguousarray(np.asarray(c["inp"][0]).reshape(TH, TW, 4)[iy][:, ix])
    cf = np.ascontiguousarray(np.asarray(c["inp"][1]).reshape(TH, TW, 2)[iy][:, ix])
    args = (yf, cf, W, H, s.gb["depth"], F.Depth32, W, H, s.gb["normal"], W, H, s.gp, filter_index)
    with passes.gpu_signature(backend, 2 * W * H) as sg:
        yg, cg = passes.gpu_gi_spatial(backend, *args)
    fast_only(backend, "spatial%d full-res" % filter_index)
    with passes.orc_signature(2 * W * H) as so:
        yo, co = passes.orc_gi_spatial(*args)
    flipped = _flipped_samples(sg.words, so.words)
    clean = flipped == 0
    got = np.concatenate([U(yg).reshape(-1, 4), U(cg).reshape(-1, 2)], axis=1)
    ref = np.concatenate([U(yo).reshape(-1, 4), U(co).reshape(-1, 2)], axis=1)
    bad = parity.half_violations(got, ref, floor_frac=2.0 ** -10)
    edge = edge_mask(W, H, *SPATIAL_BLOCK).reshape(-1)
    edge_flips = int(flipped[edge].sum())
    report("spatial%d full-res%s" % (filter_index, tag), sample_flip_rate=float(flipped.sum() / (32.0 * clean.size)), clean_violations=int((bad & clean).sum()),
           edge_flipped_samples=edge_flips, edge_pixels=int(edge.sum()))
    assert not (bad & clean).any()
    assert flipped.sum() <= count_cap(1e-3, 32 * clean.size)
    assert edge_flips <= count_cap(1e-3, 32 * int(edge.sum())), "edge region"


def check_temporal_filter(backend, s, W, H, TW, TH):
    c = s.cap["temporal"]
    args = (*c["inp"], TW, TH, s.gb["motion"], s.gb["motion"], W, H, s.gp)
    tg = passes.gpu_gi_temporal(backend, *args)
    fast_only(backend, "temporal")
    got = np.concatenate([U(tg[0]).reshape(-1, 4), U(tg[1]).reshape(-1, 2)], axis=1)
    ref = np.concatenate([U(c["out"][0]).reshape(-1, 4), U(c["out"][1]).reshape(-1, 2)], axis=1)
    bad = parity.half_violations(got, ref, floor_frac=2.0 ** -10)
    report("temporal", violations=int(bad.sum()), max_err=float(np.abs(got - ref).max()), scale=float(np.abs(ref).max()))
    assert not bad.any()
    assert np.array_equal(tg[0], tg[2]) and np.array_equal(tg[1], tg[3])


def check_upscale(backend, s, W, H, TW, TH):
    c = s.cap["upscale"]
    args = (c["inp"][0], c["inp"][1], TW, TH, s.gb["depth"], c["half_depth"], W, H, s.gp)
    with passes.gpu_signature(backend, W * H) as sg:
        yg, cg = passes.gpu_gi_upscale(backend, *args)
    fast_only(backend, "upscale")
    with passes.orc_signature(W * H) as so:
        yo, co = passes.orc_gi_upscale(*args)
    assert np.array_equal(yo, c["out"][0])
    flip = sg.words != so.words
    got = np.concatenate([U(yg).reshape(-1, 4), U(cg).reshape(-1, 2)], axis=1)
    ref = np.concatenate([U(yo).reshape(-1, 4), U(co).reshape(-1, 2)], axis=1)
    bad = parity.half_violations(got, ref, floor_frac=2.0 ** -10)
    edge = edge_mask(W, H, *(UPSCALE_QUAD_BLOCK if upscale_is_regular(W, H) else UPSCALE_BLOCK)).reshape(-1)
    report("upscale", flipped=float(flip.mean()), clean_violations=int((bad & ~flip).sum()), edge_pixels=float((so.words & 1).mean()),
           edge_flipped=int(flip[edge].sum()), edge_region_pixels=int(edge.sum()))
    assert not (bad & ~flip).any()
    # the kernel evaluates both decisions with the shader's operation order, but its reciprocal is v_rcp_f32 (1 ulp) where the shader divides
    assert flip.sum() <= count_cap(3e-3, W * H), "hard cap: edge / closest-depth decisions"
    assert flip[edge].sum() <= count_cap(3e-3, int(edge.sum())), "edge region"


# ------------------------------------------------------------------ shade
def check_deferred_shading(backend, s, W, H, TW, TH):
    """On pixels with the oracle's cascade and lit-tap count every channel is within one R11G11B10 code of the oracle - a sentence that holds where the float64
    reference's `slack` is below a quarter of a code (tests/shade_reference.py, tests/test_shade_reference.py: at the max(r * r, 0.0045) roughness floor, with the
    normal on the half vector, two correct kernels are up to 7 codes apart). bench.py's scene has roughness >= 0.0625: the assertion covers all its pixels."""
    c, st = s.cap["shade"], s.settings
    args = (s.gb, W, H, s.ora.brdf_lut, 512, c["light"], s.inputs.shadow_info, s.inputs.shadow_maps, s.inputs.shadow_res, c["gi"][0], c["gi"][1], s.inputs.froxel,
            s.inputs.froxel_dims, s.inputs.vol_settings, s.inputs.sky, s.gp)
    var = (int(st.diffuse_brdf), int(st.direct_multiscatter), bool(st.use_geometry_aa), int(st.indirect_lighting_tech), int(st.sun_shadow_cascade_count))
    with passes.gpu_signature(backend, W * H) as sg:
        got = passes.gpu_deferred_shading(backend, *args, *var)
    fast_only(backend, "shade")
    arr, n = s.ora._bindless(passes.orc.global_from_bytes(s.gp))
    with passes.orc_signature(W * H) as so:
        ref = passes.orc_deferred_shading(*args, arr, n, *var)
    assert np.array_equal(ref, c["out"])
    flip = sg.words != so.words
    cascade_flip = ((sg.words ^ so.words) & 3) != 0
    d = parity.r11g11b10_code_diff(got, ref)
    sky = (so.words & 128) != 0
    worst_clean = d[~flip & ~sky].max()
    worst_sky = d[~flip & sky].max(initial=0)
    sky_over_1 = int((d[~flip & sky] > 1).any(axis=1).sum())
    lit = (so.words >> 2) & 15
    edge = edge_mask(W, H, *SHADE_BLOCK).reshape(-1)
    report("shade", pcf_flipped=float(flip.mean()), cascade_flipped=float(cascade_flip.mean()), clean_max_code_diff=int(worst_clean), sky_max_code_diff=int(worst_sky),
           sky_pixels_over_1_code=sky_over_1, clean_differing=float((d[~flip] != 0).any(axis=1).mean()),
           flipped_max_code_diff=int(d[flip].max(initial=0)), partially_lit=float(((lit > 0) & (lit < 12)).mean()), edge_flipped=int(flip[edge].sum()),
           edge_region_pixels=int(edge.sum()))
    assert worst_clean <= 1, "same cascade and the same number of lit PCF taps: every channel within one R11G11B10 code (where slack is below a quarter of a code: this scene)"
    # sky stand-in pixels (depth == 0): the synthetic sky LUT drops to 15 % between two rows just below the horizon, where the LUT's v coordinate is
    # sqrt-steep; a handful of pixels on that row pair differ by a second code
    assert worst_sky <= 2 and sky_over_1 <= count_cap(1e-4, int((~flip & sky).sum()))
    assert flip.sum() <= count_cap(2e-3, W * H), "hard cap (measured: profiles/r03_parity_4k.txt): pixels whose number of lit PCF taps differs from the oracle's"
    assert cascade_flip.sum() <= count_cap(1e-4, W * H)
    assert flip[edge].sum() <= count_cap(2e-3, int(edge.sum())), "edge region"
    # (no bound on HOW MANY taps of a flipped pixel differ: on a surface facing the light all twelve taps compare the same stored depth with the
    #  surface's own, and flip together)


def check_fused_upscale_and_shade(backend, s, W, H, TW, TH):
    """What the benchmark frame runs: indirectLightUpscale + the deferred shade as ONE launch (pass fusion; the upscaled texels never reach HBM at
    fusion level 2). The fused kernel writes both passes' decision signatures (shade word | upscale word << 8); held to the oracle's upscale
    followed by the oracle's shade, and to the two separate fast kernels' bytes. A size that is not exactly twice the trace's (odd W or H) does not
    fuse: the pair runs as the separate fast upscale and shade launches, and the upscale's words come from a signature run of the upscale alone."""
    cu, c, st = s.cap["upscale"], s.cap["shade"], s.settings
    var = (int(st.diffuse_brdf), int(st.direct_multiscatter), bool(st.use_geometry_aa), int(st.sun_shadow_cascade_count))
    assert int(st.indirect_lighting_tech) == 0
    fused = upscale_is_regular(W, H)
    common = (s.gb, W, H, s.ora.brdf_lut, 512, c["light"], s.inputs.shadow_info, s.inputs.shadow_maps, s.inputs.shadow_res)
    tail = (s.inputs.froxel, s.inputs.froxel_dims, s.inputs.vol_settings, s.inputs.sky, s.gp)
    with passes.gpu_signature(backend, W * H) as sg:
        got = passes.gpu_upscale_and_shade(backend, cu["inp"][0], cu["inp"][1], TW, TH, cu["half_depth"], *common, *tail, *var)
    fast_only(backend, "upscale + shade")
    up_args = (cu["inp"][0], cu["inp"][1], TW, TH, s.gb["depth"], cu["half_depth"], W, H, s.gp)
    if fused:
        assert backend.getPassFusion() == (2, 2), "the two executions ran inside one fused launch"
        words = sg.words
    else:
        assert backend.getPassFusion()[1] == 0, "a target that is not twice the half-resolution images does not fuse"
        with passes.gpu_signature(backend, W * H) as su_gpu:
            passes.gpu_gi_upscale(backend, *up_args)
        fast_only(backend, "upscale")
        words = (sg.words & 0xff) | (su_gpu.words << 8)   # the shade's words overwrote the upscale's in the pair's run
    with passes.orc_signature(W * H) as su:
        yo, co = passes.orc_gi_upscale(*up_args)
    arr, n = s.ora._bindless(passes.orc.global_from_bytes(s.gp))
    with passes.orc_signature(W * H) as so:
        ref = passes.orc_deferred_shading(*common, yo, co, *tail, arr, n, var[0], var[1], var[2], 0, var[3])
    assert np.array_equal(ref, c["out"])
    want = so.words | (su.words << 8)
    up_flip = (words >> 8) != (want >> 8)
    shade_flip = (words & 0xff) != (want & 0xff)
    d = parity.r11g11b10_code_diff(got, ref)
    sky = (so.words & 128) != 0
    clean = ~up_flip & ~shade_flip
    edge = edge_mask(W, H, *(UPSCALE_QUAD_BLOCK if fused else SHADE_BLOCK)).reshape(-1)
    n_edge = int(edge.sum())
    report("fused_upscale_shade" if fused else "upscale_then_shade", upscale_flipped=float(up_flip.mean()), pcf_flipped=float(shade_flip.mean()),
           clean_max_code_diff=int(d[clean & ~sky].max()), sky_max_code_diff=int(d[clean & sky].max(initial=0)), flipped_max_code_diff=int(d[~clean].max(initial=0)),
           edge_flipped=int((~clean)[edge].sum()), edge_region_pixels=n_edge)
    assert d[clean & ~sky].max() <= 1, ("same upscale texel choice, same cascade, same number of lit PCF taps: every channel within one R11G11B10 code (where slack is below a "
                                        "quarter of a code, tests/shade_reference.py: this scene)")
    assert d[clean & sky].max(initial=0) <= 2
    assert up_flip.sum() <= count_cap(3e-3, W * H) and shade_flip.sum() <= count_cap(2e-3, W * H)
    assert up_flip[edge].sum() <= count_cap(3e-3, n_edge) and shade_flip[edge].sum() <= count_cap(2e-3, n_edge), "edge region"
    # the fused launch equals the two separate fast kernels byte for byte (colour and, at level 1, the upscaled images)
    backend.setPassFusion(0)
    try:
        sep, ys, cs = passes.gpu_upscale_and_shade(backend, cu["inp"][0], cu["inp"][1], TW, TH, cu["half_depth"], *common, *tail, *var, download_upscaled=True)
        assert backend.getPassFusion() == (0, 0)
        fast_only(backend, "upscale + shade, fusion 0")
        backend.setPassFusion(1)
        one, y1, c1 = passes.gpu_upscale_and_shade(backend, cu["inp"][0], cu["inp"][1], TW, TH, cu["half_depth"], *common, *tail, *var, download_upscaled=True)
        fast_only(backend, "upscale + shade, fusion 1")
    finally:
        backend.setPassFusion(2)
    assert np.array_equal(sep, got) and np.array_equal(one, got)
    assert np.array_equal(ys, y1) and np.array_equal(cs, c1)
    if not fused:
        return
    # round 6 - the pair as TWO launches: the shade's direct lighting as the early part (beside the GI chain in a full frame; forced here, where the pair is all that is
    # recorded), then upscale + indirect + fog + pack. Its discrete decisions are the single launch's (the same statements), so the single launch's signatures say which
    # pixels are clean; held to the oracle with the same caps, and to the single launch within one code on EVERY pixel
    level = backend.getEarlyParts()[0]
    backend.setEarlyParts(2)
    try:
        split = passes.gpu_upscale_and_shade(backend, cu["inp"][0], cu["inp"][1], TW, TH, cu["half_depth"], *common, *tail, *var)
        assert backend.getEarlyParts() == (2, 1) and backend.getPassFusion() == (2, 2), "direct lighting launched as the early part, the rest as the fused launch"
        fast_only(backend, "early part + fused launch")
    finally:
        backend.setEarlyParts(level)
    ds = parity.r11g11b10_code_diff(split, ref)
    dd = parity.r11g11b10_code_diff(split, got)
    report("split_upscale_shade", clean_max_code_diff=int(ds[clean & ~sky].max()), sky_max_code_diff=int(ds[clean & sky].max(initial=0)),
           against_single_launch_max_code_diff=int(dd.max()), against_single_launch_differing=float((dd != 0).any(axis=1).mean()),
           clean_differing_from_oracle=float((ds[clean] != 0).any(axis=1).mean()), single_launch_clean_differing_from_oracle=float((d[clean] != 0).any(axis=1).mean()))
    assert ds[clean & ~sky].max() <= 1 and ds[clean & sky].max(initial=0) <= 2
    assert dd.max() <= 1, "two launches against one: the direct term travels in fp32, the indirect operands in fp16 - never more than one code"
    assert np.array_equal(split.reshape(-1)[sky.reshape(-1)], got.reshape(-1)[sky.reshape(-1)]), "sky pixels are packed by the direct launch from the same value"


# ------------------------------------------------------------------ config 3: TAA + bloom + HiZ
def check_taa(backend, s, W, H, TW, TH, clip=True, dilate=True, tech=4, tonemap=True, name="taa"):
    """TAA resolve (default: clip, dilate, Bicubic1Tap, tonemapped). The history fetch's texels and 8-bit sub-texel weights are placed as the shader
    places them (taa_fast.hip cubicAxis, texelCoord); what is left has no discrete decision a kernel could take differently from the oracle: every
    channel of every pixel within one code (measured on MI355X: at most 4e-4 of the pixels differ at all, profiles/r07_parity_ragged.txt)"""
    c = s.cap["taa"]
    args = (c["inp"], c["history"], s.gb["motion"], s.gb["depth"], W, H, c["weights"], s.gp, clip, dilate, tech, tonemap)
    og, hg = passes.gpu_taa(backend, *args)
    fast_only(backend, name)
    if (clip, dilate, tech, tonemap) == (True, True, 4, True):
        oo = c["out"]
    else:
        oo, _ = passes.orc_taa(*args)
    d = parity.r11g11b10_code_diff(og, oo)
    edge = edge_mask(W, H, *(TAA_STRIP_BLOCK if tech in (0, 4) else TAA_BLOCK)).reshape(-1)
    report(name, max_code_diff=int(d.max()), differing=float((d != 0).any(axis=1).mean()), over_one=float((d > 1).any(axis=1).mean()),
           edge_max_code_diff=int(d[edge].max()), edge_region_pixels=int(edge.sum()))
    assert d.max() <= 1, "every channel of every pixel within one R11G11B10 code"
    assert np.array_equal(og, hg)


def check_bloom(backend, s, W, H, TW, TH):
    c, st = s.cap["bloom"], s.settings
    out_g, downs_g, ups_g = passes.gpu_bloom(backend, c["inp"], W, H, float(st.bloom_strength), float(st.bloom_radius))
    fast_only(backend, "bloom")
    out_o, downs_o, ups_o = passes.orc_bloom(c["inp"], W, H, float(st.bloom_strength), float(st.bloom_radius))
    assert np.array_equal(out_o, c["out"])
    worst = 0
    for a, b in zip(downs_g + ups_g, downs_o + ups_o):
        worst = max(worst, int(parity.r11g11b10_code_diff(a, b).max()))
    d = parity.r11g11b10_code_diff(out_g, out_o)
    report("bloom", chain_max_code_diff=worst, applied_max_code_diff=int(d.max()), applied_differing=float((d != 0).any(axis=1).mean()))
    # every level re-quantises to R11G11B10 and feeds the next: a one-code difference at a coarse level can move a finer level's value across
    # a rounding boundary, never further
    assert worst <= 2 and d.max() <= 1


def check_tonemap_and_exposure(backend, s, W, H, TW, TH):
    c = s.cap["tonemap"]
    a = passes.gpu_tonemap(backend, c["inp"], W, H, s.gp, F.BGRA8_uNorm).astype(int).reshape(-1)
    fast_only(backend, "tonemap")
    d = np.abs(a - c["out"].astype(int).reshape(-1))
    report("tonemap", max_lsb=int(d.max()), differing=float((d != 0).mean()))
    assert d.max() <= 1
    # luminance histogram of the oracle's previous frame image: integer bins, bit exact
    _, hist_g = passes.gpu_histogram(backend, s.ora.color[s.ora.rt_index], W, H, s.ora.light)
    fast_only(backend, "histogram")
    _, hist_o = passes.orc_histogram(s.ora.color[s.ora.rt_index], W, H, s.ora.light)
    assert np.array_equal(hist_g, hist_o)
    if histogram_counts_every_pixel(W, H, hist_o.size):
        assert int(hist_o.sum()) == W * H
    expected, ambiguous = expected_histogram_total(s.ora.color[s.ora.rt_index], W, H, s.ora.light, hist_o.size)
    report("histogram", total=int(hist_o.sum()), expected=expected, ambiguous=ambiguous, pixels=W * H)
    assert abs(int(hist_o.sum()) - expected) <= ambiguous, "histogram total against the partial-tile rule of histogramPerTile.comp"


def check_hiz_and_depth_downscale(backend, s, W, H, TW, TH):
    """config 3's pyramid with the benchmarked kernels (kernels_fast/hiz_fast.hip: DPP quad / row reductions, 4x4 depth texels per lane) and the
    half-resolution depth the fused launch writes next to it: min / max and the half conversion are exact, so every level equals the oracle's bits"""
    depth = s.gb["depth"]
    levels_g, _, _ = passes.gpu_hiz(backend, depth, W, H)
    fast_only(backend, "hiz")
    levels_o = passes.orc_hiz(depth, W, H)
    assert len(levels_g) == len(levels_o) >= 6
    for m, (a, b) in enumerate(zip(levels_g, levels_o)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "pyramid level %d (%s)" % (m, a.shape)
    assert levels_o[-1].shape[:2] == (1, 1) and float(levels_o[-1][0, 0, 1]) == float(depth.max())
    # what the frame itself produced (depthHiZPyramid + depthDownscale recorded back to back: one fused launch)
    pyramid = s.fp.image("pyramid")
    for m in (0, 1, 2, 3, 4, len(levels_o) - 1):
        got = backend.downloadImage(pyramid, m, np.float32).reshape(levels_o[m].shape)
        assert np.array_equal(got.view(np.uint32), levels_o[m].view(np.uint32)), "frame pyramid level %d" % m
    half = backend.downloadImage(s.fp.image("depthHalfRes"), 0, np.uint16)
    assert np.array_equal(half.reshape(-1), passes.orc_depth_downscale(depth, W, H).reshape(-1))
    enabled, fused = backend.getPassFusion()
    report("hiz", levels=len(levels_o), fusion_enabled=enabled)


# ------------------------------------------------------------------ the whole frame, end to end (decision flips propagate through the chain here)
def check_frame_end_to_end(backend, s, W, H, TW, TH):
    """Two full frames of the C++ FramePipeline in PLR_MATH_FAST against the oracle frame. A flipped ray / sample / PCF tap of an early pass
    is carried through denoise, shade, TAA and bloom, so the end-to-end statement is statistical; the per-pass checks carry the bound."""
    d = parity.r11g11b10_code_diff(s.post_gpu, s.ora.post1)
    within1 = (d <= 1).all(axis=1)
    within4 = (d <= 4).all(axis=1)
    sw = np.abs(s.swap_gpu.astype(int).reshape(-1) - s.ora.swapchain.astype(int).reshape(-1))
    lit = pixfmt.unpack_r11g11b10(s.post_gpu)
    ref = pixfmt.unpack_r11g11b10(s.ora.post1)
    mean_rel = float(np.abs(lit - ref).mean() / ref.mean())
    hist_equal = float((s.hist_gpu == s.ora.hist).mean())
    report("frame", within_one_code=float(within1.mean()), within_4_codes=float(within4.mean()), max_code_diff=int(d.max()), swapchain_within_1lsb=float((sw <= 1).mean()),
           swapchain_max_lsb=int(sw.max()), mean_rel_err=mean_rel, histogram_bins_equal=hist_equal, histogram_total=int(s.hist_gpu.sum()), general_kernels=s.general[0])
    assert s.general[0] == 0, "the fast frame ran general kernels: %s" % (s.general[1],)
    assert np.isfinite(lit).all()
    # measured on MI355X at 3840 x 2160: 99.989 % within one code (round 2, before the shade's light-space geometry followed the shader's operation order: 98.04 %)
    assert (~within1).sum() <= count_cap(5e-3, W * H), "at least 99.5 % of the pixels of the final HDR image within one R11G11B10 code of the oracle frame"
    assert (~within4).sum() <= count_cap(5e-4, W * H)
    assert (sw > 1).sum() <= count_cap(1e-4, sw.size), "tonemapped swapchain: 99.99 % of the channels within 1 LSB"
    assert mean_rel <= 2e-3
    if histogram_counts_every_pixel(W, H, s.hist_gpu.size):
        assert int(s.hist_gpu.sum()) == W * H
    else:
        assert 0 < int(s.hist_gpu.sum()) < W * H
