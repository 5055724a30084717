"""plrf_generate_noise in the frame pipeline (include/plr_frame.h; DESIGN.md "Noise textures as compute passes"), on a 256 x 144 pipeline with the froxel passes on.

After generate_noise(seed, BLUE | PERLIN) and one frame, noise0 .. noise3 and perlinNoise3D, downloaded, equal tests/noise_reference.py run on the host
functions' tables, and the status words equal the reference's. Six frames of that pipeline then equal, byte for byte in every output image, six frames of a
second pipeline that got the same bytes by upload - all four frameIndexMod4 textures are used -, with a second generation from another seed between frames 3 and
4 and the matching upload on the second pipeline: everything the frame derives from a noise texture (the fast deferred shade's tap table by noise-texel position)
has to rebuild itself when a pass writes the texture, as it does after an upload. A pipeline that never calls it records nothing: its noise images keep what was
uploaded and the status words stay zero. Both ranks of a two-band partition, given one seed, write the same bytes. Flags 0 or unknown bits are refused.
"""
import numpy as np
import pytest

import noise_cases as nc
from plainrenderer_amd import synth
from plainrenderer_amd.scene import Camera

W, H, FROXEL_DEPTH, N_FRAMES = 256, 144, 8, 6
FP_ARGS = dict(shadow_map_res=128, brdf_lut_res=16, froxel_depth=FROXEL_DEPTH, max_sdf_instances=64)
IMAGES = ["swapchain", "post1", "color0", "color1", "taaHistory0", "taaHistory1", "sceneLuminance0", "sceneLuminance1", "giYSH0", "giYSH1", "giCoCg0", "giCoCg1",
          "giHistoryYSH0", "giHistoryYSH1", "giHistoryCoCg0", "giHistoryCoCg1", "depthHalfRes", "pyramid", "volumeMaterialVolume", "scatteringTransmittanceVolume",
          "volumetricHistory0", "volumetricHistory1", "volumetricIntegrationVolume"]
BUFFERS = [("histogram", 512), ("light", 20)]


def _cams(n):
    return [Camera.look((15.0 + 0.03 * i, -7.0, -6.0 + 0.05 * i), (0.0, 0.16, 1.0), aspect=W / H) for i in range(n + 1)]


def _inputs(cams):
    from plainrenderer_amd.frame import SyntheticInputs
    scene = synth.SynthScene(grid=4, cell=8.0, seed_id=973)
    return SyntheticInputs(scene, cams[1], cams[0], W, H, sdf_res=16, shadow_res=128, froxel_depth=FROXEL_DEPTH, sun_direction=(0.35, -0.8, 0.45))


def _expected(seed):
    """what the generation must write, from the reference run on the host functions' tables"""
    from plainrenderer_amd import backend as b
    return nc.frame_noise(seed, b.noise_gaussian_table(32, 32).tobytes(), b.noise_perlin_gradients(seed, 8).tobytes())


ALWAYS_WRITTEN = ("swapchain", "post1", "color0", "color1", "taaHistory0", "taaHistory1", "volumetricIntegrationVolume")


def _outputs(be, fp):
    """every output image and buffer; None for an intermediate the fast set's fused launches kept in registers in this frame (pass fusion level 2, the default:
    the backend refuses its download rather than return an older frame's bytes) - the same images in both pipelines, which the comparison checks"""
    from plainrenderer_amd.backend import PlrError
    out = []
    for name in IMAGES:
        try:
            out.append(be.downloadImage(fp.image(name), 0, np.uint8).copy())
        except PlrError as e:
            assert "not written in the last frame" in str(e) and name not in ALWAYS_WRITTEN, (name, e)
            out.append(None)
    return out + [be.downloadStorageBuffer(fp.storage_buffer(name), size).copy() for name, size in BUFFERS]


def _upload_noise(be, fp, expected):
    textures, _, volume = expected
    for t in range(4):
        be.uploadImage(fp.image("noise%d" % t), textures[t])
    be.uploadImage(fp.image("perlinNoise3D"), volume)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_gpu_generated_noise_equals_the_reference_and_frames_equal_those_of_uploaded_noise(backend, fast):
    from plainrenderer_amd.frame import NOISE_BLUE, NOISE_PERLIN, FramePipeline
    cams = _cams(N_FRAMES)
    inputs = _inputs(cams)
    expected = [_expected(seed) for seed in nc.FRAME_SEEDS]
    backend.setMathMode(fast)
    results = {}
    try:
        for how in ("generated", "uploaded"):
            fp = FramePipeline(backend, W, H, run_volumetrics=1, **FP_ARGS)
            try:
                inputs.upload(fp)  # (seeded white noise in noise0 .. noise3: replaced below)
                if how == "generated":
                    assert not fp.noise_stats().any()
                    fp.generate_noise(nc.FRAME_SEEDS[0], NOISE_BLUE | NOISE_PERLIN)
                else:
                    _upload_noise(backend, fp, expected[0])
                out = []
                for f in range(N_FRAMES):
                    if f == 3:  # the second generation: what the frame has derived from the first must not survive it
                        if how == "generated":
                            fp.generate_noise(nc.FRAME_SEEDS[1])
                        else:
                            _upload_noise(backend, fp, expected[1])
                    fp.frame(cams[f + 1], 1.0 / 60.0, 0.5 + f / 60.0)
                    if fast:
                        general, which = backend.getGeneralKernelExecutions()
                        assert general == 0, which
                    if how == "generated" and f in (0, 3):
                        textures, status, volume = expected[0 if f == 0 else 1]
                        for t in range(4):
                            got = backend.downloadImage(fp.image("noise%d" % t)).reshape(32, 32, 2)
                            assert np.array_equal(got, textures[t]), "noise%d after frame %d: %d bytes differ from the reference" % (t, f, int((got != textures[t]).sum()))
                        got = backend.downloadImage(fp.image("perlinNoise3D")).reshape(32, 32, 32)
                        assert np.array_equal(got, volume), "perlinNoise3D after frame %d: %d bytes differ from the reference" % (f, int((got != volume).sum()))
                        assert np.array_equal(fp.noise_stats(), status), (fp.noise_stats().tolist(), status.tolist())
                    out.append(_outputs(backend, fp))
                if how == "uploaded":
                    assert not fp.noise_stats().any(), "a pipeline that never generates records no noise pass"
                    assert np.array_equal(backend.downloadImage(fp.image("noise2")).reshape(32, 32, 2), expected[1][0][2])
                results[how] = out
            finally:
                fp.destroy()
    finally:
        backend.setMathMode(False)
    what = IMAGES + [name for name, _ in BUFFERS]
    for f in range(N_FRAMES):
        for a, b, name in zip(results["generated"][f], results["uploaded"][f], what):
            assert (a is None) == (b is None), "%s was written in one pipeline's frame %d and kept in registers in the other's" % (name, f)
            if a is not None:
                assert np.array_equal(a, b), "%s differs between generated and uploaded noise in frame %d (%d bytes)" % (name, f, int((a != b).sum()))
    assert fast or all(a is not None for frame in results["generated"] for a in frame), "the exact set writes every image"
    assert not np.array_equal(expected[0][0][0], expected[1][0][0]), "the two seeds give different textures: the second generation changes what frames 3 .. 5 read"


@pytest.mark.gpu
def test_gpu_generate_noise_refuses_unknown_flags_and_both_bands_agree(backend):
    from plainrenderer_amd.backend import PlrError
    from plainrenderer_amd.frame import NOISE_BLUE, NOISE_PERLIN, FramePipeline
    cams = _cams(1)
    inputs = _inputs(cams)
    textures, status, volume = _expected(nc.FRAME_SEEDS[0])
    fp = FramePipeline(backend, W, H, **FP_ARGS)
    try:
        for flags in (0, 4, NOISE_BLUE | 8):
            with pytest.raises(PlrError, match="PLRF_NOISE_BLUE") as e:
                fp.generate_noise(1, flags)
            assert e.value.code == -1  # PLR_ERR_INVALID_ARGUMENT
        inputs.upload(fp)
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        assert not fp.noise_stats().any(), "a refused call records nothing"
        assert np.array_equal(backend.downloadImage(fp.image("noise0")).reshape(32, 32, 2), inputs.noise[0].reshape(32, 32, 2))
        # one kind alone: the other image keeps its bytes
        fp.generate_noise(nc.FRAME_SEEDS[0], NOISE_PERLIN)
        fp.frame(cams[1], 1.0 / 60.0, 0.5)
        assert np.array_equal(backend.downloadImage(fp.image("perlinNoise3D")).reshape(32, 32, 32), volume)
        assert np.array_equal(backend.downloadImage(fp.image("noise0")).reshape(32, 32, 2), inputs.noise[0].reshape(32, 32, 2))
    finally:
        fp.destroy()
    for rows in ((0, 64), (64, H)):  # (band rows start and end on multiples of 64, or at the last row)
        band = FramePipeline(backend, W, H, band_row_begin=rows[0], band_row_end=rows[1], **FP_ARGS)
        try:
            inputs.upload(band)
            band.generate_noise(nc.FRAME_SEEDS[0], NOISE_BLUE | NOISE_PERLIN)
            band.frame(cams[1], 1.0 / 60.0, 0.5)
            for t in range(4):
                assert np.array_equal(backend.downloadImage(band.image("noise%d" % t)).reshape(32, 32, 2), textures[t]), (rows, t)
            assert np.array_equal(backend.downloadImage(band.image("perlinNoise3D")).reshape(32, 32, 32), volume), rows
            assert np.array_equal(band.noise_stats(), status)
        finally:
            band.destroy()
