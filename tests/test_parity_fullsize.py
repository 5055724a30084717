"""The BENCHMARKED kernel set (PLR_MATH_FAST) against the oracle at the BENCHMARKED size: BASELINE configs 3, 4 and the full frame at
3840x2160 with 256 SDF instances x 64^3 (bench.py's workload, frame 2 so that every history is populated).

Every HIP pass is fed exactly what the oracle pass consumed and is held to the tolerance statement of tests/parity.py: one storage
quantum per channel for every pixel whose discrete decisions agree with the oracle's (decision signatures, oracle/oracle.h), a hard cap
on the number of pixels where a float rounding flipped a decision, and a bound on what a flipped pixel may differ by. The checks
themselves live in tests/pass_parity.py (tests/test_parity_ragged.py runs them at sizes no kernel geometry divides).
PLR_PARITY_SIZE=WxH (multiples of 64) runs the same tests at another size. Measured numbers: profiles/r06f_parity_4k.txt.
"""
import os

import pytest

import pass_parity as pp
from plainrenderer_amd import pixfmt

W, H = (int(v) for v in os.environ.get("PLR_PARITY_SIZE", "3840x2160").split("x"))
TW, TH = W // 2, H // 2
U = pixfmt.unpack_half
State = pp.State
report = pp.report


def build_state(backend, W=W, H=H):
    return pp.build_state(backend, W, H)


@pytest.fixture(scope="module")
def fs(backend):
    s = build_state(backend)
    yield s
    s.fp.destroy()
    backend.setMathMode(False)


# ------------------------------------------------------------------ config 4: trace + denoise
@pytest.mark.gpu
def test_gpu_fullsize_trace(backend, fs):
    pp.check_trace(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
@pytest.mark.parametrize("which,filter_index", [("spatial0", 0), ("spatial1", 1)])
def test_gpu_fullsize_spatial_filter(backend, fs, which, filter_index):
    pp.check_spatial_filter(backend, fs, W, H, TW, TH, which, filter_index)


@pytest.mark.gpu
def test_gpu_fullsize_temporal_filter(backend, fs):
    pp.check_temporal_filter(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
def test_gpu_fullsize_upscale(backend, fs):
    pp.check_upscale(backend, fs, W, H, TW, TH)


# ------------------------------------------------------------------ shade
@pytest.mark.gpu
def test_gpu_fullsize_deferred_shading(backend, fs):
    pp.check_deferred_shading(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
def test_gpu_fullsize_fused_upscale_and_shade(backend, fs):
    pp.check_fused_upscale_and_shade(backend, fs, W, H, TW, TH)


# ------------------------------------------------------------------ config 3: TAA + bloom (+ HiZ: bit exact in tests/test_hiz_bloom_taa.py at 3840x2160)
@pytest.mark.gpu
def test_gpu_fullsize_taa(backend, fs):
    pp.check_taa(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
def test_gpu_fullsize_bloom(backend, fs):
    pp.check_bloom(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
def test_gpu_fullsize_tonemap_and_exposure(backend, fs):
    pp.check_tonemap_and_exposure(backend, fs, W, H, TW, TH)


@pytest.mark.gpu
def test_gpu_fullsize_hiz_and_depth_downscale_bit_exact(backend, fs):
    pp.check_hiz_and_depth_downscale(backend, fs, W, H, TW, TH)


# ------------------------------------------------------------------ the whole frame, end to end (decision flips propagate through the chain here)
@pytest.mark.gpu
def test_gpu_fullsize_frame_end_to_end(backend, fs):
    pp.check_frame_end_to_end(backend, fs, W, H, TW, TH)
