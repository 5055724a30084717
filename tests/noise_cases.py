"""The cases of the noise passes' tests (test_noise_cpu.py, test_noise.py, test_noise_frame.py): the smallest shapes at which "blueNoiseVoidAndCluster.comp"
and "perlinNoise3D.comp" can still go wrong, and their reference results, computed once per session (tests/noise_reference.py) and shared.

Blue noise:  8 x 8 R8     N = 64: one wave of the block holds every pixel, 6 minority pixels
             20 x 12 RG8  N = 240 is no multiple of 64, not square (a pitch of H instead of W would show), two blocks
             32 x 32 RG8  the pipeline's shape: one pixel per lane
             64 x 64 R8   four pixels per lane; Gaussian entries that are denormal (368 of 4096) or 0 (1735)
Perlin:      8^3 g = 8 (every voxel on a cell corner: residual 0), 20^3 g = 8 (cells of 2.5 voxels), 32^3 g = 8 (the pipeline's), 12^3 g = 5 (neither a power of two)
"""
import functools

import numpy as np

import noise_reference as ref

SEEDS = (1, 2024)
# name -> (width, height, channels)
BLUE_CASES = {"8x8 R8": (8, 8, 1), "20x12 RG8": (20, 12, 2), "32x32 RG8": (32, 32, 2), "64x64 R8": (64, 64, 1)}
# swaps the prototype loop takes (DESIGN.md "Noise textures as compute passes", measured with the contract's hash for seeds 1 and 2024) against the cap N
SWAP_RANGE = {"8x8 R8": (1, 3), "20x12 RG8": (6, 11), "32x32 RG8": (31, 35), "64x64 R8": (135, 144)}
FIRST_STREAM = 0
# name -> (resolution, gridCellCount)
PERLIN_CASES = {"8^3 g8": (8, 8), "20^3 g8": (20, 8), "32^3 g8": (32, 8), "12^3 g5": (12, 5)}
PERLIN_SEED = 7

FRAME_SEEDS = (11, 12)  # test_noise_frame.py: the first generation, and the one between frames 3 and 4


@functools.lru_cache(maxsize=None)
def blue_channel(name, seed, channel):
    w, h, _ = BLUE_CASES[name]
    r = ref.blue_noise_channel(seed, FIRST_STREAM + channel, w, h)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def blue_texture(name, seed):
    """-> (bytes (H, W, channels) uint8, status (channels, 4) uint32), from numpy's own table"""
    w, h, channels = BLUE_CASES[name]
    out = np.zeros((h, w, channels), np.uint8)
    status = np.zeros((channels, 4), np.uint32)
    for c in range(channels):
        r = blue_channel(name, seed, c)
        out[:, :, c] = r["codes"].reshape(h, w)
        status[c] = (r["swaps"], r["converged"], r["ones"], 0)
    out.setflags(write=False)
    status.setflags(write=False)
    return out, status


@functools.lru_cache(maxsize=None)
def perlin(name):
    """-> (gradients (g^3, 4) float32, volume (R, R, R) uint8), from numpy's own gradients"""
    res, g = PERLIN_CASES[name]
    gradients = ref.perlin_gradients(PERLIN_SEED, g)
    volume = ref.perlin_volume(gradients, res, g)
    gradients.setflags(write=False)
    volume.setflags(write=False)
    return gradients, volume


@functools.lru_cache(maxsize=None)
def frame_noise(seed, table_bytes, gradient_bytes):
    """what plrf_generate_noise(seed, BLUE | PERLIN) must leave in noise0 .. noise3 and perlinNoise3D, on the tables given (the host functions', as bytes):
    -> ([4 x (32, 32, 2) uint8], (4, 2, 4) uint32 status, (32, 32, 32) uint8)"""
    table = np.frombuffer(table_bytes, np.float32)
    textures, status = [], np.zeros((4, 2, 4), np.uint32)
    for t in range(4):
        tex, st = ref.blue_noise_texture(seed, 2 * t, 2, 32, 32, table)
        textures.append(tex)
        status[t] = st
    volume = ref.perlin_volume(np.frombuffer(gradient_bytes, np.float32).reshape(-1, 4), 32, 8)
    return textures, status, volume
