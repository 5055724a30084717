"""The noise contract without a GPU (DESIGN.md "Noise textures as compute passes"): the two host tables of include/plr.h against numpy's, and what the numpy
reference of tests/noise_reference.py - the thing the GPU tests compare bytes with - itself has to satisfy.

Tables: plr_noise_gaussian_table and plr_noise_perlin_gradients equal the reference's to within 1 ulp of fp32 (two correct double exp / sin can round differently
onto fp32: the only freedom), and exactly wherever the value is 0 or 1.
Reference: ranks are a permutation of 0 .. N - 1 for every case; every case converges inside the N-swap cap, with the swap counts the contract's hash gives; a cap
of 1 on 20 x 12 ends flagged not converged with ranks that are still a permutation; the output is blue (mean power below 0.125 cycles per texel over the mean power of
the spectrum < 0.01; the white-noise seeds it starts from give about 1); the Perlin volume stays in [0, 255], is not constant, and wraps.
"""
import numpy as np
import pytest

import noise_cases as nc
import noise_reference as ref


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    assert not (np.signbit(a) != np.signbit(b))[(a != 0) | (b != 0)].any(), "a sign differs"
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("size", [(4, 4), (8, 8), (20, 12), (32, 32), (64, 64), (4, 64)], ids=lambda s: "%dx%d" % s)
def test_host_gaussian_table_equals_numpy_to_one_ulp(size):
    from plainrenderer_amd import backend
    got, want = backend.noise_gaussian_table(*size), ref.gaussian_table(*size)
    assert got.shape == want.shape == (size[0] * size[1],)
    d = _ulps(got, want)
    print("gaussian table %dx%d: %d of %d entries differ, at most %d ulp" % (size[0], size[1], int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1
    exact = (want == 0) | (want == 1)
    assert got[0] == 1 and exact.sum() >= 1 and np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32))


def test_gaussian_table_of_64_has_denormal_and_zero_entries():
    """the 64 x 64 case is there for these: the LUT arithmetic must keep denormals"""
    g = ref.gaussian_table(64, 64)
    tiny = np.finfo(np.float32).tiny
    assert int((g == 0).sum()) == 1735 and int(((g > 0) & (g < tiny)).sum()) == 368
    assert ref.gaussian_table(32, 32).min() > tiny  # the pipeline's table has neither


@pytest.mark.parametrize("seed,g", [(1, 8), (2024, 5), (7, 32), (3, 1), (nc.PERLIN_SEED, 8)])
def test_host_perlin_gradients_equal_numpy_to_one_ulp(seed, g):
    from plainrenderer_amd import backend
    got, want = backend.noise_perlin_gradients(seed, g), ref.perlin_gradients(seed, g)
    assert got.shape == want.shape == (g ** 3, 4)
    d = _ulps(got, want)
    print("perlin gradients seed %d g %d: %d of %d entries differ, at most %d ulp" % (seed, g, int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1
    exact = (want == 0) | (want == 1)
    assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)) and not got[:, 3].any()
    assert (want[:, 1] >= 0).all(), "the second component is sin rx sin rx, the reference's repeated sin rx"


def test_host_tables_refuse_sizes_outside_the_contract():
    from plainrenderer_amd import backend
    for size in ((3, 8), (8, 65), (0, 0)):
        with pytest.raises(backend.PlrError, match="outside 4 .. 64"):
            backend.noise_gaussian_table(*size)
    for g in (0, 33):
        with pytest.raises(backend.PlrError, match="1 .. 32"):
            backend.noise_perlin_gradients(1, g)


def test_hash_and_streams():
    assert int(ref.lowbias32(0)) == 0
    x = 1  # lowbias32(1) by hand
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(ref.lowbias32(1)) == x
    keys = {ref.stream_key(1, s) for s in range(9)}
    assert len(keys) == 9, "the eight blue-noise streams and the Perlin stream of a seed are distinct"
    assert ref.minority_count(64) == 6 and ref.minority_count(240) == 24 and ref.minority_count(1024) == 102 and ref.minority_count(4096) == 409


@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("name", list(nc.BLUE_CASES))
def test_reference_ranks_are_a_permutation_and_the_prototype_converges(name, seed):
    w, h, channels = nc.BLUE_CASES[name]
    n = w * h
    for c in range(channels):
        r = nc.blue_channel(name, seed, c)
        print("blue noise %-9s seed %4d channel %d: %d swaps of at most %d, converged %d, ones %d" % (name, seed, c, r["swaps"], n, r["converged"], r["ones"]))
        assert np.array_equal(np.sort(r["ranks"]), np.arange(n))
        assert r["converged"] == 1 and r["ones"] == ref.minority_count(n)
        lo, hi = nc.SWAP_RANGE[name]
        assert lo <= r["swaps"] <= hi < n


def test_reference_stops_at_the_swap_cap_flagged_and_still_ranks_every_pixel():
    r = ref.blue_noise_channel(nc.SEEDS[0], 0, 20, 12, max_swaps=1)
    assert (r["swaps"], r["converged"]) == (1, 0)
    assert np.array_equal(np.sort(r["ranks"]), np.arange(240))
    assert nc.blue_channel("20x12 RG8", nc.SEEDS[0], 0)["swaps"] > 1  # the same channel does need more


@pytest.mark.parametrize("seed", nc.SEEDS)
@pytest.mark.parametrize("name", ["32x32 RG8", "64x64 R8"])
def test_reference_output_is_blue(name, seed):
    w, h, channels = nc.BLUE_CASES[name]
    for c in range(channels):
        blue = ref.low_frequency_ratio(nc.blue_channel(name, seed, c)["codes"].reshape(h, w))
        white = ref.low_frequency_ratio(ref.white_noise(ref.stream_key(seed, c), w * h).reshape(h, w))
        print("spectrum %-9s seed %4d channel %d: low-frequency power ratio %.5f, of the white noise it starts from %.3f" % (name, seed, c, blue, white))
        assert blue < 0.01
        assert white > 0.5  # white: 1 in expectation; about 50 (32 x 32) or 200 bins lie below the cutoff


@pytest.mark.parametrize("name", list(nc.PERLIN_CASES))
def test_reference_perlin_volume_is_in_range_and_not_constant(name):
    res, g = nc.PERLIN_CASES[name]
    gradients, volume = nc.perlin(name)
    assert volume.shape == (res, res, res) and volume.dtype == np.uint8
    print("perlin %-8s: min %d, max %d, %d distinct values" % (name, volume.min(), volume.max(), np.unique(volume).size))
    if res == g:  # every voxel on a cell corner: residual 0, every dot 0, the value 0.5f -> 127
        assert (volume == 127).all()
    else:
        assert np.unique(volume).size > 8


@pytest.mark.parametrize("g", [5, 8])
def test_reference_perlin_volume_wraps(g):
    """plane x = 0 of a volume with R = 2 g equals what the cell-wrap rule gives for x = R (uv = 1: cell g wraps to cell 0, residual 0); the same for y and z"""
    res = 2 * g
    gradients = ref.perlin_gradients(nc.PERLIN_SEED, g)
    volume = ref.perlin_volume(gradients, res, g)  # [z, y, x]
    a, b = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    edge = np.full_like(a, res)
    assert np.array_equal(ref.perlin_volume(gradients, res, g, coords=(edge, b, a)), volume[:, :, 0])  # [z = a, y = b]
    assert np.array_equal(ref.perlin_volume(gradients, res, g, coords=(b, edge, a)), volume[:, 0, :])  # [z = a, x = b]
    assert np.array_equal(ref.perlin_volume(gradients, res, g, coords=(b, a, edge)), volume[0, :, :])  # [y = a, x = b]
    assert np.unique(volume[:, :, 0]).size > 1


def test_both_passes_are_registered_and_the_api_is_bound():
    import ctypes as C
    from plainrenderer_amd import backend, frame, supported_shaders
    have = set(supported_shaders())
    assert {"blueNoiseVoidAndCluster.comp", "perlinNoise3D.comp"} <= have
    lib = C.CDLL(backend.LIB_PATH)
    for symbol in ("plrf_generate_noise", "plrf_get_noise_stats", "plr_noise_gaussian_table", "plr_noise_perlin_gradients"):
        assert hasattr(lib, symbol), symbol
    assert (frame.NOISE_BLUE, frame.NOISE_PERLIN) == (1, 2)
    assert lib.plrf_generate_noise(None, 1, 3) != 0  # a null pipeline is an error, not a crash
