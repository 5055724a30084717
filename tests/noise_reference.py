"""numpy restatement of "blueNoiseVoidAndCluster.comp" and "perlinNoise3D.comp", written from the contract text (DESIGN.md "Noise textures as compute passes";
kernels/noise.hip, device/noise.h), not from the kernels: integers and IEEE fp32 operation for operation, float64 only where the contract names it (the two
tables, evaluated with np.exp / np.sin / np.cos and rounded once to fp32).

Every fp32 value below is a numpy float32 scalar or array, so each operation rounds once to fp32; numpy keeps denormals.
"""
import numpy as np

F32, U32 = np.float32, np.uint32
BLUE_STREAMS, PERLIN_STREAM = 8, 8  # streams 0 .. 7 = 2 texture + channel; stream 8 = the Perlin gradients
MIN_SIZE, MAX_SIZE = 4, 64
SQRT_3_4 = np.sqrt(F32(3) / F32(4))  # sqrt(3 / 4.f) in fp32, correctly rounded: 0x3f5db3d7


def lowbias32(x):
    """the hash on a uint32 scalar or array"""
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x.astype(U32)


def stream_key(seed, stream):
    return int(lowbias32((int(seed) ^ (0x9E3779B9 * (int(stream) + 1))) & 0xFFFFFFFF))


# ---- the two tables
def gaussian_table(width, height):
    """G[dy * W + dx]: exp, in float64 and rounded once, of the fp32 argument -float(r^2) / (2.f * (1.9f * 1.9f)) at the toroidal offset"""
    dx = np.minimum(np.arange(width), width - np.arange(width)).astype(np.int64)
    dy = np.minimum(np.arange(height), height - np.arange(height)).astype(np.int64)
    r2 = (dy[:, None] ** 2 + dx[None, :] ** 2).astype(F32)
    arg = -r2 / (F32(2) * (F32(1.9) * F32(1.9)))
    assert arg.dtype == F32
    return np.exp(arg.astype(np.float64)).astype(F32).reshape(-1)


def perlin_angles(seed, g):
    key = stream_key(seed, PERLIN_STREAM)
    c = np.arange(g ** 3, dtype=np.uint64)
    scale = F32(2) * F32(3.1415)

    def angle(offset):
        h = lowbias32((key + 2 * c + offset) & 0xFFFFFFFF)
        return ((h >> 8).astype(F32) * F32(2.0 ** -24)) * scale

    return angle(0), angle(1)


def perlin_gradients(seed, g):
    """(g^3, 4) float32, cell c = (x g + y) g + z: (sin rx cos ry, sin rx sin rx, cos rx, 0) in float64 from the fp32 angles, rounded once"""
    rx, ry = perlin_angles(seed, g)
    assert rx.dtype == F32
    rx, ry = rx.astype(np.float64), ry.astype(np.float64)
    out = np.zeros((g ** 3, 4), F32)
    out[:, 0] = (np.sin(rx) * np.cos(ry)).astype(F32)
    out[:, 1] = (np.sin(rx) * np.sin(rx)).astype(F32)  # the repeated sin rx is the reference's (Noise.cpp:444)
    out[:, 2] = np.cos(rx).astype(F32)
    return out


# ---- blue noise
def white_noise(key, n):
    return (lowbias32((key + np.arange(n, dtype=np.uint64)) & 0xFFFFFFFF) & 255).astype(np.int64)


def minority_count(n):
    return int(U32(F32(n) * F32(0.1)))


def binarise(white, ones):
    n = white.size
    cum = np.cumsum(np.bincount(white, minlength=256))
    target = F32(ones) / F32(n)
    threshold = 0
    for t in range(256):
        if F32(cum[t]) / F32(n) >= target:
            threshold = t
            break
    pattern = white <= threshold
    pattern &= np.cumsum(pattern) <= ones  # in index order, every set entry beyond the first `ones` is cleared
    return pattern


class _Lut:
    """the filter LUT of one channel: H x W fp32, every update one fp32 add or subtract per pixel"""

    def __init__(self, table, width, height):
        self.g = np.asarray(table, F32).reshape(height, width)
        self.w, self.h = width, height

    def influence(self, index):
        # influence of (x0, y0) on (x, y) = G[((y - y0) mod H) W + ((x - x0) mod W)]
        return np.roll(self.g, (index // self.w, index % self.w), axis=(0, 1)).reshape(-1)

    def fresh(self, pattern):
        lut = np.zeros(self.w * self.h, F32)
        for i in np.flatnonzero(pattern):  # index order, from 0.f
            lut = lut + self.influence(int(i))
        return lut


def tightest_cluster(lut, pattern):
    return int(np.argmax(np.where(pattern, lut, F32(-np.inf))))  # the largest value among the minority pixels; argmax takes the lowest index of a tie


def biggest_void(lut, pattern):
    return int(np.argmin(np.where(pattern, F32(np.inf), lut)))


def blue_noise_channel(seed, stream, width, height, table=None, max_swaps=None):
    """-> dict(ranks (N,) int64, codes (N,) uint8, swaps, converged, ones) of one channel. table: G (default: gaussian_table); max_swaps: the cap (default N)"""
    assert MIN_SIZE <= width <= MAX_SIZE and MIN_SIZE <= height <= MAX_SIZE
    n = width * height
    cap = n if max_swaps is None else int(max_swaps)
    f = _Lut(gaussian_table(width, height) if table is None else table, width, height)
    ones = minority_count(n)
    pattern = binarise(white_noise(stream_key(seed, stream), n), ones)
    assert int(pattern.sum()) == ones
    lut = f.fresh(pattern)
    swaps, converged = 0, 0
    while swaps < cap:
        removed = tightest_cluster(lut, pattern)
        pattern[removed] = False
        lut = lut - f.influence(removed)
        added = biggest_void(lut, pattern)
        if added == removed:
            pattern[removed] = True
            converged = 1
            break
        pattern[added] = True
        lut = lut + f.influence(added)
        swaps += 1
    prototype = pattern.copy()
    initial = f.fresh(prototype)
    ranks = np.full(n, -1, np.int64)
    pattern, lut = prototype.copy(), initial.copy()
    for rank in range(ones - 1, -1, -1):
        i = tightest_cluster(lut, pattern)
        pattern[i] = False
        lut = lut - f.influence(i)
        ranks[i] = rank
    pattern, lut = prototype.copy(), initial.copy()
    for rank in range(ones, n):
        i = biggest_void(lut, pattern)
        pattern[i] = True
        lut = lut + f.influence(i)
        ranks[i] = rank
    codes = ((ranks.astype(F32) + F32(0.5)) / F32(n) * F32(255)).astype(np.uint8)
    return dict(ranks=ranks, codes=codes, swaps=swaps, converged=converged, ones=ones)


def blue_noise_texture(seed, first_stream, channels, width, height, table=None):
    """-> (bytes (H, W, channels) uint8, status (channels, 4) uint32 {swaps, converged, ones, 0})"""
    out = np.zeros((height, width, channels), np.uint8)
    status = np.zeros((channels, 4), U32)
    for c in range(channels):
        r = blue_noise_channel(seed, first_stream + c, width, height, table)
        out[:, :, c] = r["codes"].reshape(height, width)
        status[c] = (r["swaps"], r["converged"], r["ones"], 0)
    return out, status


# ---- the Perlin volume
def corner_dot(gradients, g, cell, corner, residual):
    """dot(gradient of the wrapped cell, residual - corner) = (gx ox + gy oy) + gz oz"""
    ix, iy, iz = ((cell[k] + corner[k]) % g for k in range(3))
    grad = gradients[(ix * g + iy) * g + iz]
    o = [residual[k] - F32(corner[k]) for k in range(3)]
    return (grad[..., 0] * o[0] + grad[..., 1] * o[1]) + grad[..., 2] * o[2]


def _mix(a, b, t):
    return a * (F32(1) - t) + b * t


def perlin_volume(gradients, res, g, coords=None):
    """-> (R, R, R) uint8 indexed [z, y, x] (index = x + y R + z R^2). coords: evaluate at these integer (x, y, z) arrays instead (-> uint8 of their shape)"""
    gradients = np.asarray(gradients, F32).reshape(-1, 4)
    if coords is None:
        z, y, x = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij")
    else:
        x, y, z = coords
    uv = [np.asarray(v).astype(F32) / F32(res) for v in (x, y, z)]
    scaled = [u * F32(g) for u in uv]
    cell = [s.astype(np.int32) for s in scaled]
    residual = [F32(g) * u - c.astype(F32) for u, c in zip(uv, cell)]
    assert all(r.dtype == F32 for r in residual)
    d = {(cx, cy, cz): corner_dot(gradients, g, cell, (cx, cy, cz), residual) for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)}
    i00, i01 = _mix(d[0, 0, 0], d[0, 0, 1], residual[2]), _mix(d[0, 1, 0], d[0, 1, 1], residual[2])
    i10, i11 = _mix(d[1, 0, 0], d[1, 0, 1], residual[2]), _mix(d[1, 1, 0], d[1, 1, 1], residual[2])
    value = _mix(_mix(i00, i01, residual[1]), _mix(i10, i11, residual[1]), residual[0])
    value = value / SQRT_3_4
    value = value * F32(0.5) + F32(0.5)
    value = np.minimum(np.maximum(value, F32(0)), F32(1))
    assert value.dtype == F32
    return (value * F32(255)).astype(np.uint8)


# ---- what the spectrum test measures
def low_frequency_ratio(codes2d, cutoff=0.125):
    """mean power below `cutoff` cycles per texel (DC removed) over the mean power of the whole spectrum (DC removed)"""
    a = np.asarray(codes2d, np.float64)
    p = np.abs(np.fft.fft2(a - a.mean())) ** 2
    fy, fx = np.meshgrid(np.fft.fftfreq(a.shape[0]), np.fft.fftfreq(a.shape[1]), indexing="ij")
    r = np.hypot(fx, fy)
    keep = r > 0
    return float(p[keep & (r < cutoff)].mean() / p[keep].mean())
