"""numpy reference of the texture store built on the GPU (plrf_build_scene_textures: "textureMipChain.comp", "textureBlockEncode.comp"), written from the contract
text (DESIGN.md "Texture store built on the GPU"; csrc/device/texture_build.h, csrc/kernels/texture_build.hip and csrc/frontend/scene_packing.cpp implement the same
contracts independently and must agree byte for byte).

Four parts:
  the chain          level l + 1 from level l: per byte (a + b + c + d + 2) >> 2 of the clamped 2 x 2 taps
  block gathering    block (bx, by) takes texel (min(4 bx + i, W - 1), min(4 by + j, H - 1)) at position 4 j + i
  the encoders       the range-fit colour block and alpha block; their palettes are the DECODE contract's, taken from prepass_bc_reference's decoders and not re-stated
  the store          what plrf_build_scene_textures leaves in the texel store for a list of sources: prepass_bc_reference.pack_store of the textures with all levels
"""
import numpy as np

import prepass_bc_reference as bref
import prepass_texture_reference as tref

RGBA8, BC1, BC3, BC5 = bref.RGBA8, bref.BC1, bref.BC3, bref.BC5
U32 = np.uint32


# ---- the chain
def next_level(level):
    """h x w uint32 words -> max(1, h >> 1) x max(1, w >> 1)"""
    level = np.ascontiguousarray(level, U32)
    h, w = level.shape
    nw, nh = max(1, w >> 1), max(1, h >> 1)
    x0, x1 = np.minimum(2 * np.arange(nw), w - 1), np.minimum(2 * np.arange(nw) + 1, w - 1)
    y0, y1 = np.minimum(2 * np.arange(nh), h - 1), np.minimum(2 * np.arange(nh) + 1, h - 1)
    b = level.view(np.uint8).reshape(h, w, 4).astype(np.uint32)
    s = b[y0][:, x0] + b[y0][:, x1] + b[y1][:, x0] + b[y1][:, x1] + 2
    return np.ascontiguousarray((s >> 2).astype(np.uint8)).view(U32).reshape(nh, nw)


def chain(level0):
    """every level of the full chain of an h x w level 0, level 0 first"""
    levels = [np.ascontiguousarray(level0, U32)]
    while levels[-1].shape != (1, 1):
        levels.append(next_level(levels[-1]))
    return levels


def split_levels(words, width, height, mips):
    """the levels of `mips` RGBA8 levels stored back to back"""
    words, out, at = np.asarray(words, U32).reshape(-1), [], 0
    for l in range(mips):
        w, h = tref.level_size(width, height, l)
        out.append(words[at:at + w * h].reshape(h, w))
        at += w * h
    assert at == words.size
    return out


# ---- block gathering
def gather(level):
    """h x w words -> (blocks, 16) words, blocks row-major, position 4 j + i; positions beyond an edge repeat the edge texel"""
    level = np.asarray(level, U32)
    h, w = level.shape
    bw, bh = bref.level_blocks(w, h)
    ys, xs = np.minimum(np.arange(4 * bh), h - 1), np.minimum(np.arange(4 * bw), w - 1)
    return level[ys][:, xs].reshape(bh, 4, bw, 4).transpose(0, 2, 1, 3).reshape(bh * bw, 16)


# ---- the encoders
def colour_palette(c0, c1):
    """the decode contract's four colours of (c0, c1) in four-colour mode, N x 4 x 3: decoded from a block whose texel k has index k"""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    blocks = np.stack([c0 & 255, c0 >> 8, c1 & 255, c1 >> 8, np.full_like(c0, 0xE4), np.zeros_like(c0), np.zeros_like(c0), np.zeros_like(c0)], axis=1).astype(np.uint8)
    words = bref.decode_colour_blocks(blocks, True)[:, :4].astype(np.int64)
    return np.stack([(words >> (8 * c)) & 255 for c in range(3)], axis=2)


def alpha_palette(a0, a1):
    """the decode contract's eight values of (a0, a1), N x 8 (meaningful where a0 > a1): decoded from a block whose texel k has index k"""
    a0, a1 = np.asarray(a0, np.int64), np.asarray(a1, np.int64)
    bits = sum(k << (3 * k) for k in range(8))
    blocks = np.stack([a0, a1] + [np.full_like(a0, (bits >> (8 * k)) & 255) for k in range(6)], axis=1).astype(np.uint8)
    return bref.decode_alpha_blocks(blocks)[:, :8].astype(np.int64)


def colour_endpoints(t):
    """(blocks, 16) words -> c0, c1 (RGB565, c0 >= c1) by steps 1 - 4 of the colour block contract"""
    t = np.asarray(t, U32).astype(np.int64)
    n = t.shape[0]
    ch = np.stack([(t >> (8 * c)) & 255 for c in range(3)], axis=2)                  # blocks x 16 x 3
    lo, hi = ch.min(axis=1), ch.max(axis=1)
    m = np.argmax(hi - lo, axis=1)                                                   # the first of r, g, b on a tie
    rows = np.arange(n)
    dm = 2 * ch[rows, :, m] - (lo[rows, m] + hi[rows, m])[:, None]                   # blocks x 16
    s = (dm[:, :, None] * (2 * ch - (lo + hi)[:, None, :])).sum(axis=1)              # blocks x 3
    up = s >= 0
    up[rows, m] = True
    a, b = np.where(up, hi, lo), np.where(up, lo, hi)
    q5, q6 = (lambda v: (31 * v + 127) // 255), (lambda v: (63 * v + 127) // 255)
    e0 = (q5(a[:, 0]) << 11) | (q6(a[:, 1]) << 5) | q5(a[:, 2])
    e1 = (q5(b[:, 0]) << 11) | (q6(b[:, 1]) << 5) | q5(b[:, 2])
    return np.maximum(e0, e1), np.minimum(e0, e1)


def encode_colour_blocks(t):
    """(blocks, 16) words -> blocks x 8 uint8"""
    t = np.asarray(t, U32).astype(np.int64)
    c0, c1 = colour_endpoints(t)
    ch = np.stack([(t >> (8 * c)) & 255 for c in range(3)], axis=2)
    p = colour_palette(c0, c1)
    d = ((p[:, None, :, :] - ch[:, :, None, :]) ** 2).sum(axis=3)                    # blocks x 16 x 4
    k = np.argmin(d, axis=2)                                                         # the lowest k on a tie
    indices = np.where(c0 == c1, 0, sum(k[:, i] << (2 * i) for i in range(16)))
    return np.stack([c0 & 255, c0 >> 8, c1 & 255, c1 >> 8] + [(indices >> (8 * j)) & 255 for j in range(4)], axis=1).astype(np.uint8)


def alpha_choice(a0, a1, v):
    """the index the alpha block contract gives value v under endpoints a0 > a1 (arrays that broadcast), and the value that index decodes to"""
    shape = np.broadcast(a0, a1, v).shape
    p = alpha_palette(np.broadcast_to(a0, shape).reshape(-1), np.broadcast_to(a1, shape).reshape(-1)).reshape(shape + (8,))
    k = np.argmin(np.abs(p - np.asarray(v, np.int64)[..., None]), axis=-1)
    return k, np.take_along_axis(p, k[..., None], axis=-1)[..., 0]


def encode_alpha_blocks(v):
    """(blocks, 16) codes -> blocks x 8 uint8"""
    v = np.asarray(v).astype(np.int64)
    a0, a1 = v.max(axis=1), v.min(axis=1)
    k, _ = alpha_choice(a0[:, None], a1[:, None], v)
    bits = np.where(a0 == a1, 0, sum(k[:, i] << (3 * i) for i in range(16)))
    return np.stack([a0, a1] + [(bits >> (8 * j)) & 255 for j in range(6)], axis=1).astype(np.uint8)


def encode_blocks(fmt, t):
    """(blocks, 16) RGBA8 words -> blocks x (8 | 16) uint8"""
    t = np.asarray(t, U32)
    byte = lambda c: (t >> U32(8 * c)) & U32(255)
    if fmt == BC1:
        return encode_colour_blocks(t)
    if fmt == BC3:
        return np.concatenate([encode_alpha_blocks(byte(3)), encode_colour_blocks(t)], axis=1)
    return np.concatenate([encode_alpha_blocks(byte(0)), encode_alpha_blocks(byte(1))], axis=1)


def encode_level(fmt, level):
    """h x w words -> the bytes of the level's blocks"""
    return encode_blocks(fmt, gather(level)).tobytes()


# ---- the store
def store_levels(source):
    """(data, width, height, mips, format, store_format) -> (data of all levels as the store holds them, width, height, levels, store_format): a pack_store entry"""
    data, width, height, mips, fmt, stored = source
    full = tref.full_mip_count(width, height)
    assert fmt == RGBA8 or fmt == stored, "outside the table"
    if fmt == RGBA8:
        levels = split_levels(data, width, height, mips) if mips else chain(np.asarray(data, U32).reshape(height, width))
        if stored == RGBA8:
            return np.concatenate([l.reshape(-1) for l in levels]), width, height, len(levels), RGBA8
        return b"".join(encode_level(stored, l) for l in levels), width, height, len(levels), stored
    if mips:
        return bytes(data), width, height, mips, stored
    level0 = bytes(data)
    assert len(level0) == bref.level_words(fmt, width, height) * 4
    levels = chain(bref.decode_level(fmt, width, height, level0))[1:]  # level 0 stays the caller's blocks
    return level0 + b"".join(encode_level(stored, l) for l in levels), width, height, full, stored


def build_store(sources):
    """-> table (T x 4, word offsets), words, formats: the layout of prepass_bc_reference.pack_store for the textures with all their levels"""
    return bref.pack_store([store_levels(s) for s in sources])
