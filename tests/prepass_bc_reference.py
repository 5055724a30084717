"""numpy reference of the block-compressed textures of "depthPrepassRaster.comp", written from the contract text (DESIGN.md "Block-compressed textures in the depth
prepass"; csrc/kernels/depth_prepass_raster.hip and csrc/frontend/scene_packing.cpp implement the same contract independently and must agree word for word).

Three parts:
  the decoder        BC1 / BC3 / BC5 blocks -> RGBA8 words, R in the low byte, in integers
  the packer         a store that mixes the four formats: table {word offset, width, height, mipCount}, words, format codes
  the sampler        decode_store turns such a store into the all-RGBA8 layout prepass_texture_reference, prepass_alpha_reference and prepass_normal_reference
                     understand - the out-of-range rule and the unusable-entry rules applied on the way - and those references, imported and not edited, do the rest

A texture store (a dict, as prepass_texture_reference describes, with two changes): `texels` are the uint32 words of the mixed store, `textures` rows carry word
offsets, and `formats` holds one format code per row.
"""
import numpy as np

import prepass_texture_reference as tref

RGBA8, BC1, BC3, BC5 = 0, 1, 2, 3
BLOCK_BYTES = {BC1: 8, BC3: 16, BC5: 16}
U32 = np.uint32


# ---- the decoder
def _expand565(c):
    """uint16 RGB565 (red in the high bits) -> r8, g8, b8"""
    c = c.astype(np.int64)
    r5, g6, b5 = (c >> 11) & 31, (c >> 5) & 63, c & 31
    return (r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)


def decode_colour_blocks(blocks, always_four):
    """blocks: N x 8 uint8 -> N x 16 words r | g << 8 | b << 16 (no alpha), texel i = 4 (y & 3) + (x & 3)"""
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    c0, c1 = b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8)
    indices = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)
    four = np.ones_like(c0, bool) if always_four else c0 > c1
    out = np.zeros((b.shape[0], 16), np.int64)
    for channel, (e0, e1) in enumerate(zip(_expand565(c0), _expand565(c1))):
        palette = np.stack([e0, e1, np.where(four, (2 * e0 + e1 + 1) // 3, (e0 + e1 + 1) >> 1), np.where(four, (e0 + 2 * e1 + 1) // 3, 0)], axis=1)
        for i in range(16):
            out[:, i] |= palette[np.arange(b.shape[0]), (indices >> (2 * i)) & 3] << (8 * channel)
    return out.astype(U32)


def decode_alpha_blocks(blocks):
    """blocks: N x 8 uint8 -> N x 16 codes"""
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    bits = sum(b[:, 2 + k] << (8 * k) for k in range(6))
    eight = a0 > a1
    palette = [a0, a1]
    for k in range(2, 8):
        six = np.full_like(a0, 0 if k == 6 else 255) if k >= 6 else ((6 - k) * a0 + (k - 1) * a1 + 2) // 5
        palette.append(np.where(eight, ((8 - k) * a0 + (k - 1) * a1 + 3) // 7, six))
    palette = np.stack(palette, axis=1)
    out = np.zeros((b.shape[0], 16), np.int64)
    for i in range(16):
        out[:, i] = palette[np.arange(b.shape[0]), (bits >> (3 * i)) & 7]
    return out.astype(U32)


def decode_blocks(fmt, blocks):
    """blocks: N x (8 | 16) uint8 -> N x 16 RGBA8 words"""
    b = np.asarray(blocks, np.uint8).reshape(-1, BLOCK_BYTES[fmt])
    if fmt == BC1:
        return decode_colour_blocks(b, False) | U32(0xFF000000)
    if fmt == BC3:
        return decode_colour_blocks(b[:, 8:], True) | (decode_alpha_blocks(b[:, :8]) << U32(24))
    return decode_alpha_blocks(b[:, :8]) | (decode_alpha_blocks(b[:, 8:]) << U32(8)) | U32(0xFF000000)


def level_blocks(width, height):
    return (width + 3) // 4, (height + 3) // 4


def level_words(fmt, width, height):
    if fmt == RGBA8:
        return width * height
    bw, bh = level_blocks(width, height)
    return bw * bh * BLOCK_BYTES[fmt] // 4


def texture_words(fmt, width, height, mips):
    return sum(level_words(fmt, *tref.level_size(width, height, l)) for l in range(mips))


def decode_level(fmt, width, height, data, valid=None):
    """one level: its blocks (bytes, row-major) -> height x width words. valid: per block, False where the block reads 0 (the out-of-range rule)"""
    bw, bh = level_blocks(width, height)
    words = decode_blocks(fmt, np.frombuffer(bytes(data), np.uint8).reshape(bw * bh, BLOCK_BYTES[fmt])).reshape(bh, bw, 4, 4)
    if valid is not None:
        words = np.where(np.asarray(valid, bool).reshape(bh, bw, 1, 1), words, U32(0))
    return words.transpose(0, 2, 1, 3).reshape(bh * 4, bw * 4)[:height, :width].copy()


def decode_chain(fmt, width, height, mips, data):
    """all levels of a compressed texture -> the RGBA8 texels of the same levels, back to back"""
    data, at, out = bytes(data), 0, []
    for l in range(mips):
        w, h = tref.level_size(width, height, l)
        n = level_words(fmt, w, h) * 4
        out.append(decode_level(fmt, w, h, data[at:at + n]).reshape(-1))
        at += n
    assert at == len(data), "%d bytes for levels of %d" % (len(data), at)
    return np.concatenate(out)


def random_blocks(fmt, count, seed):
    """count blocks of fmt with both orders of the endpoints, equal endpoints and every index"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (count, BLOCK_BYTES[fmt]), dtype=np.uint8)
    halves = [0] if fmt == BC1 else [8] if fmt == BC3 else []
    for at in halves:  # a colour block: every eighth one with c0 == c1
        b[::8, at + 2:at + 4] = b[::8, at:at + 2]
    for at in ([0] if fmt == BC3 else [0, 8] if fmt == BC5 else []):  # an alpha block: every eighth one with a0 == a1
        b[::8, at + 1] = b[::8, at]
    return b


# ---- the packer
def pack_store(textures):
    """[(data, width, height, mips, fmt)] - data: uint32 texels of all levels (RGBA8) or the bytes of all levels' blocks - -> table (T x 4 uint32, word offsets),
    words, formats. A compressed texture starts at a multiple of 4 words (16 bytes), zeros in front of it where needed; an RGBA8 one where the last ended"""
    table, words, formats, offset = [], [], [], 0
    for data, width, height, mips, fmt in textures:
        w = np.asarray(data, U32).reshape(-1) if fmt == RGBA8 else np.frombuffer(bytes(data), np.uint8).view(U32)
        assert w.size == texture_words(fmt, width, height, mips), (w.size, texture_words(fmt, width, height, mips))
        if fmt != RGBA8 and offset % 4:
            words.append(np.zeros(4 - offset % 4, U32))
            offset += 4 - offset % 4
        table.append((offset, width, height, mips))
        words.append(w)
        formats.append(fmt)
        offset += w.size
    return np.asarray(table, U32).reshape(-1, 4), np.concatenate(words) if words else np.zeros(0, U32), np.asarray(formats, U32)


# ---- the sampler
def _usable_shape(width, height, mips):
    return 1 <= width <= 16384 and 1 <= height <= 16384 and 1 <= mips <= tref.full_mip_count(width, height)


def decode_store(tex):
    """the mixed store as an all-RGBA8 store the existing references sample: every usable row's levels decoded texel by texel - a texel whose word (RGBA8) or whose
    block (compressed) does not lie wholly inside `texels` is 0 -, a row that is unusable (the shape rule, a format code above 3, a compressed row whose offset is
    no multiple of its block's words) gets width 0, which makes it the draw's constant word there too"""
    table = np.asarray(tex["textures"], U32).reshape(-1, 4)
    words = np.asarray(tex["texels"], U32).reshape(-1)
    formats = np.asarray(tex["formats"], U32).reshape(-1)
    out_table, out_texels, at = [], [], 0
    for row in range(table.shape[0]):
        offset, width, height, mips = (int(v) for v in table[row])
        fmt = int(formats[row]) if row < formats.size else RGBA8
        usable = _usable_shape(width, height, mips) and fmt <= BC5 and (fmt == RGBA8 or offset % (BLOCK_BYTES[fmt] // 4) == 0)
        if not usable:
            out_table.append((at, 0, height, mips))
            continue
        out_table.append((at, width, height, mips))
        for l in range(mips):
            w, h = tref.level_size(width, height, l)
            n = level_words(fmt, w, h)
            index = offset + np.arange(n, dtype=np.int64)
            level = np.where(index < words.size, words[np.minimum(index, max(words.size - 1, 0))] if words.size else 0, 0).astype(U32)
            if fmt == RGBA8:
                texels = level
            else:
                per = BLOCK_BYTES[fmt] // 4
                valid = index.reshape(-1, per)[:, -1] < words.size  # the block's last word is inside: the block lies wholly inside
                texels = decode_level(fmt, w, h, level.tobytes(), valid).reshape(-1)
            out_texels.append(texels)
            at += texels.size
            offset += n
    decoded = dict(tex, textures=np.asarray(out_table, U32).reshape(-1, 4), texels=np.concatenate(out_texels) if out_texels else np.zeros(0, U32))
    decoded.pop("formats")
    return decoded
