// The block decode contract (DESIGN.md "Block-compressed textures in the depth prepass") on the device: one text for every kernel that reads a BC1 / BC3 / BC5 level
// of the scene's texture store - the taps of "depthPrepassRaster.comp" and the reduction of "sceneMeanAlbedo.comp".
#pragma once
#include <stdint.h>

#include "depth_prepass_raster.h"
#include "detmath.h"

namespace plr {
namespace prepass {

// texel i of a colour block {c0 | c1 << 16, indices} as r | g << 8 | b << 16
PLR_DI uint32_t colourBlockTexel(uint32_t endpoints, uint32_t indices, uint32_t i, bool alwaysFour) {
    const uint32_t c0 = endpoints & 0xffffu, c1 = endpoints >> 16, k = (indices >> (2u * i)) & 3u;
    const bool four = alwaysFour || c0 > c1;
    uint32_t word = 0u;
    for (int ch = 0; ch < 3; ch++) { // red in the high bits of the RGB565 word
        const uint32_t shift = ch == 0 ? 11u : ch == 1 ? 5u : 0u, bits = ch == 1 ? 6u : 5u;
        const uint32_t q0 = (c0 >> shift) & ((1u << bits) - 1u), q1 = (c1 >> shift) & ((1u << bits) - 1u);
        const uint32_t e0 = (q0 << (8u - bits)) | (q0 >> (2u * bits - 8u)), e1 = (q1 << (8u - bits)) | (q1 >> (2u * bits - 8u));
        uint32_t c;
        if (k == 0u) c = e0;
        else if (k == 1u) c = e1;
        else if (four) c = k == 2u ? (2u * e0 + e1 + 1u) / 3u : (e0 + 2u * e1 + 1u) / 3u;
        else c = k == 2u ? (e0 + e1 + 1u) >> 1 : 0u;
        word |= c << (8 * ch);
    }
    return word;
}
// texel i of an alpha block {a0 | a1 << 8 | the low 16 index bits << 16, the high 32 index bits}
PLR_DI uint32_t alphaBlockTexel(uint32_t lo, uint32_t hi, uint32_t i) {
    const uint32_t a0 = lo & 255u, a1 = (lo >> 8) & 255u;
    const uint32_t k = (uint32_t)(((((uint64_t)hi << 16) | (uint64_t)(lo >> 16)) >> (3u * i)) & 7ull);
    if (k == 0u) return a0;
    if (k == 1u) return a1;
    if (a0 > a1) return ((8u - k) * a0 + (k - 1u) * a1 + 3u) / 7u;
    if (k == 6u) return 0u;
    if (k == 7u) return 255u;
    return ((6u - k) * a0 + (k - 1u) * a1 + 2u) / 5u;
}
// the word of texel (x, y) of a compressed level (w texels wide, first word at `base`): the block's 64-bit word address is checked against wordCount before
// the load, a block that does not lie wholly inside reads 0. The loads are aligned: usableTexture refused an offset that is no multiple of the block size.
// kFirst == 3 (the alpha only): BC3 loads its alpha block alone, BC1 and BC5 load nothing
template <int kFirst>
PLR_DI uint32_t blockTexel(const uint32_t* texels, uint64_t wordCount, uint64_t base, uint32_t format, int w, int x, int y) {
    const uint32_t blockWords = format == kTextureFormatBc1 ? 2u : 4u;
    const uint64_t at = base + ((uint64_t)(y >> 2) * (uint64_t)(((uint32_t)w + 3u) >> 2) + (uint64_t)(x >> 2)) * (uint64_t)blockWords;
    if (at + (uint64_t)blockWords > wordCount) return 0u;
    const uint32_t i = 4u * ((uint32_t)y & 3u) + ((uint32_t)x & 3u);
    if (format == kTextureFormatBc1) {
        if constexpr (kFirst == 3) return 255u << 24;
        const uint2 b = *(const uint2*)(texels + at);
        return colourBlockTexel(b.x, b.y, i, false) | (255u << 24);
    }
    if (format == kTextureFormatBc3) {
        if constexpr (kFirst == 3) {
            const uint2 b = *(const uint2*)(texels + at);
            return alphaBlockTexel(b.x, b.y, i) << 24;
        }
        const uint4 b = *(const uint4*)(texels + at);
        return colourBlockTexel(b.z, b.w, i, true) | (alphaBlockTexel(b.x, b.y, i) << 24);
    }
    if constexpr (kFirst == 3) return 255u << 24; // BC5
    const uint4 b = *(const uint4*)(texels + at);
    return alphaBlockTexel(b.x, b.y, i) | (alphaBlockTexel(b.z, b.w, i) << 8) | (255u << 24);
}

} // namespace prepass
} // namespace plr
