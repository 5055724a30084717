// "textureMipChain.comp" and "textureBlockEncode.comp": what the launchers (kernels/texture_build.hip), the frame pipeline (frontend/frame_pipeline.cpp) and the host
// packer and encoder (frontend/scene_packing.cpp) share - the pass records' bindings, the job tables, and THE ENCODE CONTRACT's arithmetic as functions that
// compile for the host and the device alike (DESIGN.md "Texture store built on the GPU"): the kernel and plr_encode_rgba8_to_bc evaluate one text. Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLR_TB_HD __host__ __device__ inline
#else
#define PLR_TB_HD inline
#endif

namespace plr {
namespace texbuild {

constexpr uint32_t kGroupLanes = 256;           // lanes of a workgroup of both passes: a destination texel, or a block, per lane
constexpr uint32_t kMaxChainLaunches = 14;      // levels 1 .. 14 of a 16384 texture
constexpr uint64_t kMaxStagingWords = 1ull << 28; // the RGBA8 staging chains of one build

// ---- "textureMipChain.comp": dispatch {groupCount, 1, 1}. One execution builds one level of every texture that still has one to build: the jobs
// [firstJob, firstJob + jobCount) of the job table, each with the first workgroup of its own. A lane builds one texel of the level by the chain rule of plr_frame.h
constexpr int kChainJobBinding = 0;     // ChainJob per job
constexpr int kChainStoreBinding = 1;   // the texel store: read (a level below that lives in the store) and written (an RGBA8 entry's chain)
constexpr int kChainStagingBinding = 2; // the RGBA8 staging chains; absent in a build without a compressed entry (stagingBound = 0)
struct ChainPushConstants { uint32_t firstJob, jobCount, groupCount, stagingBound; };
// src, dst: word offsets of the level below and of the level built; srcWidth x srcHeight: the level below. flags: bits 0 - 1 the format code of the level below
// (prepass::kTextureFormat*: a compressed one is read through the block decode), kChainSrcStaging / kChainDstStaging: which buffer an offset counts in
struct ChainJob { uint32_t firstGroup, src, dst, srcWidth, srcHeight, flags, pad0, pad1; };
static_assert(sizeof(ChainJob) == 32, "chain job layout");
constexpr uint32_t kChainFormatMask = 3u, kChainSrcStaging = 4u, kChainDstStaging = 8u;

// ---- "textureBlockEncode.comp": dispatch {groupCount, 1, 1}. One execution encodes every level of every texture the build compresses: a lane per block, the
// blocks of a job row-major from its first workgroup on. The RGBA8 level is read from the staging buffer, the blocks are written to the store
constexpr int kEncodeJobBinding = 0;     // EncodeJob per job
constexpr int kEncodeStoreBinding = 1;   // the texel store (written)
constexpr int kEncodeStagingBinding = 2; // the RGBA8 staging chains (read)
struct EncodePushConstants { uint32_t jobCount, groupCount; };
// src: word offset of the width x height RGBA8 level in the staging buffer; dst: word offset of its blocks in the store; format: kTextureFormatBc1 | Bc3 | Bc5
struct EncodeJob { uint32_t firstGroup, src, dst, width, height, format, pad0, pad1; };
static_assert(sizeof(EncodeJob) == 32, "encode job layout");

// ---- THE CHAIN RULE on four words: per byte (a + b + c + d + 2) >> 2, two bytes at a time (a byte sum is at most 1022: it does not reach the next lane's bits)
PLR_TB_HD uint32_t chainMean(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t m = 0x00ff00ffu;
    const uint32_t even = ((a & m) + (b & m) + (c & m) + (d & m) + 0x00020002u) >> 2;
    const uint32_t odd = (((a >> 8) & m) + ((b >> 8) & m) + ((c >> 8) & m) + ((d >> 8) & m) + 0x00020002u) >> 2;
    return (even & m) | ((odd & m) << 8);
}

// ---- THE ENCODE CONTRACT (DESIGN.md "Texture store built on the GPU"). t[16]: the gathered block, position 4 j + i, RGBA8 words with R in the low byte
PLR_TB_HD uint32_t q5(uint32_t v) { return (31u * v + 127u) / 255u; }
PLR_TB_HD uint32_t q6(uint32_t v) { return (63u * v + 127u) / 255u; }
PLR_TB_HD uint32_t expand5(uint32_t q) { return (q << 3) | (q >> 2); }
PLR_TB_HD uint32_t expand6(uint32_t q) { return (q << 2) | (q >> 4); }

// the colour block {c0 | c1 << 16, indices} of the r, g, b of t
PLR_TB_HD void encodeColourBlock(const uint32_t t[16], uint32_t out[2]) {
    uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t v = (t[i] >> (8 * c)) & 255u;
            lo[c] = v < lo[c] ? v : lo[c];
            hi[c] = v > hi[c] ? v : hi[c];
        }
    // the main channel: the largest range, the first of r, g, b on a tie
    uint32_t m = 0u;
    if (hi[1] - lo[1] > hi[m] - lo[m]) m = 1u;
    if (hi[2] - lo[2] > (m == 0u ? hi[0] - lo[0] : hi[1] - lo[1])) m = 2u;
    const int midM = (int)(m == 0u ? lo[0] + hi[0] : m == 1u ? lo[1] + hi[1] : lo[2] + hi[2]);
    int s[3] = {0, 0, 0}; // s_c = sum (2 m_i - lo_m - hi_m) (2 c_i - lo_c - hi_c): at most 16 x 255 x 255
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int dm = 2 * (int)((t[i] >> (8u * m)) & 255u) - midM;
#pragma unroll
        for (int c = 0; c < 3; c++) s[c] += dm * (2 * (int)((t[i] >> (8 * c)) & 255u) - (int)(lo[c] + hi[c]));
    }
    uint32_t A[3], B[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const bool up = (uint32_t)c == m || s[c] >= 0;
        A[c] = up ? hi[c] : lo[c];
        B[c] = up ? lo[c] : hi[c];
    }
    uint32_t c0 = (q5(A[0]) << 11) | (q6(A[1]) << 5) | q5(A[2]), c1 = (q5(B[0]) << 11) | (q6(B[1]) << 5) | q5(B[2]);
    if (c0 < c1) { const uint32_t x = c0; c0 = c1; c1 = x; }
    out[0] = c0 | (c1 << 16);
    out[1] = 0u;
    if (c0 == c1) return;
    // the decode contract's four-colour palette of (c0, c1)
    int p[4][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t e0 = c == 0 ? expand5((c0 >> 11) & 31u) : c == 1 ? expand6((c0 >> 5) & 63u) : expand5(c0 & 31u);
        const uint32_t e1 = c == 0 ? expand5((c1 >> 11) & 31u) : c == 1 ? expand6((c1 >> 5) & 63u) : expand5(c1 & 31u);
        p[0][c] = (int)e0; p[1][c] = (int)e1; p[2][c] = (int)((2u * e0 + e1 + 1u) / 3u); p[3][c] = (int)((e0 + 2u * e1 + 1u) / 3u);
    }
    uint32_t indices = 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        int best = 0x7fffffff;
        uint32_t bestK = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int d = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) { const int e = p[k][c] - (int)((t[i] >> (8 * c)) & 255u); d += e * e; }
            if (d < best) { best = d; bestK = (uint32_t)k; } // (strictly less: the lowest k on a tie)
        }
        indices |= bestK << (2 * i);
    }
    out[1] = indices;
}

// the alpha block {a0 | a1 << 8 | low 16 index bits << 16, high 32 index bits} of byte `shift / 8` of t
PLR_TB_HD void encodeAlphaBlock(const uint32_t t[16], uint32_t shift, uint32_t out[2]) {
    uint32_t a0 = 0u, a1 = 255u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t v = (t[i] >> shift) & 255u;
        a0 = v > a0 ? v : a0;
        a1 = v < a1 ? v : a1;
    }
    out[0] = a0 | (a1 << 8);
    out[1] = 0u;
    if (a0 == a1) return;
    int p[8];
    p[0] = (int)a0; p[1] = (int)a1;
#pragma unroll
    for (int k = 2; k < 8; k++) p[k] = (int)(((8u - (uint32_t)k) * a0 + ((uint32_t)k - 1u) * a1 + 3u) / 7u);
    uint64_t bits = 0u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int v = (int)((t[i] >> shift) & 255u);
        int best = 0x7fffffff;
        uint64_t bestK = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int d = p[k] > v ? p[k] - v : v - p[k];
            if (d < best) { best = d; bestK = (uint64_t)k; }
        }
        bits |= bestK << (3 * i);
    }
    out[0] |= (uint32_t)(bits & 0xffffull) << 16;
    out[1] = (uint32_t)(bits >> 16);
}

// one block of `format` (prepass::kTextureFormatBc1 = 1, Bc3 = 2, Bc5 = 3) as 2 or 4 words
PLR_TB_HD void encodeBlock(uint32_t format, const uint32_t t[16], uint32_t out[4]) {
    if (format == 1u) { encodeColourBlock(t, out); out[2] = out[3] = 0u; }
    else if (format == 2u) { encodeAlphaBlock(t, 24u, out); encodeColourBlock(t, out + 2); }
    else { encodeAlphaBlock(t, 0u, out); encodeAlphaBlock(t, 8u, out + 2); }
}

} // namespace texbuild
} // namespace plr
