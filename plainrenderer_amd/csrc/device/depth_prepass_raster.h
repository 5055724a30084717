// "depthPrepassRaster.comp": what the launcher (kernels/depth_prepass_raster.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's
// bindings, the layout of its buffers and of its scratch buffer. Plain C++: no device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "raster_record.h"

namespace plr {
namespace prepass {

// the pass record (DESIGN.md "Depth prepass as a compute pass")
constexpr int kTransformBinding = 0, kPositionBinding = 1, kNormalBinding = 2, kIndexBinding = 3, kDrawBinding = 4, kScratchBinding = 5;                  // storage buffers
constexpr int kUvBinding = 6, kMaterialBinding = 7, kTextureBinding = 8, kTexelBinding = 9; // storage buffers of a textured execution (textureCount > 0)
constexpr int kAlphaCutoffBinding = 10; // storage buffer of an alpha-tested execution (alphaTest != 0): one uint32 cutoff code per draw
constexpr int kTangentBinding = 11, kBitangentBinding = 12, kNormalMaterialBinding = 13; // storage buffers of a normal-mapped execution (normalMap != 0)
constexpr int kTextureFormatBinding = 14; // storage buffer of a format-aware execution (textureFormats = 1): one uint32 format code per texture
constexpr int kDepthBinding = 0, kMotionBinding = 1, kNormalImageBinding = 2, kAlbedoBinding = 3, kSpecularBinding = 4;                                   // storage images
constexpr int kShadingNormalBinding = 5; // storage image of a normal-mapped execution: the per-pixel shading normal (RGBA8)
struct PushConstants { uint32_t drawCount, triangleCount; };
struct TexturedPushConstants { uint32_t drawCount, triangleCount, textureCount; }; // the optional third word: 0, or absent, is the untextured pass
struct AlphaPushConstants { uint32_t drawCount, triangleCount, textureCount, alphaTest; }; // the optional fourth word: 0, or absent, is the pass without the alpha test
struct NormalPushConstants { uint32_t drawCount, triangleCount, textureCount, alphaTest, normalMap; }; // the optional fifth word: 0, or absent, is the pass without normal maps
struct FormatPushConstants { uint32_t drawCount, triangleCount, textureCount, alphaTest, normalMap, textureFormats; }; // the optional sixth word: 0, or absent, is the pass whose textures are all RGBA8
struct AnisoPushConstants { uint32_t drawCount, triangleCount, textureCount, alphaTest, normalMap, textureFormats, maxAnisotropy; }; // the optional seventh word: 0, 1, or absent, is the pass with isotropic trilinear filtering
// the optional words 7 - 10 (a 44-byte record, words 0 - 6 as above and 0 where a feature is off): the tile window {x0, y0, x1, y1}, half-open, in 64 x 64 tiles of the
// bound images. The execution is the unwindowed one restricted to the pixels of those tiles; the four counters do not depend on it
struct WindowPushConstants { uint32_t drawCount, triangleCount, textureCount, alphaTest, normalMap, textureFormats, maxAnisotropy, windowTileX0, windowTileY0, windowTileX1, windowTileY1; };
static_assert(sizeof(WindowPushConstants) == 44, "the windowed pass record");
constexpr bool pushSizeDefined(size_t bytes) { return bytes == 8u || bytes == 12u || bytes == 16u || bytes == 20u || bytes == 24u || bytes == 28u || bytes == 44u; }
// anisotropic filtering ("Anisotropic filtering in the depth prepass"): maxAnisotropy 2 .. kMaxAnisotropy selects the anisotropic instantiations; the reference's
// sampler has 8 (ResourceDescriptions.h:169, VulkanSampler.cpp:23)
constexpr uint32_t kMaxAnisotropy = 16, kAnisotropyReference = 8;
struct Draw { uint32_t firstIndex, indexCount, vertexOffset, transformIndex, albedo, specular; }; // albedo, specular: RGBA8 texels as they are stored
struct MainPassMatrices { float model[16], mvp[16], mvpPrevious[16]; };                            // glm column-major (RenderFrontend.cpp:581-585)
// material textures ("The sampling contract"): `texels` holds RGBA8 texels, R in the low byte, every texture's levels back to back and unpadded; level l is
// row-major max(1, width >> l) x max(1, height >> l)
struct Texture { uint32_t texelOffset, width, height, mipCount; };  // texelOffset in texels
struct Material { uint32_t albedoTexture, specularTexture; };       // per draw; kNoTexture: the draw's constant word
constexpr uint32_t kNoTexture = 0xffffffffu;
// block-compressed textures ("Block-compressed textures in the depth prepass"): a format-aware execution's `textureFormats` holds one of these codes per texture.
// A compressed texture's levels are ceil(W_l / 4) x ceil(H_l / 4) blocks, row-major, back to back in `texels`; its texelOffset counts uint32 words and is a
// multiple of its block's words. A code above kTextureFormatBc5 makes the entry unusable
constexpr uint32_t kTextureFormatRgba8 = 0, kTextureFormatBc1 = 1, kTextureFormatBc3 = 2, kTextureFormatBc5 = 3;
constexpr uint32_t blockWords(uint32_t format) { return format == kTextureFormatBc1 ? 2u : 4u; } // of a compressed format: 8-byte and 16-byte blocks
// the uint32 words of all `mipCount` levels of a width x height texture of `format`
constexpr uint64_t textureWords(uint32_t format, uint32_t width, uint32_t height, uint32_t mipCount) {
    uint64_t words = 0;
    for (uint32_t l = 0; l < mipCount; l++) {
        const uint64_t w = (width >> l) ? (width >> l) : 1u, h = (height >> l) ? (height >> l) : 1u;
        words += format == kTextureFormatRgba8 ? w * h : ((w + 3u) / 4u) * ((h + 3u) / 4u) * blockWords(format);
    }
    return words;
}
constexpr uint32_t kMaxTextureSize = 16384;
constexpr uint64_t kMaxTexels = 1ull << 28;                         // what plrf_set_scene_textures accepts in total
// the alpha test ("The alpha test contract"): a draw's cutoff code c, 0 = opaque; a fragment passes when its alpha code is >= c. The kernel uses min(word, 256):
// a word above 255 discards every fragment of the draw
constexpr uint32_t kAlphaCutoffOpaque = 0, kAlphaCutoffReference = 128, kAlphaCutoffDiscardAll = 256;
// normal maps ("Normal maps in the depth prepass"): the fifth push-constant word selects the decode of the sampled texel; `tangents` and `bitangents` hold 3 floats
// per vertex, `normalMaterials` one texture index (or kNoTexture) per draw into the same textures / texels store
constexpr uint32_t kNormalDecodeReference = 1, kNormalDecodeUnit = 2;
constexpr uint32_t kNoWinner = 0xffffffffu; // what the tile kernel leaves in a shadingNormal texel without a winner, for the shading-normal kernel behind it
static_assert(sizeof(Texture) == 16 && sizeof(Material) == 8, "texture buffer layouts");
// the levels a width x height texture can have: floor(log2(max(width, height))) + 1
constexpr uint32_t fullMipCount(uint32_t width, uint32_t height) {
    uint32_t n = 1;
    for (uint32_t m = width > height ? width : height; m > 1u; m >>= 1) n++;
    return n;
}
static_assert(sizeof(Draw) == 24 && sizeof(MainPassMatrices) == 192, "pass buffer layouts");

using rastercov::kTileSize;                              // 64 x 64 64-bit keys: 32 KB of LDS per workgroup
using rastercov::kMaxResolution;
constexpr uint32_t kMaxTriangles = 1u << 28;             // 6 sub-triangles each still count in 32 bits
constexpr uint32_t kMaxSubTriangles = 6;                 // a triangle clipped by five planes has at most 8 vertices
constexpr float kGuardNdc = 32.f;                        // the four side planes of the clip volume: |x|, |y| <= 32 w

// scratch: header, one {draw, triangle within the draw} per submitted triangle (the resolve finds a winner's vertices through it), then one 4-byte tile
// rectangle and one set-up record per sub-triangle slot, 6 slots per triangle: nothing can overflow
struct alignas(8) ScratchHeader {
    uint32_t cursor;     // records appended = entries of the two arrays: the drawn sub-triangles whose tile rectangle meets the window } one 64-bit word for the set-up
    uint32_t submitted;  // triangles the draws hold                                                                               } kernel's atomic
    uint32_t drawn;      // sub-triangles with a non-empty box, counted by the set-up kernel (= cursor without a window)
    uint32_t rejects;    // triangles outside their buffers or with a non-finite clip component, and sub-triangles with a vertex w <= 0 or outside the 2^20-pixel band
    uint32_t clipped;    // triangles the clip changed
    uint32_t pad[11];
};
static_assert(sizeof(ScratchHeader) == 64, "ScratchHeader layout");

struct TriangleOrigin { uint32_t draw, local; };
struct alignas(16) Record {
    rastercov::SetupRecord s; // the sub-triangle with vertices 1 and 2 exchanged: A > 0, the shadow contract's record
    uint32_t t;               // the triangle's number in submission order
    uint32_t pad[3];
};
static_assert(sizeof(Record) == 96, "Record layout");

constexpr size_t originOffset() { return sizeof(ScratchHeader); }
constexpr size_t rectOffset(uint32_t triangleCount) { return (originOffset() + (size_t)triangleCount * sizeof(TriangleOrigin) + 15u) & ~(size_t)15u; }
constexpr size_t recordOffset(uint32_t triangleCount) { return (rectOffset(triangleCount) + (size_t)triangleCount * kMaxSubTriangles * 4u + 15u) & ~(size_t)15u; }
constexpr size_t scratchBytes(uint32_t triangleCount) { return recordOffset(triangleCount) + (size_t)triangleCount * kMaxSubTriangles * sizeof(Record); }

} // namespace prepass
} // namespace plr
