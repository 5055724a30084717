// "sunShadowRaster.comp": what the launcher (kernels/sun_shadow_raster.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's
// bindings and the layout of its scratch buffer. Plain C++: no device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "depth_prepass_raster.h"
#include "raster_record.h"

namespace plr {
namespace sunraster {

// the pass record (DESIGN.md "Sun shadow cascades as a compute pass")
constexpr int kSunShadowInfoBinding = 0, kTransformBinding = 1, kPositionBinding = 2, kIndexBinding = 3, kDrawBinding = 4, kScratchBinding = 5; // storage buffers
constexpr int kMapBinding = 0;                                                                                                                  // storage image, Depth16
constexpr uint32_t kCascadeIndexConstant = 0;
struct PushConstants { uint32_t drawCount, triangleCount; };
struct Draw { uint32_t firstIndex, indexCount, vertexOffset, transformIndex; };
// alpha-tested cutout casters (DESIGN.md "Alpha-tested cutout casters in the sun shadow raster"): the optional third push word; 0, or absent, is the opaque pass
// and bindings 6 - 9 are ignored. The texture store is the prepass's, under the prepass's binding numbers
struct CutoutPushConstants { uint32_t drawCount, triangleCount, textureCount; };
constexpr int kUvBinding = prepass::kUvBinding, kCasterMaterialBinding = prepass::kMaterialBinding, kTextureBinding = prepass::kTextureBinding,
              kTexelBinding = prepass::kTexelBinding; // storage buffers of a tested execution (textureCount > 0)
struct CasterMaterial { uint32_t albedoTexture, cutoff; }; // per draw; kNoTexture: alpha 255 everywhere; the kernel uses min(cutoff, 256), 0 = opaque
static_assert(sizeof(CasterMaterial) == 8, "caster material layout");
// block-compressed cutout textures (DESIGN.md "Block-compressed cutout textures in the sun shadow raster"): the optional fourth push word; 0, or absent, is the
// pass whose textures are all RGBA8 and binding 14 is ignored. 1: the texture store is the prepass's format-aware one - `texels` holds uint32 words, a compressed
// entry's texelOffset counts words - and binding 14 (the prepass's number) holds one format code per texture
struct FormatPushConstants { uint32_t drawCount, triangleCount, textureCount, textureFormats; };
constexpr int kTextureFormatBinding = prepass::kTextureFormatBinding;
using prepass::kTextureFormatBc1;
using prepass::kTextureFormatBc3;
using prepass::kTextureFormatBc5;
using prepass::kTextureFormatRgba8;
// which instantiation of the two kernels an execution runs: picked by the launcher from textureCount and textureFormats
constexpr int kAlphaUntested = 0, kAlphaRgba8 = 1, kAlphaFormats = 2;
using prepass::fullMipCount;
using prepass::kAlphaCutoffDiscardAll;
using prepass::kAlphaCutoffOpaque;
using prepass::kMaxTexels;
using prepass::kMaxTextureSize;
using prepass::kNoTexture;
using prepass::Texture;

// the contract's limits and the set-up record are the two rasterisers' (device/raster_record.h); this pass keeps its tile as 4096 words of LDS
using rastercov::kGuardBandPixels;
using rastercov::kMaxResolution;
using rastercov::kNarrowFlag;
using rastercov::kNarrowSpan;
using rastercov::kSubPixelBits;
using rastercov::kTileSize;
using rastercov::SetupRecord;

// scratch: header, then one 4-byte tile rectangle per surviving triangle (dense, for the tile kernel's scan), then one set-up record per surviving triangle
struct alignas(8) ScratchHeader {
    uint32_t cursor;    // surviving triangles = entries of the two arrays  } one 64-bit word for the set-up kernel's atomic: the cursor is the low half,
    uint32_t submitted; // triangles the draws hold                          } and it never carries (at most triangleCount < 2^32 survivors)
    uint32_t drawn;     // = cursor, copied by the tile kernel: back faces inside the guard band whose pixel box meets the map
    uint32_t guardBandRejects;
    uint32_t pad[12];
};
static_assert(sizeof(ScratchHeader) == 64, "ScratchHeader layout");

constexpr size_t rectOffset() { return sizeof(ScratchHeader); }
constexpr size_t recordOffset(uint32_t triangleCount) { return sizeof(ScratchHeader) + (((size_t)triangleCount * 4u + 15u) & ~(size_t)15u); }
constexpr size_t scratchBytes(uint32_t triangleCount) { return recordOffset(triangleCount) + (size_t)triangleCount * sizeof(SetupRecord); }

// a tested execution's record: the set-up record and what the alpha of a fragment needs beyond the weights - everything that depends on the triangle alone
struct alignas(16) CutoutRecord {
    SetupRecord s;
    uint32_t test;             // bits 0 - 8: kAlphaCutoffOpaque: the record takes the opaque path (c = 0, or no usable texture and c <= 255); kAlphaCutoffDiscardAll:
                               // it is dropped whole; else c of a sampled record. Bits 16 - 23: fw. Bit 24: L1 != L0. Bit 25 (a format-aware execution): the
                               // texture is BC3 - a sampled record is RGBA8 or BC3, a BC1 or BC5 one has alpha 255 everywhere and takes the opaque path
    uint32_t size0, size1;     // W | H << 16 of levels L0 and L1
    uint32_t base0Low, base0High; // the first texel of level L0 in `texels`, 64 bits; L1's is base0 + W_L0 H_L0 where L1 != L0. A BC3 record: the first word of
                               // L0's blocks, and L1's is base0 + 4 ceil(W_L0 / 4) ceil(H_L0 / 4)
    float u0, v0, u1, v1, u2, v2; // the vertices' UVs
    uint32_t pad;
};
static_assert(sizeof(CutoutRecord) == 128, "CutoutRecord layout");
// scratch of a tested execution: the same header and rectangles, 128-byte records: 64 + 16 ceil(T / 4) + 128 T bytes
constexpr size_t cutoutScratchBytes(uint32_t triangleCount) { return recordOffset(triangleCount) + (size_t)triangleCount * sizeof(CutoutRecord); }

} // namespace sunraster
} // namespace plr
