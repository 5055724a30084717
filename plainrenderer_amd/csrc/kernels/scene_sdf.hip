// "sdfInstanceUpdate.comp" and "sceneMeanAlbedo.comp": the SDF instances of the GI trace from the scene's meshes and transforms - SDFGI::updateSDFScene
// (Techniques/SDFGI.cpp:260-313, whose first line asks for a compute shader) and computeMeanAlbedo (ModelImport.cpp:78-112) as two compute passes
// (DESIGN.md "SDF instances from the scene"; plrf_set_scene_sdf). Both kernel sets run these kernels: every output is decided by a written contract.
//
// THE INSTANCE CONTRACT (device/scene_sdf.h holds the arithmetic, one text for this kernel and for the host's determinant test). fp32 IEEE operations in the
// order written, no contraction, fp64 where named. Lane i < instanceCount reads table[i] = {draw, sdfTextureIndex, local min, local max}; an entry whose draw is
// not below drawCount writes nothing. Lane 0 of the grid writes the header {instanceCount, 0, 0, 0} (also when instanceCount is 0). Then, with model =
// matrices[draw].model (glm column-major, element [c][r] at 4 c + r):
//   padded local box  pad = max(0.075f (max - min), 0.5f) per component, min - pad, max + pad: plr_sdf_padded_bounds operation for operation;
//                     localExtends = paddedMax - paddedMin; bbOffset = (paddedMin + paddedMax) 0.5f
//   world box         the eight corners of the UNPADDED local box (corner k takes max on the axes whose bit of k is set), component i of a corner
//                     ((m[0][i] x + m[1][i] y) + m[2][i] z) + m[3][i]; component min / max over k ascending with min(a, v) = v < a ? v : a, max(a, v) = a < v ? v : a;
//                     then the padding rule; sdfWorldBBs[i] = {min, 0, max, 0}
//   worldToLocal      L = model translate(bbOffset): columns 0 - 2 are model's, column 3 is the row rule at bbOffset, all four rows. inverse(L) is the adjugate
//                     over the determinant in fp64 from the promoted floats: the twelve 2 x 2 sub-determinants first (each p q - r s), det =
//                     ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0, each adjugate element three products combined left to right as inverseOf writes them,
//                     ONE division per element, one rounding to fp32. The host refuses a draw whose det is zero or not finite (plrf_set_scene_sdf,
//                     plrf_set_scene_mesh_transforms), so no element is a NaN; an element beyond fp32 is the infinity the rounding gives.
//                     This differs from the reference's fp32 glm::inverse in rounding only.
//   meanAlbedo        overrides[draw] where its red is not a NaN; else means[materials[draw].albedoTexture] where textureCount > 0 and the index is below it;
//                     else the mean albedo rule on the draw's constant albedo word as a one-texel image
//   padding           0
// Bytes of the two buffers beyond instance instanceCount - 1 are not written.
//
// THE MEAN ALBEDO CONTRACT. Per texture that some draw's material names as albedo, over level 0: per texel term_c = (uint)trunc(float(c) (float(a) / 255.f))
// for c = r, g, b (divide and multiply correctly rounded, no sRGB decode), S_c the exact integer sum, mean_c = (float(S_c) / 255.f) / float(width height),
// means[t] = {r, g, b, 0}. A BC1 / BC3 / BC5 level is decoded texel by texel with the prepass's block decode (device/bc_decode.h: BC1 alpha 255, BC5 (R, G, 0,
// 255)); texels of a block beyond the level's width or height are not counted. Integer sums: the result does not depend on the order of execution. The entry of
// a texture no draw names, of an unusable entry (a size outside 1 .. 16384, a format code above 3, a compressed offset that is no multiple of the block's words)
// and of a level that does not lie inside `texels` is not written.
// Three launches: mark (a lane per draw sets used[albedoTexture]), reduce (grid {groups, textureCount}: 256 lanes stride over the level, 16-byte loads of four
// RGBA8 texels or one block per lane, 32-bit partial sums - a lane's is at most 4096 rounds of 16 texels of 255, below 2^24, a wave's 64 of those -, reduced across the wave with
// DPP and across the block through LDS, one 64-bit atomic add per block, round and channel), finish (a lane per texture: the three divisions).
#include <algorithm>

#include "../backend.h"
#include "../device/bc_decode.h"
#include "../device/depth_prepass_raster.h"
#include "../device/scene_sdf.h"

namespace plr {
namespace scenesdf {

using prepass::Draw;
using prepass::MainPassMatrices;
using prepass::Material;
using prepass::Texture;

struct InstanceParams {
    const MainPassMatrices* matrices;
    const InstanceEntry* table;
    const Draw* draws;
    const float* overrides;
    const Material* materials; // null: textureCount == 0
    const float* means;
    uint32_t* header;          // the instance buffer: 4 words, then 24 words per instance
    float* worldBBs;
    uint32_t instanceCount, drawCount, textureCount;
};

__global__ void __launch_bounds__(64) sdfInstanceUpdateKernel(InstanceParams p) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i == 0u) *(uint4*)p.header = make_uint4(p.instanceCount, 0u, 0u, 0u);
    if (i >= p.instanceCount) return;
    const InstanceEntry e = p.table[i];
    if (e.draw >= p.drawCount) return;
    const float* model = p.matrices[e.draw].model;
    float m[16];
    for (int k = 0; k < 16; k++) m[k] = model[k];
    Box local;
    for (int c = 0; c < 3; c++) { local.mn[c] = e.localMin[c]; local.mx[c] = e.localMax[c]; }
    const Box padded = paddedBox(local);
    const Box world = paddedBox(worldBoxOf(m, local));
    float localToWorld[16], worldToLocal[16];
    localToWorldOf(m, padded, localToWorld);
    inverseOf(localToWorld, worldToLocal);
    float albedo[3];
    const float* o = p.overrides + (size_t)e.draw * 3u;
    const uint32_t texture = p.textureCount ? p.materials[e.draw].albedoTexture : prepass::kNoTexture;
    if (!(o[0] != o[0])) { albedo[0] = o[0]; albedo[1] = o[1]; albedo[2] = o[2]; }
    else if (texture < p.textureCount) { albedo[0] = p.means[4u * texture]; albedo[1] = p.means[4u * texture + 1u]; albedo[2] = p.means[4u * texture + 2u]; }
    else meanOfWord(p.draws[e.draw].albedo, albedo);
    float4* out = (float4*)(p.header + 4u + (size_t)i * 24u);
    out[0] = make_float4(padded.mx[0] - padded.mn[0], padded.mx[1] - padded.mn[1], padded.mx[2] - padded.mn[2], __uint_as_float(e.sdfTextureIndex));
    out[1] = make_float4(albedo[0], albedo[1], albedo[2], 0.f);
    for (int c = 0; c < 4; c++) out[2 + c] = make_float4(worldToLocal[4 * c], worldToLocal[4 * c + 1], worldToLocal[4 * c + 2], worldToLocal[4 * c + 3]);
    float4* bb = (float4*)(p.worldBBs + (size_t)i * 8u);
    bb[0] = make_float4(world.mn[0], world.mn[1], world.mn[2], 0.f);
    bb[1] = make_float4(world.mx[0], world.mx[1], world.mx[2], 0.f);
}

static int launchSdfInstanceUpdate(const PassCtx& c) {
    if (c.push.size() != sizeof(InstancePushConstants)) return c.fail(-1, "sdfInstanceUpdate: push constants {instanceCount, drawCount, textureCount} missing");
    InstancePushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    const uint32_t blocks = divUp(std::max(pc.instanceCount, 1u), 64u);
    if (c.dispatch[0] != blocks || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "sdfInstanceUpdate: the dispatch is {ceil(max(instanceCount, 1) / 64), 1, 1}: a lane per instance");
    if (int rc = c.needSbuf(kMatricesBinding, (size_t)pc.drawCount * sizeof(MainPassMatrices), "sdfInstanceUpdate mainPassMatrices (binding 0: {model, mvp, mvpPrevious} per draw)")) return rc;
    if (int rc = c.needSbuf(kTableBinding, (size_t)pc.instanceCount * sizeof(InstanceEntry), "sdfInstanceUpdate instance table (binding 1: {draw, sdfTextureIndex, local min, local max})")) return rc;
    if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * sizeof(Draw), "sdfInstanceUpdate draws (binding 2)")) return rc;
    if (int rc = c.needSbuf(kOverrideBinding, (size_t)pc.drawCount * 12u, "sdfInstanceUpdate mean albedo overrides (binding 3: 3 floats per draw)")) return rc;
    if (int rc = c.needSbuf(kInstanceBinding, kInstanceHeaderBytes + (size_t)pc.instanceCount * kInstanceBytes, "sdfInstanceUpdate sdfInstances (binding 4: 16 + 96 instanceCount bytes)")) return rc;
    if (int rc = c.needSbuf(kWorldBBBinding, (size_t)pc.instanceCount * kWorldBBBytes, "sdfInstanceUpdate sdfWorldBBs (binding 5: 32 instanceCount bytes)")) return rc;
    if (pc.textureCount) {
        if (int rc = c.needSbuf(kMaterialBinding, (size_t)pc.drawCount * sizeof(Material), "sdfInstanceUpdate materials (binding 6: {albedoTexture, specularTexture} per draw)")) return rc;
        if (int rc = c.needSbuf(kMeanAlbedoBinding, (size_t)pc.textureCount * 16u, "sdfInstanceUpdate mean albedos (binding 7: float[4] per texture)")) return rc;
    }
    if (c.sbuf[kInstanceBinding].readOnly || c.sbuf[kWorldBBBinding].readOnly) return c.fail(-4, "sdfInstanceUpdate: an output buffer (binding 4 or 5) is bound read-only");
    for (int out : {kInstanceBinding, kWorldBBBinding})
        for (int in : {kMatricesBinding, kTableBinding, kDrawBinding, kOverrideBinding, kMaterialBinding, kMeanAlbedoBinding})
            if (c.hasSbuf(in) && c.sbuf[in].ptr == c.sbuf[out].ptr) return c.fail(-4, "sdfInstanceUpdate: an output buffer is also bound as an input (binding " + std::to_string(in) + ")");
    if (c.sbuf[kInstanceBinding].ptr == c.sbuf[kWorldBBBinding].ptr) return c.fail(-4, "sdfInstanceUpdate: sdfInstances and sdfWorldBBs are one buffer");
    InstanceParams p{};
    p.matrices = (const MainPassMatrices*)c.sbuf[kMatricesBinding].ptr; p.table = (const InstanceEntry*)c.sbuf[kTableBinding].ptr;
    p.draws = (const Draw*)c.sbuf[kDrawBinding].ptr; p.overrides = (const float*)c.sbuf[kOverrideBinding].ptr;
    p.materials = pc.textureCount ? (const Material*)c.sbuf[kMaterialBinding].ptr : nullptr;
    p.means = pc.textureCount ? (const float*)c.sbuf[kMeanAlbedoBinding].ptr : nullptr;
    p.header = (uint32_t*)c.sbuf[kInstanceBinding].ptr; p.worldBBs = (float*)c.sbuf[kWorldBBBinding].ptr;
    p.instanceCount = pc.instanceCount; p.drawCount = pc.drawCount; p.textureCount = pc.textureCount;
    sdfInstanceUpdateKernel<<<blocks, 64, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

// ---- "sceneMeanAlbedo.comp"
struct MeanParams {
    const Texture* textures;
    const uint32_t* texels;
    const uint32_t* formats; // null: every texture is RGBA8
    const Material* materials;
    unsigned long long* sums; // 4 per texture
    uint32_t* used;           // 1 per texture
    float* means;
    uint64_t wordCount;       // of `texels`
    uint32_t textureCount, drawCount;
};

// the level-0 description of texture t when the reduction can run over it
PLR_DI bool reducibleTexture(const MeanParams& p, uint32_t t, Texture* out, uint32_t* format) {
    const Texture tex = p.textures[t];
    const uint32_t f = p.formats ? p.formats[t] : prepass::kTextureFormatRgba8;
    if (tex.width < 1u || tex.height < 1u || tex.width > prepass::kMaxTextureSize || tex.height > prepass::kMaxTextureSize || f > prepass::kTextureFormatBc5) return false;
    if (f != prepass::kTextureFormatRgba8 && (tex.texelOffset & (f == prepass::kTextureFormatBc1 ? 1u : 3u)) != 0u) return false;
    const uint64_t words = f == prepass::kTextureFormatRgba8 ? (uint64_t)tex.width * tex.height
                                                             : (uint64_t)((tex.width + 3u) >> 2) * ((tex.height + 3u) >> 2) * (f == prepass::kTextureFormatBc1 ? 2u : 4u);
    if ((uint64_t)tex.texelOffset + words > p.wordCount) return false;
    *out = tex; *format = f;
    return true;
}

__global__ void __launch_bounds__(256) meanAlbedoMarkKernel(MeanParams p) {
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d >= p.drawCount) return;
    const uint32_t t = p.materials[d].albedoTexture;
    if (t < p.textureCount) atomicOr(&p.used[t], 1u);
}

// the sum of v over the wave, in every lane of row 0: DPP within the 16-lane rows, then the four row sums
PLR_DI uint32_t waveSum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // quad_perm [1, 0, 3, 2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // quad_perm [2, 3, 0, 1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false); // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

PLR_DI void addTexel(uint32_t word, uint32_t sum[3]) {
    const float alpha = (float)(word >> 24) / 255.f;
    for (int c = 0; c < 3; c++) sum[c] += albedoTerm((word >> (8 * c)) & 255u, alpha);
}

constexpr uint32_t kRoundsPerFlush = 4096; // a lane's partial: 4096 rounds x 16 texels (a block; RGBA8: 4) x 255 < 2^24; a wave's sum of 64 partials < 2^30

__global__ void __launch_bounds__(256) meanAlbedoReduceKernel(MeanParams p) {
    __shared__ uint32_t partial[4][3];
    const uint32_t t = blockIdx.y;
    if (p.used[t] == 0u) return;
    Texture tex;
    uint32_t format;
    if (!reducibleTexture(p, t, &tex, &format)) return;
    const uint32_t wave = threadIdx.x >> 6;
    // items: groups of four words at a 16-byte address (RGBA8), or blocks
    uint64_t first, count;
    if (format == prepass::kTextureFormatRgba8) {
        first = (uint64_t)tex.texelOffset >> 2;
        count = (((uint64_t)tex.texelOffset + (uint64_t)tex.width * tex.height + 3u) >> 2) - first;
    } else {
        first = 0u;
        count = (uint64_t)((tex.width + 3u) >> 2) * ((tex.height + 3u) >> 2);
    }
    const uint64_t begin = tex.texelOffset, end = begin + (uint64_t)tex.width * tex.height; // RGBA8: the level's words
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    const uint32_t blocksX = (tex.width + 3u) >> 2;
    for (uint64_t base = 0; base < count; base += stride * kRoundsPerFlush) { // (uniform over the block: the barriers below are reached by every lane)
        uint32_t sum[3] = {0u, 0u, 0u};
        for (uint32_t r = 0; r < kRoundsPerFlush; r++) {
            const uint64_t item = base + (uint64_t)r * stride + (uint64_t)blockIdx.x * 256u + threadIdx.x;
            if (item >= count) break;
            if (format == prepass::kTextureFormatRgba8) {
                const uint64_t w0 = (first + item) * 4u;
                if (w0 >= begin && w0 + 4u <= end) {
                    const uint4 v = *(const uint4*)(p.texels + w0);
                    addTexel(v.x, sum); addTexel(v.y, sum); addTexel(v.z, sum); addTexel(v.w, sum);
                } else {
                    for (uint64_t w = w0; w < w0 + 4u; w++)
                        if (w >= begin && w < end) addTexel(p.texels[w], sum);
                }
            } else {
                const uint32_t by = (uint32_t)(item / blocksX), bx = (uint32_t)(item - (uint64_t)by * blocksX);
                for (uint32_t k = 0; k < 16u; k++) {
                    const uint32_t x = 4u * bx + (k & 3u), y = 4u * by + (k >> 2);
                    if (x < tex.width && y < tex.height) addTexel(prepass::blockTexel<0>(p.texels, p.wordCount, tex.texelOffset, format, (int)tex.width, (int)x, (int)y), sum);
                }
            }
        }
        for (int c = 0; c < 3; c++) {
            const uint32_t s = waveSum(sum[c]);
            if ((threadIdx.x & 63u) == 0u) partial[wave][c] = s;
        }
        __syncthreads();
        if (threadIdx.x < 3u) {
            const unsigned long long s = (unsigned long long)partial[0][threadIdx.x] + partial[1][threadIdx.x] + partial[2][threadIdx.x] + partial[3][threadIdx.x];
            if (s) atomicAdd(&p.sums[4u * t + threadIdx.x], s);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) meanAlbedoFinishKernel(MeanParams p) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= p.textureCount || p.used[t] == 0u) return;
    Texture tex;
    uint32_t format;
    if (!reducibleTexture(p, t, &tex, &format)) return;
    const uint32_t texelCount = tex.width * tex.height;
    *(float4*)(p.means + 4u * (size_t)t) = make_float4(meanOfSum(p.sums[4u * t], texelCount), meanOfSum(p.sums[4u * t + 1u], texelCount), meanOfSum(p.sums[4u * t + 2u], texelCount), 0.f);
}

static int launchSceneMeanAlbedo(const PassCtx& c) {
    if (c.push.size() != sizeof(MeanPushConstants)) return c.fail(-1, "sceneMeanAlbedo: push constants {textureCount, drawCount, formats} missing");
    MeanPushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (c.dispatch[0] < 1u || c.dispatch[0] > 65535u || c.dispatch[1] != pc.textureCount || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "sceneMeanAlbedo: the dispatch is {groups per texture (1 .. 65535), textureCount, 1}");
    if (pc.textureCount == 0u || pc.textureCount > 65535u) return c.fail(-1, "sceneMeanAlbedo: textureCount is " + std::to_string(pc.textureCount) + ", it must be 1 .. 65535");
    if (int rc = c.needSbuf(kMeanTextureBinding, (size_t)pc.textureCount * sizeof(Texture), "sceneMeanAlbedo textures (binding 0: {texelOffset, width, height, mipCount})")) return rc;
    if (int rc = c.needSbuf(kMeanTexelBinding, 0, "sceneMeanAlbedo texels (binding 1)")) return rc;
    if (int rc = c.needSbuf(kMeanMaterialBinding, (size_t)pc.drawCount * sizeof(Material), "sceneMeanAlbedo materials (binding 2: {albedoTexture, specularTexture} per draw)")) return rc;
    if (int rc = c.needSbuf(kMeanScratchBinding, meanScratchBytes(pc.textureCount), "sceneMeanAlbedo scratch (binding 3: 36 textureCount bytes, rounded up to 16)")) return rc;
    if (int rc = c.needSbuf(kMeanOutBinding, (size_t)pc.textureCount * 16u, "sceneMeanAlbedo mean albedos (binding 4: float[4] per texture)")) return rc;
    if (pc.formats)
        if (int rc = c.needSbuf(kMeanFormatBinding, (size_t)pc.textureCount * 4u, "sceneMeanAlbedo texture formats (binding 5: one code per texture)")) return rc;
    if (c.sbuf[kMeanScratchBinding].readOnly || c.sbuf[kMeanOutBinding].readOnly) return c.fail(-4, "sceneMeanAlbedo: the scratch or the output buffer (binding 3 or 4) is bound read-only");
    for (int out : {kMeanScratchBinding, kMeanOutBinding})
        for (int in : {kMeanTextureBinding, kMeanTexelBinding, kMeanMaterialBinding, kMeanFormatBinding})
            if (c.hasSbuf(in) && c.sbuf[in].ptr == c.sbuf[out].ptr) return c.fail(-4, "sceneMeanAlbedo: an output buffer is also bound as an input (binding " + std::to_string(in) + ")");
    if (c.sbuf[kMeanScratchBinding].ptr == c.sbuf[kMeanOutBinding].ptr) return c.fail(-4, "sceneMeanAlbedo: the scratch and the output are one buffer");
    if (((uintptr_t)c.sbuf[kMeanTexelBinding].ptr & 15u) != 0u) return c.fail(-4, "sceneMeanAlbedo: the texel store (binding 1) is not at a 16-byte address");
    MeanParams p{};
    p.textures = (const Texture*)c.sbuf[kMeanTextureBinding].ptr; p.texels = (const uint32_t*)c.sbuf[kMeanTexelBinding].ptr;
    p.formats = pc.formats ? (const uint32_t*)c.sbuf[kMeanFormatBinding].ptr : nullptr;
    p.materials = (const Material*)c.sbuf[kMeanMaterialBinding].ptr;
    uint8_t* scratch = (uint8_t*)c.sbuf[kMeanScratchBinding].ptr;
    p.sums = (unsigned long long*)scratch; p.used = (uint32_t*)(scratch + (size_t)pc.textureCount * 32u);
    p.means = (float*)c.sbuf[kMeanOutBinding].ptr;
    p.wordCount = c.sbuf[kMeanTexelBinding].size / 4u;
    p.textureCount = pc.textureCount; p.drawCount = pc.drawCount;
    if (hipMemsetAsync(scratch, 0, meanScratchBytes(pc.textureCount), c.stream) != hipSuccess) return c.fail(-2, "sceneMeanAlbedo: clearing the scratch failed");
    if (pc.drawCount) {
        meanAlbedoMarkKernel<<<divUp(pc.drawCount, 256u), 256, 0, c.stream>>>(p);
        PLR_CHECK_LAUNCH(c);
        c.splitTiming("mark");
    }
    meanAlbedoReduceKernel<<<dim3(c.dispatch[0], pc.textureCount), 256, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    meanAlbedoFinishKernel<<<divUp(pc.textureCount, 64u), 64, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace scenesdf
static int sdf_instance_update_launch(const PassCtx& c) { return scenesdf::launchSdfInstanceUpdate(c); }
static int sdf_instance_update_launch_fast(const PassCtx& c) { return scenesdf::launchSdfInstanceUpdate(c); }
static int scene_mean_albedo_launch(const PassCtx& c) { return scenesdf::launchSceneMeanAlbedo(c); }
static int scene_mean_albedo_launch_fast(const PassCtx& c) { return scenesdf::launchSceneMeanAlbedo(c); }
PLR_REGISTER_SHADER("sdfInstanceUpdate.comp", sdf_instance_update_launch);
PLR_REGISTER_SHADER_FAST("sdfInstanceUpdate.comp", sdf_instance_update_launch_fast);
PLR_REGISTER_SHADER("sceneMeanAlbedo.comp", scene_mean_albedo_launch);
PLR_REGISTER_SHADER_FAST("sceneMeanAlbedo.comp", scene_mean_albedo_launch_fast);
} // namespace plr
