// "sdfInstanceUpdate.comp" and "sceneMeanAlbedo.comp": what the launchers (kernels/scene_sdf.hip), the frame pipeline (frontend/frame_pipeline.cpp) and the host
// validation (frontend/scene_sdf_packing.cpp) share - the pass records' bindings, the buffer layouts, and THE INSTANCE CONTRACT's arithmetic as functions that
// compile for the host and the device alike (DESIGN.md "SDF instances from the scene"): the kernel and the host's determinant test evaluate one text.
// Every translation unit that includes this is compiled without floating-point contraction (-ffp-contract=off).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLR_SDF_HD __host__ __device__ inline
#else
#define PLR_SDF_HD inline
#endif

namespace plr {
namespace scenesdf {

// ---- "sdfInstanceUpdate.comp": dispatch {ceil(max(instanceCount, 1) / 64), 1, 1}, a lane per instance
constexpr int kMatricesBinding = 0;   // MainPassMatrices per draw (prepass::MainPassMatrices, 192 bytes); `model` alone is read
constexpr int kTableBinding = 1;      // InstanceEntry per instance
constexpr int kDrawBinding = 2;       // prepass::Draw per draw (24 bytes); `albedo` alone is read
constexpr int kOverrideBinding = 3;   // 3 floats per draw: the mean albedo, or a NaN red = derive
constexpr int kInstanceBinding = 4;   // out: {n, 0, 0, 0} and n SDFInstance records of 96 bytes
constexpr int kWorldBBBinding = 5;    // out: n {vec3 min; float 0; vec3 max; float 0}
constexpr int kMaterialBinding = 6;   // textureCount > 0: prepass::Material per draw; albedoTexture alone is read
constexpr int kMeanAlbedoBinding = 7; // textureCount > 0: float[4] per texture, what "sceneMeanAlbedo.comp" wrote
struct InstancePushConstants { uint32_t instanceCount, drawCount, textureCount; };
struct InstanceEntry { uint32_t draw, sdfTextureIndex; float localMin[3], localMax[3]; };
static_assert(sizeof(InstanceEntry) == 32, "instance table layout");
constexpr uint32_t kInstanceBytes = 96, kInstanceHeaderBytes = 16, kWorldBBBytes = 32;

// ---- "sceneMeanAlbedo.comp": dispatch {groups per texture >= 1, textureCount, 1}; the result does not depend on the first number
constexpr int kMeanTextureBinding = 0;  // prepass::Texture per texture
constexpr int kMeanTexelBinding = 1;    // the texel store
constexpr int kMeanMaterialBinding = 2; // prepass::Material per draw
constexpr int kMeanScratchBinding = 3;  // meanScratchBytes(textureCount): 4 uint64 sums per texture, then one `used` word per texture
constexpr int kMeanOutBinding = 4;      // out: float[4] per texture {r, g, b, 0}; the entry of a texture no draw names as albedo is not written
constexpr int kMeanFormatBinding = 5;   // formats != 0: one prepass::kTextureFormat* code per texture
struct MeanPushConstants { uint32_t textureCount, drawCount, formats; };
constexpr size_t meanScratchBytes(uint32_t textureCount) { return ((size_t)textureCount * 36u + 15u) & ~(size_t)15u; }

// ---- THE INSTANCE CONTRACT. fp32 IEEE operations in the order written, no contraction; fp64 where a double appears.
// min / max are the comparisons of plr_sdf_padded_bounds (kernels/sdf_bake.hip minH / maxH): a NaN on the right is dropped
PLR_SDF_HD float minOf(float x, float y) { return (y < x) ? y : x; }
PLR_SDF_HD float maxOf(float x, float y) { return (x < y) ? y : x; }

struct Box { float mn[3], mx[3]; };
// padSDFBoundingBox as plr_sdf_padded_bounds evaluates it, operation for operation
PLR_SDF_HD Box paddedBox(const Box& b) {
    Box p;
    for (int c = 0; c < 3; c++) {
        const float pad = maxOf(0.075f * (b.mx[c] - b.mn[c]), 0.5f);
        p.mn[c] = b.mn[c] - pad;
        p.mx[c] = b.mx[c] + pad;
    }
    return p;
}
// row i of model * (x, y, z, 1): the prepass's clip rule, summed left to right
PLR_SDF_HD float transformRow(const float* m, int i, float x, float y, float z) { return ((m[0 * 4 + i] * x + m[1 * 4 + i] * y) + m[2 * 4 + i] * z) + m[3 * 4 + i]; }
// the component min / max of the eight transformed corners of the UNPADDED local box, corner k taking max on the axes whose bit of k is set, k ascending
PLR_SDF_HD Box worldBoxOf(const float* model, const Box& local) {
    Box w;
    for (int k = 0; k < 8; k++) {
        const float x = (k & 1) ? local.mx[0] : local.mn[0], y = (k & 2) ? local.mx[1] : local.mn[1], z = (k & 4) ? local.mx[2] : local.mn[2];
        for (int i = 0; i < 3; i++) {
            const float v = transformRow(model, i, x, y, z);
            w.mn[i] = k == 0 ? v : minOf(w.mn[i], v);
            w.mx[i] = k == 0 ? v : maxOf(w.mx[i], v);
        }
    }
    return w;
}
// model * translate(bbOffset), glm column-major: the first three columns are model's, the fourth is the row rule at bbOffset (all four rows)
PLR_SDF_HD void localToWorldOf(const float* model, const Box& padded, float* out16) {
    const float ox = (padded.mn[0] + padded.mx[0]) * 0.5f, oy = (padded.mn[1] + padded.mx[1]) * 0.5f, oz = (padded.mn[2] + padded.mx[2]) * 0.5f;
    for (int e = 0; e < 12; e++) out16[e] = model[e];
    for (int i = 0; i < 4; i++) out16[12 + i] = transformRow(model, i, ox, oy, oz);
}
// the inverse as adjugate over determinant in fp64. a[i][j] = (double)m[4 i + j]; the twelve 2 x 2 sub-determinants first, each `p q - r s`:
//   s0 .. s5 from rows 0 and 1 (column pairs 01 02 03 12 13 23), c0 .. c5 from rows 2 and 3 (the same pairs);
//   det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0;
// every adjugate element is three products combined left to right as written in inverseOf; one division per element, one rounding to fp32.
// (The flat array is glm's column-major matrix read as if it were row-major, i.e. its transpose; the inverse of the transpose is the transpose of the inverse,
// so the result, written back the same way, is the column-major inverse.)
struct SubDeterminants { double s[6], c[6]; };
PLR_SDF_HD SubDeterminants subDeterminantsOf(const float* m) {
    double a[16];
    for (int e = 0; e < 16; e++) a[e] = (double)m[e];
    SubDeterminants d;
    d.s[0] = a[0] * a[5] - a[4] * a[1];
    d.s[1] = a[0] * a[6] - a[4] * a[2];
    d.s[2] = a[0] * a[7] - a[4] * a[3];
    d.s[3] = a[1] * a[6] - a[5] * a[2];
    d.s[4] = a[1] * a[7] - a[5] * a[3];
    d.s[5] = a[2] * a[7] - a[6] * a[3];
    d.c[0] = a[8] * a[13] - a[12] * a[9];
    d.c[1] = a[8] * a[14] - a[12] * a[10];
    d.c[2] = a[8] * a[15] - a[12] * a[11];
    d.c[3] = a[9] * a[14] - a[13] * a[10];
    d.c[4] = a[9] * a[15] - a[13] * a[11];
    d.c[5] = a[10] * a[15] - a[14] * a[11];
    return d;
}
PLR_SDF_HD double determinantOf(const SubDeterminants& d) {
    return ((((d.s[0] * d.c[5] - d.s[1] * d.c[4]) + d.s[2] * d.c[3]) + d.s[3] * d.c[2]) - d.s[4] * d.c[1]) + d.s[5] * d.c[0];
}
PLR_SDF_HD void inverseOf(const float* m, float* out16) {
    double a[16];
    for (int e = 0; e < 16; e++) a[e] = (double)m[e];
    const SubDeterminants d = subDeterminantsOf(m);
    const double* s = d.s;
    const double* c = d.c;
    const double det = determinantOf(d);
    double b[16];
    b[0] = (a[5] * c[5] - a[6] * c[4]) + a[7] * c[3];
    b[1] = (a[2] * c[4] - a[1] * c[5]) - a[3] * c[3];
    b[2] = (a[13] * s[5] - a[14] * s[4]) + a[15] * s[3];
    b[3] = (a[10] * s[4] - a[9] * s[5]) - a[11] * s[3];
    b[4] = (a[6] * c[2] - a[4] * c[5]) - a[7] * c[1];
    b[5] = (a[0] * c[5] - a[2] * c[2]) + a[3] * c[1];
    b[6] = (a[14] * s[2] - a[12] * s[5]) - a[15] * s[1];
    b[7] = (a[8] * s[5] - a[10] * s[2]) + a[11] * s[1];
    b[8] = (a[4] * c[4] - a[5] * c[2]) + a[7] * c[0];
    b[9] = (a[1] * c[2] - a[0] * c[4]) - a[3] * c[0];
    b[10] = (a[12] * s[4] - a[13] * s[2]) + a[15] * s[0];
    b[11] = (a[9] * s[2] - a[8] * s[4]) - a[11] * s[0];
    b[12] = (a[5] * c[1] - a[4] * c[3]) - a[6] * c[0];
    b[13] = (a[0] * c[3] - a[1] * c[1]) + a[2] * c[0];
    b[14] = (a[13] * s[1] - a[12] * s[3]) - a[14] * s[0];
    b[15] = (a[8] * s[3] - a[9] * s[1]) + a[10] * s[0];
    for (int e = 0; e < 16; e++) out16[e] = (float)(b[e] / det);
}
// what plrf_set_scene_sdf and plrf_set_scene_mesh_transforms test: the determinant the kernel will divide by for this draw of a mesh with this local box
PLR_SDF_HD double instanceDeterminant(const float* model, const Box& local) {
    float m[16];
    localToWorldOf(model, paddedBox(local), m);
    return determinantOf(subDeterminantsOf(m));
}

// ---- THE MEAN ALBEDO CONTRACT (computeMeanAlbedo, ModelImport.cpp:78-112, its quirks kept: no sRGB decode, the alpha-weighted term truncated per texel).
// term_c = (uint)trunc(float(c) * (float(a) / 255.f)), divide and multiply correctly rounded; S_c the exact integer sum; mean_c = (float(S_c) / 255.f) / float(texelCount)
PLR_SDF_HD uint32_t albedoTerm(uint32_t c, float alphaOver255) { return (uint32_t)((float)c * alphaOver255); }
PLR_SDF_HD float meanOfSum(uint64_t sum, uint32_t texelCount) { return ((float)sum / 255.f) / (float)texelCount; }
// a draw without an albedo texture: the rule on its constant albedo word as a one-texel image
PLR_SDF_HD void meanOfWord(uint32_t word, float out[3]) {
    const float alpha = (float)(word >> 24) / 255.f;
    for (int c = 0; c < 3; c++) out[c] = meanOfSum(albedoTerm((word >> (8 * c)) & 255u, alpha), 1u);
}

} // namespace scenesdf
} // namespace plr
