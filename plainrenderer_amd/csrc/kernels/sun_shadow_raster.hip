// "sunShadowRaster.comp": the sun shadow cascades as a compute pass - RenderFrontend::renderSunShadowCascades (RenderFrontend.cpp:354, 760-774; pass description
// :1565-1590; sunShadow.vert / sunShadow.frag): depth only, orthographic, one Depth16 target per execution, opaque casters and alpha-tested cutouts. One kernel
// family serves both math modes: every decision is an integer one and the float part is a dozen IEEE operations per fragment (and, for a cutout's fragment, fp64
// operations in a fixed order).
// PLR_BUILD_FLAGS: -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
//
// THE RASTERISATION CONTRACT (DESIGN.md "Sun shadow cascades as a compute pass"; tests/shadow_raster_reference.py implements it independently and every texel
// and counter must agree bit for bit). fp32 IEEE, no contraction. Cascade c, L = sunShadowInfo.lightMatrices[c], a draw with model matrix T, both column-major:
//   M = L * T first (GLSL's A * B * v is (A * B) * v, sunShadow.vert:29), each element a0 b0 + a1 b1 + a2 b2 + a3 b3 summed left to right
//   clip = M * (p, 1), each component m[0][i] x + m[1][i] y + m[2][i] z + m[3][i] summed left to right; w is not divided by: T is affine (the host boundary
//     refuses anything else) and L orthographic (lightMatrix.comp:57-138)
//   viewport 0 .. res on both axes, no Y flip, depth 0 .. 1 (VulkanCommandRecording.cpp:44-48): xf = (clip.x * 0.5 + 0.5) * res, yf likewise, z = clip.z
//   X = rint(xf * 256), Y = rint(yf * 256), round to nearest even, int32: eight sub-pixel bits
//   guard band: a triangle with a non-finite xf, yf or z, or |xf| or |yf| >= 2^20 pixels, is not drawn and counted as a reject (no clipping). Inside the band
//     every product below fits int64.
//   outside a buffer: a triangle counts as submitted and as a reject, and draws nothing, when its three index slots are not all inside `indices`, when a
//     vertex (index + vertexOffset, in 64 bits) is not inside `positions`, or when its draw's transformIndex is not inside `transforms`. A draw submits
//     indexCount / 3 triangles (rounded down), whatever becomes of them.
//   A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0); Vulkan's area is -A / 2 and the front face counter-clockwise (VulkanPipeline.cpp:61), so A < 0 faces front;
//     the pass culls FRONT faces (RenderFrontend.cpp:1576): only A > 0 is drawn
//   pixel box: columns (Xmin + 127) >> 8 .. (Xmax - 128) >> 8 (the pixel centres 256 i + 128 inside [Xmin, Xmax]) clipped to 0 .. res - 1, rows likewise; a
//     triangle with an empty box is dropped, every other one counts as drawn
//   edges 0 -> 1, 1 -> 2, 2 -> 0; for a -> b and the pixel centre P = (256 i + 128, 256 j + 128): E = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa), int64
//   a pixel is covered when every E > 0, or E == 0 on a top (dy == 0 && dx > 0) or left (dy < 0) edge, d = b - a: the top-left rule in a y-down frame
//   l1 = float(E_20) / float(A), l2 = float(E_01) / float(A) (int64 -> fp32 to nearest even, IEEE divide); zf = (z0 + l1 (z1 - z0)) + l2 (z2 - z0)
//   depth clamp on (:1578): zf to [0, 1] as fmin(fmax(zf, 0), 1) with IEEE maxNum / minNum semantics (of a NaN and a number, the number): a NaN zf - finite
//     vertex depths whose difference overflows, times a zero weight - stores code 0, +inf stores 65535; code = rint(zf * 65535) as uint16
//   cleared to 0, depth test GreaterEqual (RenderPass.cpp:105, :1574): a texel is the MAXIMUM code of its fragments, 0 without any. Every texel of the map is
//     written by every execution: the clear is part of the pass.
//   sunShadow.frag's alpha test (:17-21) is the clause below, of an execution with textureCount > 0; without it casters are opaque.
//
// THE CUTOUT CONTRACT (DESIGN.md "Alpha-tested cutout casters in the sun shadow raster"; tests/shadow_alpha_reference.py implements it independently, bit for
// bit). Everything above stands; one clause is added. fp64 IEEE without contraction where fp64 is named.
//   texture store: the prepass's (DESIGN.md "The sampling contract", Texture store): `texels` RGBA8 words, R in the low byte, levels back to back and unpadded;
//     `textures` {texelOffset, width, height, mipCount}; an entry is usable when 1 <= width, height <= 16384 and 1 <= mipCount <= floor(log2(max(width,
//     height))) + 1; a texel whose 64-bit address is outside `texels` reads 0
//   uvs: 2 floats per vertex, indexed like positions (index + vertexOffset); a vertex outside `uvs` has (0, 0)
//   casterMaterials: {albedoTexture, cutoff} per draw; c = min(cutoff, 256). c = 0: the draw is opaque and never sampled. A draw whose albedoTexture is
//     0xffffffff, is >= textureCount or names an unusable entry has the alpha code 255 everywhere (shadow draws have no constant albedo word): opaque for
//     c <= 255, nothing for c = 256
//   UV of a fragment (no perspective: the pass is affine): with l1, l2 exactly the fp32 weights of the depth clause, u = (u0 + (double)l1 (u1 - u0)) +
//     (double)l2 (u2 - u0) in fp64, the differences taken in fp64 from the widened floats; v likewise. If u or v is not finite, or |.| >= 2^20, both are 0 for
//     the taps
//   level: one per (triangle, texture). With the walk's integer steps sx20 = -256 (Y0 - Y2), sx01 = -256 (Y1 - Y0), sy20 = 256 (X0 - X2), sy01 = 256 (X1 - X0)
//     and A, each converted to fp64 (nearest even): dudx = ((double)sx20 / (double)A) (u1 - u0) + ((double)sx01 / (double)A) (u2 - u0), dvdx with v, dudy and
//     dvdy with sy. ax = (dudx W_0, dvdx H_0), ay likewise, rx = ax.x^2 + ax.y^2, ry likewise, rho2 = rx > ry ? rx : ry; r = (float)rho2; lod = 0.5f
//     det_log2f(r) - the bias is 0: sunShadow.frag:18 calls texture() without g_mipBias -; !(lod > 0) -> 0; lod > mipCount - 1 -> that; q = (int)floorf(lod 256
//     + 0.5f), L0 = q >> 8, fw = q & 255, L1 = min(L0 + 1, mipCount - 1). The gradient is taken from the raw UVs, before the validity rule
//   alpha of a fragment: bits 24 - 31 of what the sampling contract's Taps clause yields for (u, v) at L0, L1, fw: per level Tu = (int64)floor((u W - 0.5) 256 +
//     0.5) in fp64, x0 = Tu >> 8, fx = Tu & 255, x1 = x0 + 1, both wrapped to [0, W) by a non-negative modulo, y likewise; S_l = (256 - fx)(256 - fy) a00 +
//     fx (256 - fy) a10 + (256 - fx) fy a01 + fx fy a11; S = (256 - fw) S_L0 + fw S_L1; alpha = (S + 2^23 - 1 + ((S >> 24) & 1)) >> 24
//   visibility: a texel is the maximum code over its fragments that pass coverage AND alpha >= c, 0 without any: still an order-independent maximum. submitted,
//     drawn and guardBandRejects do not depend on alpha, and there is no counter of discarded fragments: a fragment whose code is not above its cell's
//     current value need not be sampled
//   deviations from the reference: isotropic trilinear filtering for g_sampler_anisotropicRepeat; l is the depth's fp32 weight, not an exact plane
//
// THE FORMAT CLAUSE (DESIGN.md "Block-compressed cutout textures in the sun shadow raster"; tests/shadow_bc_reference.py implements it independently, bit for bit),
// of an execution with textureCount > 0 and textureFormats = 1. The cutout contract stands word for word except its texture store clause, which becomes the
// prepass's format-aware store (DESIGN.md "Block-compressed textures in the depth prepass"):
//   texture store: buffer `textureFormats` holds one code per texture, kTextureFormatRgba8 / Bc1 / Bc3 / Bc5 = 0 .. 3; `texels` holds uint32 words and an entry's
//     texelOffset counts words. A compressed entry's level l is ceil(W_l / 4) x ceil(H_l / 4) blocks (BC1: 2 words, BC3 and BC5: 4), row-major, levels back to
//     back, and its offset must be a multiple of its block's words. An entry is usable by the cutout contract's rule and: a code above BC5, or a misaligned
//     offset, makes it unusable (alpha 255 everywhere, as for a draw without a texture). A block that does not lie wholly inside `texels` reads 0; an RGBA8
//     entry's texel outside `texels` reads 0, as before
//   alpha of a texel: bits 24 - 31 of what the block decode contract (device/bc_decode.h) yields for it - BC3: its block's alpha block, {a0, a1, 16 indices of 3
//     bits}: index 0 -> a0, 1 -> a1, a0 > a1: ((8 - k) a0 + (k - 1) a1 + 3) / 7, else 6 -> 0, 7 -> 255, ((6 - k) a0 + (k - 1) a1 + 2) / 5; BC1 and BC5: 255
//   everything downstream is unchanged: the level per triangle from the texture's texel dimensions, bias 0, 8 sub-texel bits, repeat wrap,
//     S = (256 - fw) S_L0 + fw S_L1, round half even, alpha >= c, the order-independent maximum, the counters
//   the property: an execution with compressed entries equals, texel for texel and counter for counter, the same execution whose store holds
//     plr_decode_bc_to_rgba8 of the same levels
//
// Two kernels. SET-UP: a lane per triangle finds its draw, transforms, snaps, culls and boxes; survivors are appended through a cursor (one atomic per block) to a dense
// array of 4-byte tile rectangles and an array of set-up records (order free: the result is a maximum). TILES: a 256-thread block per 64 x 64 tile keeps the tile as
// 4096 words of LDS; each wave scans the rectangles and walks those that touch its tile; LDS atomic max; the block then stores its tile as Depth16 rows. Every tile
// scans every rectangle: no bins in this version. The draw lookup and the record are device/raster_setup.h's, the scan, the walk and a fragment's coverage and
// depth device/raster_tile_walk.h's, both shared with "depthPrepassRaster.comp"; this file holds the transform, the block's append, what becomes of a fragment
// (clamp, encode, alpha test, maximum), the tile's store and the launcher. Both kernels are templates over a three-way mode - kAlphaUntested, kAlphaRgba8,
// kAlphaFormats - picked by textureCount and textureFormats; the untested instantiations hold none of the cutout code and the RGBA8-tested ones none of the
// format code. The format-aware set-up decides per record: a BC1 or BC5 texture has alpha 255 everywhere and its record is stored like one without a usable
// texture; an RGBA8 or BC3 record reaches the fragment hook, bit 25 of its test word telling them apart, and a BC3 tap loads its alpha block alone. The tested set-up stores everything that depends on the triangle alone (cutoff, level sizes, first texel,
// fw, the three UVs) behind the set-up record (128 bytes per record instead of 80); only u, v and the taps are per fragment.
#include <algorithm>
#include <type_traits>

#include "../backend.h"
#include "../device/bc_decode.h"
#include "../device/detmath.h"
#include "../device/raster_setup.h"
#include "../device/raster_tile_walk.h"
#include "../device/sun_shadow_raster.h"

namespace plr {
namespace sunraster {

struct SetupParams {
    const ShadowCascadeInfo* info; const float* transforms; const float* positions; const uint32_t* indices; const Draw* draws;
    ScratchHeader* header; uint32_t* rects; SetupRecord* records;
    uint32_t cascade, drawCount, triangleCount, capacity, transformCount, vertexCount, indexCount;
    int32_t res;
};
// a tested execution's set-up: `s.records` is null, the 128-byte records go to `records`
struct CutoutSetupParams {
    SetupParams s;
    const float* uvs; const CasterMaterial* materials; const Texture* textures; CutoutRecord* records;
    uint64_t uvVertexCount;
    uint32_t textureCount;
};
// a format-aware execution's set-up: the same, and one format code per texture
struct FormatSetupParams {
    CutoutSetupParams c;
    const uint32_t* formats;
};
template <int kMode> using SetupArgs = std::conditional_t<kMode == kAlphaFormats, FormatSetupParams, std::conditional_t<kMode == kAlphaRgba8, CutoutSetupParams, SetupParams>>;
PLR_DI const SetupParams& plainParams(const SetupParams& a) { return a; }
PLR_DI const SetupParams& plainParams(const CutoutSetupParams& a) { return a.s; }
PLR_DI const SetupParams& plainParams(const FormatSetupParams& a) { return a.c.s; }
PLR_DI const CutoutSetupParams& cutoutParams(const CutoutSetupParams& a) { return a; }
PLR_DI const CutoutSetupParams& cutoutParams(const FormatSetupParams& a) { return a.c; }
PLR_DI SetupRecord& setupOf(SetupRecord& r) { return r; }
PLR_DI SetupRecord& setupOf(CutoutRecord& r) { return r.s; }

// the table entry `index` names when it is usable: inside the table, 1 <= width, height <= 16384, 1 <= mipCount <= floor(log2(max(width, height))) + 1
PLR_DI bool usableTexture(const Texture* textures, uint32_t textureCount, uint32_t index, Texture* out) {
    if (index == kNoTexture || index >= textureCount) return false;
    const Texture t = textures[index];
    if (t.width < 1u || t.height < 1u || t.width > kMaxTextureSize || t.height > kMaxTextureSize) return false;
    if (t.mipCount < 1u || t.mipCount > 32u - (uint32_t)__clz(max(t.width, t.height))) return false;
    *out = t;
    return true;
}

// the uint32 words of a w x h level: texels, or the 16-byte blocks of a BC3 level
PLR_DI uint64_t levelWords(bool bc3, uint32_t w, uint32_t h) {
    return bc3 ? (uint64_t)((w + 3u) >> 2) * (uint64_t)((h + 3u) >> 2) * 4u : (uint64_t)w * (uint64_t)h;
}

// what the alpha of a fragment of this triangle needs beyond its weights (the cutout contract: material, UVs, level): once per record. v: the three vertices
// Params: CutoutSetupParams, or FormatSetupParams (the format clause: the entry's format code decides whether it is usable, constant or sampled)
template <class Params>
PLR_DI void cutoutOfTriangle(const Params& args, uint32_t draw, const uint64_t v[3], CutoutRecord& r) {
    constexpr bool kFormats = std::is_same_v<Params, FormatSetupParams>;
    const CutoutSetupParams& p = cutoutParams(args);
    r.test = kAlphaCutoffOpaque;
    r.size0 = r.size1 = r.base0Low = r.base0High = r.pad = 0u;
    r.u0 = r.v0 = r.u1 = r.v1 = r.u2 = r.v2 = 0.f;
    const CasterMaterial m = p.materials[draw]; // (draw < drawCount, and the launcher checked drawCount entries)
    const uint32_t c = min(m.cutoff, kAlphaCutoffDiscardAll);
    if (c == kAlphaCutoffOpaque) return;
    if (c == kAlphaCutoffDiscardAll) { r.test = kAlphaCutoffDiscardAll; return; } // no alpha code reaches 256, sampled or constant
    Texture tex;
    if (!usableTexture(p.textures, p.textureCount, m.albedoTexture, &tex)) return; // alpha 255 everywhere: opaque for c <= 255
    bool bc3 = false;
    if constexpr (kFormats) {
        const uint32_t format = args.formats[m.albedoTexture]; // (usable: the index is inside the table, and the launcher checked textureCount entries)
        if (format > kTextureFormatBc5) return;                // unusable by the prepass's rule
        if (format != kTextureFormatRgba8 && (tex.texelOffset & (format == kTextureFormatBc1 ? 1u : 3u)) != 0u) return; // a misaligned offset: unusable too
        if (format == kTextureFormatBc1 || format == kTextureFormatBc5) return; // alpha 255 everywhere: stored like a record without a usable texture
        bc3 = format == kTextureFormatBc3;
    }
    float uv[6];
    for (int k = 0; k < 3; k++) { // a vertex outside `uvs` has (0, 0)
        const bool inside = v[k] < p.uvVertexCount;
        uv[2 * k] = inside ? p.uvs[v[k] * 2u] : 0.f;
        uv[2 * k + 1] = inside ? p.uvs[v[k] * 2u + 1u] : 0.f;
    }
    const SetupRecord& s = r.s;
    const double A = (double)s.area;
    const double sx20 = (double)(-256ll * (int64_t)(s.y0 - s.y2)), sx01 = (double)(-256ll * (int64_t)(s.y1 - s.y0));
    const double sy20 = (double)(256ll * (int64_t)(s.x0 - s.x2)), sy01 = (double)(256ll * (int64_t)(s.x1 - s.x0));
    const double du1 = (double)uv[2] - (double)uv[0], du2 = (double)uv[4] - (double)uv[0];
    const double dv1 = (double)uv[3] - (double)uv[1], dv2 = (double)uv[5] - (double)uv[1];
    const double dudx = (sx20 / A) * du1 + (sx01 / A) * du2, dvdx = (sx20 / A) * dv1 + (sx01 / A) * dv2;
    const double dudy = (sy20 / A) * du1 + (sy01 / A) * du2, dvdy = (sy20 / A) * dv1 + (sy01 / A) * dv2;
    const double w0 = (double)tex.width, h0 = (double)tex.height;
    const double axx = dudx * w0, axy = dvdx * h0, ayx = dudy * w0, ayy = dvdy * h0;
    const double rx = axx * axx + axy * axy, ry = ayx * ayx + ayy * ayy;
    const double rho2 = rx > ry ? rx : ry;
    float lod = 0.5f * det_log2f((float)rho2); // bias 0
    if (!(lod > 0.f)) lod = 0.f;
    const float top = (float)(tex.mipCount - 1u);
    if (lod > top) lod = top;
    const int q = (int)__builtin_floorf(lod * 256.f + 0.5f);
    const int L0 = q >> 8, L1 = min(L0 + 1, (int)tex.mipCount - 1);
    uint64_t base = tex.texelOffset;
    for (int l = 0; l < L0; l++) {
        if constexpr (kFormats) base += levelWords(bc3, max(1u, tex.width >> l), max(1u, tex.height >> l));
        else base += (uint64_t)max(1u, tex.width >> l) * (uint64_t)max(1u, tex.height >> l);
    }
    r.test = c | ((uint32_t)(q & 255) << 16) | (L1 != L0 ? 1u << 24 : 0u) | (bc3 ? 1u << 25 : 0u);
    r.size0 = max(1u, tex.width >> L0) | (max(1u, tex.height >> L0) << 16); // (a level is at most 16384 wide and high: 15 bits)
    r.size1 = max(1u, tex.width >> L1) | (max(1u, tex.height >> L1) << 16);
    r.base0Low = (uint32_t)base; r.base0High = (uint32_t)(base >> 32);
    r.u0 = uv[0]; r.v0 = uv[1]; r.u1 = uv[2]; r.v1 = uv[3]; r.u2 = uv[4]; r.v2 = uv[5];
}

template <int kMode>
__global__ __launch_bounds__(256) void sunShadowSetupKernel(SetupArgs<kMode> args) {
    constexpr bool kAlphaTest = kMode != kAlphaUntested;
    const SetupParams& p = plainParams(args);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const rastercov::TriangleSlot found = rastercov::drawOfTriangle(p.draws, p.drawCount, p.triangleCount, t);
    Draw draw{};
    if (found.found) draw = p.draws[found.draw];
    bool reject = false, survivor = false;
    std::conditional_t<kAlphaTest, CutoutRecord, SetupRecord> rec{};
    uint32_t rect = 0;
    if (found.found) {
        const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)found.local * 3u;
        bool inBuffers = at + 3u <= (uint64_t)p.indexCount && draw.transformIndex < p.transformCount;
        uint64_t v[3] = {0, 0, 0};
        if (inBuffers)
            for (int k = 0; k < 3; k++) {
                v[k] = (uint64_t)p.indices[at + k] + (uint64_t)draw.vertexOffset;
                inBuffers = inBuffers && v[k] < (uint64_t)p.vertexCount;
            }
        if (!inBuffers) reject = true;
        else {
            const float* L = p.info->lightMatrices[p.cascade];
            const float* T = p.transforms + (size_t)draw.transformIndex * 16u;
            float M[12]; // rows 0 .. 2 of the four columns: M[c * 3 + r]
            for (int c = 0; c < 4; c++)
                for (int r = 0; r < 3; r++) M[c * 3 + r] = ((L[0 * 4 + r] * T[c * 4 + 0] + L[1 * 4 + r] * T[c * 4 + 1]) + L[2 * 4 + r] * T[c * 4 + 2]) + L[3 * 4 + r] * T[c * 4 + 3];
            const float resf = (float)p.res;
            int32_t X[3], Y[3];
            float z[3];
            bool inside = true;
            for (int k = 0; k < 3; k++) {
                const float* q = p.positions + v[k] * 3u;
                const float x = q[0], y = q[1], zz = q[2];
                const float cx = ((M[0] * x + M[3] * y) + M[6] * zz) + M[9];
                const float cy = ((M[1] * x + M[4] * y) + M[7] * zz) + M[10];
                const float cz = ((M[2] * x + M[5] * y) + M[8] * zz) + M[11];
                const float xf = (cx * 0.5f + 0.5f) * resf, yf = (cy * 0.5f + 0.5f) * resf;
                // (a NaN or an infinity fails the comparisons)
                const bool ok = fabsf(xf) < kGuardBandPixels && fabsf(yf) < kGuardBandPixels && fabsf(cz) < __builtin_inff();
                inside = inside && ok;
                X[k] = ok ? (int32_t)__builtin_rintf(xf * 256.f) : 0;
                Y[k] = ok ? (int32_t)__builtin_rintf(yf * 256.f) : 0;
                z[k] = cz;
            }
            if (!inside) reject = true;
            else survivor = rastercov::setupTriangle(X, Y, z, p.res, p.res, &setupOf(rec), &rect);
            if constexpr (kAlphaTest)
                if (survivor) cutoutOfTriangle(args, found.draw, v, rec);
        }
    }
    // one 64-bit atomic per block hands it a run of slots (the low word is the cursor) and counts its triangles (the high word): a frame's waves adding to
    // the header one by one were most of this kernel's time (measured for 100 k triangles: 1569 waves x 4 atomics on one cache line, 62 us against 18)
    // (the prepass appends 0 .. 6 records per lane through a prefix sum of counts; this is one survivor per lane by ballot, and neither form serves the other)
    __shared__ uint32_t waveSurvivors[4], waveFound[4], waveRejects[4], blockBase;
    const unsigned long long foundMask = __ballot(found.found), rejectMask = __ballot(reject), survivorMask = __ballot(survivor);
    if (lane == 0) { waveSurvivors[wave] = (uint32_t)__popcll(survivorMask); waveFound[wave] = (uint32_t)__popcll(foundMask); waveRejects[wave] = (uint32_t)__popcll(rejectMask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t survivors = waveSurvivors[0] + waveSurvivors[1] + waveSurvivors[2] + waveSurvivors[3];
        const uint32_t foundHere = waveFound[0] + waveFound[1] + waveFound[2] + waveFound[3], rejects = waveRejects[0] + waveRejects[1] + waveRejects[2] + waveRejects[3];
        const unsigned long long old = atomicAdd((unsigned long long*)&p.header->cursor, (unsigned long long)survivors | ((unsigned long long)foundHere << 32));
        blockBase = (uint32_t)old;
        if (rejects) atomicAdd(&p.header->guardBandRejects, rejects);
    }
    __syncthreads();
    uint32_t base = blockBase;
    for (uint32_t w = 0; w < wave; w++) base += waveSurvivors[w];
    if (survivor) {
        const uint32_t slot = base + (uint32_t)__popcll(survivorMask & ((1ull << lane) - 1ull));
        if (slot < p.capacity) { // (always: the cursor counts at most triangleCount survivors and the launcher sized the arrays for that many)
            p.rects[slot] = rect;
            if constexpr (kAlphaTest) cutoutParams(args).records[slot] = rec;
            else p.records[slot] = rec;
        }
    }
}

struct TileParams {
    ScratchHeader* header; const uint32_t* rects; const SetupRecord* records;
    uint16_t* map;
    uint32_t capacity;
    int32_t res;
};
// a tested execution's tiles: `t.records` is null
struct CutoutTileParams {
    TileParams t;
    const CutoutRecord* records; const uint32_t* texels;
    uint64_t texelCount;
};
PLR_DI const TileParams& plainParams(const TileParams& a) { return a; }
PLR_DI const TileParams& plainParams(const CutoutTileParams& a) { return a.t; }
PLR_DI const SetupRecord* recordsOf(const TileParams& a) { return a.records; }
PLR_DI const CutoutRecord* recordsOf(const CutoutTileParams& a) { return a.records; }

// what becomes of a fragment: depth clamp, Depth16 code, maximum. tile: the block's 64 x 64 words
struct ShadowWalk : rastercov::PlainWalk {
    uint32_t* tile;
    int ox, oy;
    static PLR_DI const SetupRecord& setup(const SetupRecord& r) { return r; }
    template <class D> PLR_DI void fragment(const SetupRecord&, int, int px, int py, D&& depthAt) {
        float zf;
        if (!depthAt(&zf)) return;
        zf = fminf(fmaxf(zf, 0.f), 1.f);
        const uint32_t code = (uint32_t)__builtin_rintf(zf * 65535.f);
        atomicMax(&tile[(py - oy) * kTileSize + (px - ox)], code);
    }
};

// t mod n in [0, n) for |t| < 2^35 and 1 <= n <= 2^14: t / n is an integer or at least 2^-14 away from one, 16 times the spacing of fp64 at 2^34, so the floor
// of the fp64 quotient is the exact one (|u| < 2^20 and W <= 2^14 bound Tu >> 8 by 2^34)
PLR_DI int wrapRepeat(int64_t t, int n) {
    const double q = __builtin_floor((double)t / (double)n);
    return (int)(t - (int64_t)q * (int64_t)n);
}

// the alpha channel's weighted sum over the four taps of one level (w x h texels, the first at `base`); every address in 64 bits and checked before its load
// kFormats, bc3: the level is BC3 blocks and a tap decodes its alpha block alone (device/bc_decode.h, kFirst == 3: the block's word address is checked there)
template <bool kFormats = false>
PLR_DI uint32_t alphaTaps(const uint32_t* texels, uint64_t texelCount, uint64_t base, int w, int h, double u, double v, bool bc3 = false) {
    const int64_t Tu = (int64_t)__builtin_floor((u * (double)w - 0.5) * 256.0 + 0.5), Tv = (int64_t)__builtin_floor((v * (double)h - 0.5) * 256.0 + 0.5);
    const uint32_t fx = (uint32_t)(Tu & 255), fy = (uint32_t)(Tv & 255);
    const int x0 = wrapRepeat(Tu >> 8, w), y0 = wrapRepeat(Tv >> 8, h);
    const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
    auto fetch = [&](int x, int y) {
        if constexpr (kFormats) {
            if (bc3) return prepass::blockTexel<3>(texels, texelCount, base, kTextureFormatBc3, w, x, y) >> 24;
        }
        const uint64_t at = base + (uint64_t)y * (uint64_t)w + (uint64_t)x;
        return (at < texelCount ? texels[at] : 0u) >> 24;
    };
    return ((256u - fx) * (256u - fy) * fetch(x0, y0) + fx * (256u - fy) * fetch(x1, y0)) + ((256u - fx) * fy * fetch(x0, y1) + fx * fy * fetch(x1, y1));
}

// the alpha code of the fragment of record r with the depth's weights l1, l2 (the cutout contract)
template <bool kFormats = false>
PLR_DI uint32_t fragmentAlpha(const CutoutRecord& r, const uint32_t* texels, uint64_t texelCount, float l1, float l2) {
    const double u0 = (double)r.u0, v0 = (double)r.v0;
    double u = (u0 + (double)l1 * ((double)r.u1 - u0)) + (double)l2 * ((double)r.u2 - u0);
    double v = (v0 + (double)l1 * ((double)r.v1 - v0)) + (double)l2 * ((double)r.v2 - v0);
    if (!(__builtin_fabs(u) < 1048576.0 && __builtin_fabs(v) < 1048576.0)) u = v = 0.0; // (a NaN fails the comparison)
    const uint32_t fw = (r.test >> 16) & 255u;
    const uint64_t base = (uint64_t)r.base0Low | ((uint64_t)r.base0High << 32);
    const int w = (int)(r.size0 & 0xffffu), h = (int)(r.size0 >> 16);
    const bool bc3 = kFormats && ((r.test >> 25) & 1u) != 0u; // (a constant false in the RGBA8-tested instantiation: levelWords is then W H, the taps the texel taps)
    const uint32_t s0 = alphaTaps<kFormats>(texels, texelCount, base, w, h, u, v, bc3);
    uint32_t s1 = 0u;
    if (fw != 0u) // (with fw == 0 the upper level has no weight; with L1 == L0 it is the same level again)
        s1 = alphaTaps<kFormats>(texels, texelCount, (r.test >> 24) & 1u ? base + levelWords(bc3, (uint32_t)w, (uint32_t)h) : base, (int)(r.size1 & 0xffffu), (int)(r.size1 >> 16), u, v, bc3);
    const uint32_t S = (256u - fw) * s0 + fw * s1;
    return (S + 0x7fffffu + ((S >> 24) & 1u)) >> 24;
}

// a tested execution's fragment: the same, and a record with a cutoff samples its alpha before the maximum. kFormats: `texels` are the words of a format-aware
// store, texelCount their number, and a record is RGBA8 or BC3 (bit 25 of its test word)
template <bool kFormats>
struct CutoutWalk : rastercov::PlainWalk {
    uint32_t* tile;
    int ox, oy;
    const uint32_t* texels;
    uint64_t texelCount;
    uint32_t myCutoff; // of this lane's record of the step
    static PLR_DI const SetupRecord& setup(const CutoutRecord& r) { return r.s; }
    PLR_DI void beginStep(const CutoutRecord& rr, bool hit, bool, int, int, int, int) { myCutoff = hit ? rr.test & 0x1ffu : kAlphaCutoffOpaque; }
    PLR_DI bool lanePath() const { return myCutoff != kAlphaCutoffDiscardAll; } // a record with c = 256 is dropped whole
    PLR_DI bool beginStamps(int src) { return (uint32_t)__builtin_amdgcn_readlane((int)myCutoff, src) != kAlphaCutoffDiscardAll; }
    template <class D> PLR_DI void fragment(const CutoutRecord& r, int, int px, int py, D&& depthAt) {
        float zf, weights[2];
        if (!depthAt(&zf, weights)) return;
        zf = fminf(fmaxf(zf, 0.f), 1.f);
        const uint32_t code = (uint32_t)__builtin_rintf(zf * 65535.f);
        uint32_t* cell = &tile[(py - oy) * kTileSize + (px - ox)];
        const uint32_t c = r.test & 0x1ffu;
        if (c != kAlphaCutoffOpaque) { // the one branch: every other record's fragment goes the opaque way
            if (code <= *cell) return; // a filter only: the atomic below decides
            if (fragmentAlpha<kFormats>(r, texels, texelCount, weights[0], weights[1]) < c) return;
        }
        atomicMax(cell, code);
    }
};

template <int kMode>
__global__ __launch_bounds__(256) void sunShadowTileKernel(std::conditional_t<kMode != kAlphaUntested, CutoutTileParams, TileParams> args) {
    constexpr bool kAlphaTest = kMode != kAlphaUntested;
    const TileParams& p = plainParams(args);
    __shared__ uint32_t tile[kTileSize * kTileSize];
    __shared__ uint32_t hitQueue[4][256]; // per wave: the entries of the current step that touch the tile
    const int tx = (int)blockIdx.x, ty = (int)blockIdx.y;
    const int ox = tx * kTileSize, oy = ty * kTileSize;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kTileSize * kTileSize); i += 256u) tile[i] = 0u;
    __syncthreads();
    const uint32_t n = min(p.header->cursor, p.capacity);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.header->drawn = n;
    // the kernel's time in a busy tile is the hits' arithmetic
    const rastercov::TileWindow window{tx, ty, ox, oy, min(ox + kTileSize - 1, p.res - 1), min(oy + kTileSize - 1, p.res - 1)};
    if constexpr (kAlphaTest) {
        CutoutWalk<kMode == kAlphaFormats> walk{{}, tile, ox, oy, args.texels, args.texelCount, kAlphaCutoffOpaque};
        rastercov::rasteriseTile(p.rects, args.records, n, window, hitQueue[wave], walk);
    } else {
        ShadowWalk walk{{}, tile, ox, oy};
        rastercov::rasteriseTile(p.rects, p.records, n, window, hitQueue[wave], walk);
    }
    __syncthreads();
    // the tile as Depth16 rows: eight texels per 16-byte store where the eight lie inside the map and the address allows, texel by texel at ragged edges
    const bool rowsAligned = (p.res & 7) == 0;
    for (uint32_t c = threadIdx.x; c < (uint32_t)(kTileSize * kTileSize / 8); c += 256u) {
        const int row = (int)(c >> 3), col = (int)(c & 7u) * 8;
        const int y = oy + row, x = ox + col;
        if (y >= p.res || x >= p.res) continue;
        const uint32_t* src = tile + row * kTileSize + col;
        uint16_t* dst = p.map + (size_t)y * (size_t)p.res + (size_t)x;
        if (rowsAligned && x + 8 <= p.res) {
            uint4 v;
            v.x = src[0] | (src[1] << 16); v.y = src[2] | (src[3] << 16); v.z = src[4] | (src[5] << 16); v.w = src[6] | (src[7] << 16);
            *(uint4*)dst = v;
        } else {
            for (int k = 0; k < 8 && x + k < p.res; k++) dst[k] = (uint16_t)src[k];
        }
    }
}

static int launchSunShadowRaster(const PassCtx& c) {
    const uint32_t cascade = c.specUint(kCascadeIndexConstant, 0u);
    if (cascade >= 4u) return c.fail(-1, "sunShadowRaster: cascadeIndex (specialisation constant 0) is " + std::to_string(cascade) + ", a sunShadowInfo block holds 4 light matrices");
    if (c.push.size() < sizeof(PushConstants)) return c.fail(-1, "sunShadowRaster: push constants {drawCount, triangleCount} missing");
    FormatPushConstants pc{};
    std::memcpy(&pc, c.push.data(), std::min(c.push.size(), sizeof(pc)) / 4u * 4u); // 8 bytes: {drawCount, triangleCount}, textureCount 0; 12: textureFormats 0
    const bool tested = pc.textureCount != 0u, formatted = pc.textureFormats != 0u;
    if (formatted) {
        if (pc.textureFormats != 1u)
            return c.fail(-1, "sunShadowRaster: textureFormats is " + std::to_string(pc.textureFormats) + ", it must be 0 (every texture is RGBA8) or 1 (binding 14 holds a format code per texture)");
        if (!tested) return c.fail(-1, "sunShadowRaster: textureFormats is set and textureCount is 0 (a format belongs to a texture of the texture store)");
    }
    if (c.dispatch[0] != 1u || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "sunShadowRaster: the dispatch is {1, 1, 1} (the launcher derives its grids from the push constants and the map)");
    if (int rc = c.needSbuf(kSunShadowInfoBinding, sizeof(ShadowCascadeInfo), "sunShadowRaster sunShadowInfo")) return rc;
    if (int rc = c.needSbuf(kTransformBinding, 0, "sunShadowRaster transforms (mat4[])")) return rc;
    if (int rc = c.needSbuf(kPositionBinding, 0, "sunShadowRaster positions (3 floats per vertex)")) return rc;
    if (int rc = c.needSbuf(kIndexBinding, 0, "sunShadowRaster indices (uint32 triangle list)")) return rc;
    if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * sizeof(Draw), "sunShadowRaster draws {firstIndex, indexCount, vertexOffset, transformIndex}")) return rc;
    if (!tested) {
        if (int rc = c.needSbuf(kScratchBinding, scratchBytes(pc.triangleCount), "sunShadowRaster scratch (64 + 16 ceil(triangleCount / 4) + 80 triangleCount bytes)")) return rc;
    } else {
        if (int rc = c.needSbuf(kScratchBinding, cutoutScratchBytes(pc.triangleCount),
                                "sunShadowRaster scratch of an execution with textureCount > 0 (64 + 16 ceil(triangleCount / 4) + 128 triangleCount bytes)"))
            return rc;
        if (int rc = c.needSbuf(kUvBinding, 0, "sunShadowRaster uvs (binding 6: 2 floats per vertex)")) return rc;
        if (int rc = c.needSbuf(kCasterMaterialBinding, (size_t)pc.drawCount * sizeof(CasterMaterial), "sunShadowRaster casterMaterials (binding 7: {albedoTexture, cutoff} per draw)")) return rc;
        if (int rc = c.needSbuf(kTextureBinding, (size_t)pc.textureCount * sizeof(Texture), "sunShadowRaster textures (binding 8: {texelOffset, width, height, mipCount})")) return rc;
        if (int rc = c.needSbuf(kTexelBinding, 0, formatted ? "sunShadowRaster texels (binding 9: the words of a format-aware store - RGBA8 texels, BC1 / BC3 / BC5 blocks -, every texture's levels back to back)"
                                                            : "sunShadowRaster texels (binding 9: RGBA8, every texture's levels back to back)"))
            return rc;
        if (formatted)
            if (int rc = c.needSbuf(kTextureFormatBinding, (size_t)pc.textureCount * 4u, "sunShadowRaster textureFormats (binding 14: one uint32 format code per texture)")) return rc;
    }
    if (c.sbuf[kScratchBinding].readOnly) return c.fail(-4, "sunShadowRaster: the scratch buffer (binding 5) is bound read-only");
    if (int rc = c.needStorage(kMapBinding, F_D16, "sunShadowRaster shadow map")) return rc;
    const ImgView map = c.storage[kMapBinding];
    if (map.w != map.h || map.w < 1 || map.w > kMaxResolution || map.d > 1)
        return c.fail(-4, "sunShadowRaster: the shadow map is " + std::to_string(map.w) + " x " + std::to_string(map.h) + ", it must be square, 2D and at most 16384 texels wide");
    if ((pc.drawCount == 0u) != (pc.triangleCount == 0u)) return c.fail(-1, "sunShadowRaster: drawCount and triangleCount must both be zero or both be non-zero");
    for (int b : {kTransformBinding, kPositionBinding, kIndexBinding, kDrawBinding, kSunShadowInfoBinding})
        if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr) return c.fail(-4, "sunShadowRaster: the scratch buffer is also bound as an input");
    if (tested)
        for (int b : {kUvBinding, kCasterMaterialBinding, kTextureBinding, kTexelBinding})
            if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr)
                return c.fail(-4, "sunShadowRaster: the scratch buffer is also bound as an input (binding " + std::to_string(b) + ")");
    if (formatted && c.sbuf[kTextureFormatBinding].ptr == c.sbuf[kScratchBinding].ptr)
        return c.fail(-4, "sunShadowRaster: the scratch buffer is also bound as an input (binding 14, textureFormats)");

    uint8_t* scratch = (uint8_t*)c.sbuf[kScratchBinding].ptr;
    if (hipMemsetAsync(scratch, 0, sizeof(ScratchHeader), c.stream) != hipSuccess) return c.fail(-2, "sunShadowRaster: clearing the scratch header failed");
    if (pc.triangleCount) {
        FormatSetupParams fs{};
        CutoutSetupParams& cs = fs.c;
        SetupParams& s = cs.s;
        s.info = (const ShadowCascadeInfo*)c.sbuf[kSunShadowInfoBinding].ptr; s.transforms = (const float*)c.sbuf[kTransformBinding].ptr;
        s.positions = (const float*)c.sbuf[kPositionBinding].ptr; s.indices = (const uint32_t*)c.sbuf[kIndexBinding].ptr; s.draws = (const Draw*)c.sbuf[kDrawBinding].ptr;
        s.header = (ScratchHeader*)scratch; s.rects = (uint32_t*)(scratch + rectOffset());
        s.cascade = cascade; s.drawCount = pc.drawCount; s.triangleCount = pc.triangleCount; s.capacity = pc.triangleCount;
        s.transformCount = (uint32_t)std::min<size_t>(c.sbuf[kTransformBinding].size / 64u, 0xffffffffu);
        s.vertexCount = (uint32_t)std::min<size_t>(c.sbuf[kPositionBinding].size / 12u, 0xffffffffu);
        s.indexCount = (uint32_t)std::min<size_t>(c.sbuf[kIndexBinding].size / 4u, 0xffffffffu);
        s.res = map.w;
        if (tested) {
            cs.uvs = (const float*)c.sbuf[kUvBinding].ptr; cs.materials = (const CasterMaterial*)c.sbuf[kCasterMaterialBinding].ptr;
            cs.textures = (const Texture*)c.sbuf[kTextureBinding].ptr; cs.records = (CutoutRecord*)(scratch + recordOffset(pc.triangleCount));
            cs.uvVertexCount = c.sbuf[kUvBinding].size / 8u; cs.textureCount = pc.textureCount;
            if (formatted) {
                fs.formats = (const uint32_t*)c.sbuf[kTextureFormatBinding].ptr;
                sunShadowSetupKernel<kAlphaFormats><<<divUp(pc.triangleCount, 256u), 256, 0, c.stream>>>(fs);
            } else
                sunShadowSetupKernel<kAlphaRgba8><<<divUp(pc.triangleCount, 256u), 256, 0, c.stream>>>(cs);
        } else {
            s.records = (SetupRecord*)(scratch + recordOffset(pc.triangleCount));
            sunShadowSetupKernel<kAlphaUntested><<<divUp(pc.triangleCount, 256u), 256, 0, c.stream>>>(s);
        }
        PLR_CHECK_LAUNCH(c);
        c.splitTiming("set-up");
    }
    CutoutTileParams ct{};
    TileParams& t = ct.t;
    t.header = (ScratchHeader*)scratch; t.rects = (const uint32_t*)(scratch + rectOffset());
    t.map = (uint16_t*)map.ptr; t.capacity = pc.triangleCount; t.res = map.w;
    const unsigned tiles = divUp((unsigned)map.w, (unsigned)kTileSize);
    if (tested) {
        ct.records = (const CutoutRecord*)(scratch + recordOffset(pc.triangleCount)); ct.texels = (const uint32_t*)c.sbuf[kTexelBinding].ptr;
        ct.texelCount = c.sbuf[kTexelBinding].size / 4u;
        if (formatted) sunShadowTileKernel<kAlphaFormats><<<dim3(tiles, tiles), 256, 0, c.stream>>>(ct); // (texelCount: the words of the format-aware store)
        else sunShadowTileKernel<kAlphaRgba8><<<dim3(tiles, tiles), 256, 0, c.stream>>>(ct);
    } else {
        t.records = (const SetupRecord*)(scratch + recordOffset(pc.triangleCount));
        sunShadowTileKernel<kAlphaUntested><<<dim3(tiles, tiles), 256, 0, c.stream>>>(t);
    }
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace sunraster
static int sun_shadow_raster_launch(const PassCtx& c) { return sunraster::launchSunShadowRaster(c); }
static int sun_shadow_raster_launch_fast(const PassCtx& c) { return sunraster::launchSunShadowRaster(c); }
PLR_REGISTER_SHADER("sunShadowRaster.comp", sun_shadow_raster_launch);
PLR_REGISTER_SHADER_FAST("sunShadowRaster.comp", sun_shadow_raster_launch_fast);
} // namespace plr
