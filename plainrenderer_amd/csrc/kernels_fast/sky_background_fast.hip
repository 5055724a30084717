// PLR_MATH_FAST kernel of "skyAndSunSprite.comp" (general kernel and the pass' definition: kernels/sky_background.hip; DESIGN.md "Sky and sun disc as a compute
// pass"). The pass reads 4 B of depth per pixel and writes 4 B on sky pixels only, so what the kernel is built around is doing nothing quickly where there
// is geometry and little where there is sky:
//  * a wave owns one row of 256 pixels, a lane four neighbouring pixels: ONE 16-byte depth load per lane, and a wave whose 256 texels are all geometry
//    leaves right behind it (the colour buffer is never read, geometry pixels are never written);
//  * everything that is constant over the frame or along a row is computed once per wave from scalar loads of the uniform blocks, not per pixel: the
//    froxel lookup's uv.z with its two slices and their weight (the depth is the constant 30), the row's froxel rows and their weight, the row's part
//    of the view ray, the row terms of the two dither hashes (as kernels_fast/stream_fast.hip tonemapRowTerms);
//  * the froxel footprint is reduced over z and y to its two columns when a pixel enters a new footprint (every 8th pixel), so a pixel's lookup is one lerp;
//  * the sun disc is 0.535 degrees wide - a handful of 256 x 4 tiles of a frame can see it. Each workgroup decides once, from its tile's corner rays,
//    whether the disc can reach the tile (a cone around the tile's centre ray that contains the corners contains the tile: the rays within an angle of
//    an axis cut the image plane in a convex set); only those tiles run the sprite code.
#include "../backend.h"
#include "../device/fastmath.h"
#include "../device/sky_background.h"

namespace plr {
namespace skybg {

PLR_DI vec3 halves4xyz(uint2 u, float* w) {
    *w = halfBitsToFloat(u.y >> 16);
    return vec3(halfBitsToFloat(u.x & 0xffffu), halfBitsToFloat(u.x >> 16), halfBitsToFloat(u.y & 0xffffu));
}

// the view ray through a point of the image plane (screenToWorld.inc:4-9 negated, not normalised): forward - tan * ndc.y * up + tan * aspect * ndc.x * right
struct RayBasis { vec3 fwd, up, right; float tanY, tanX, invResX, invResY; };
PLR_DI vec3 rayThrough(const RayBasis& B, float fx, float fy) {
    const float ndcX = fx * B.invResX * 2.f - 1.f, ndcY = fy * B.invResY * 2.f - 1.f;
    return B.fwd - (B.tanY * ndcY) * B.up + (B.tanX * ndcX) * B.right;
}
PLR_DI vec3 unit(vec3 v) { return v * __builtin_amdgcn_rsqf(dot(v, v)); }

__global__ __launch_bounds__(256) void skyAndSunSpriteFastKernel(Params P) {
    const int lane = (int)(threadIdx.x & 63u);
    const int tileX0 = P.xBase + (int)blockIdx.x * 256, tileY0 = P.yBase + (int)blockIdx.y * 4;
    const int x0 = tileX0 + lane * 4; // xBase is a multiple of 8 (PassCtx::colSpan): x0 is a multiple of 4
    const int y = tileY0 + (int)(threadIdx.x >> 6);
    if (y >= P.coverH) return;
    const int n = min(4, P.coverW - x0); // <= 0: a lane beyond the last column
    // ---- depth: four texels per lane in one load where the rows are 16-byte aligned
    float d[4] = {1.f, 1.f, 1.f, 1.f};
    const float* drow = (const float*)P.depth.ptr + (size_t)y * (size_t)P.depth.w;
    if (n == 4 && (P.depth.w & 3) == 0) {
        const float4 v = *(const float4*)(drow + x0);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (i < n) d[i] = drow[x0 + i];
    }
    uint32_t sky = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) sky |= (i < n && d[i] == 0.f) ? (1u << i) : 0u;
    if (__builtin_amdgcn_ballot_w64(sky != 0u) == 0ull) return; // a wave of geometry: done

    // ---- constants of the frame and of this row (wave-uniform; the uniform blocks are read with scalar loads)
    const GlobalUbo* g = P.g;
    const float resX = (float)g->screenResolution[0], resY = (float)g->screenResolution[1], time = g->time;
    RayBasis B;
    B.fwd = ld3(g->cameraForward); B.up = ld3(g->cameraUp); B.right = ld3(g->cameraRight);
    B.tanY = g->cameraTanFovHalf; B.tanX = g->cameraTanFovHalf * g->cameraAspectRatio;
    B.invResX = 1.f / resX; B.invResY = 1.f / resY;
    const vec3 S = ld3(g->sunDirection);
    const float fy = (float)y + 0.5f;
    const float v = fy * B.invResY;
    const vec3 rowRay = B.fwd - (B.tanY * (v * 2.f - 1.f)) * B.up;
    // dither.inc:6-12 on ivec2(gl_FragCoord.xy * g_screenResolution) (sky.frag:27): the y terms of the two hashes
    const uint32_t UI0 = 1597334673u, UI1 = 3812015801u, UI2 = 2798796415u;
    const float uy = (float)(int32_t)(fy * resY);
    const uint32_t nyA = (uint32_t)(int32_t)(float)(uint32_t)(uy * time) * UI1, nyB = (uint32_t)(int32_t)(float)(uint32_t)((uy + 1292.f) * time) * UI1;
    // volumeTextureLookup at the constant depth 30 (volumetricFroxelLighting.inc:33-50): slices k0 / k1 with weight wz, rows j0 / j1 with weight wy
    const ImgView& vol = P.volume;
    int k0, j0; float wz, wy;
    {
        const float linear = kMaxVolumetricLightingDepth / P.vol->maxDistance;
        const float uvZ = det_logf(linear * (det_expf(kFroxelK) - 1.f) + 1.f) / kFroxelK;
        linearCoord(uvZ * (float)vol.d, &k0, &wz);
        linearCoord(v * (float)vol.h, &j0, &wy);
    }
    const int k1 = clampi(k0 + 1, vol.d), j1 = clampi(j0 + 1, vol.h);
    k0 = clampi(k0, vol.d); j0 = clampi(j0, vol.h);
    const uint2* vrow[4] = {(const uint2*)vol.ptr + ((size_t)k0 * (size_t)vol.h + (size_t)j0) * (size_t)vol.w, (const uint2*)vol.ptr + ((size_t)k0 * (size_t)vol.h + (size_t)j1) * (size_t)vol.w,
                            (const uint2*)vol.ptr + ((size_t)k1 * (size_t)vol.h + (size_t)j0) * (size_t)vol.w, (const uint2*)vol.ptr + ((size_t)k1 * (size_t)vol.h + (size_t)j1) * (size_t)vol.w};
    const float wrow[4] = {(1.f - wz) * (1.f - wy), (1.f - wz) * wy, wz * (1.f - wy), wz * wy};

    // ---- can the sun disc reach this workgroup's tile? pixel rectangle [tileX0, tx1) x [tileY0, ty1), outer edges; chords on the unit sphere obey the
    // triangle inequality: |centre ray - sun| <= max |centre ray - corner ray| + the disc's chord, with room for the rounding of the rays
    bool sunTile;
    {
        const float tx0 = (float)tileX0, tx1 = (float)min(tileX0 + 256, P.coverW), ty0 = (float)tileY0, ty1 = (float)min(tileY0 + 4, P.coverH);
        const vec3 centre = unit(rayThrough(B, 0.5f * (tx0 + tx1), 0.5f * (ty0 + ty1)));
        float reach = 0.f;
        for (int k = 0; k < 4; k++) {
            const vec3 c = unit(rayThrough(B, (k & 1) ? tx1 : tx0, (k & 2) ? ty1 : ty0)) - centre;
            reach = __builtin_fmaxf(reach, dot(c, c));
        }
        const float s2 = dot(S, S);
        const vec3 toSun = S * __builtin_amdgcn_rsqf(s2) - centre;
        const float limit = (__builtin_amdgcn_sqrtf(reach) + kSunChord) * 1.02f + 1e-5f;
        // a sun direction that is not a unit vector moves and resizes the disc (the sprite plane is where dot(q, S) = 1): no shortcut then
        sunTile = dot(toSun, toSun) <= limit * limit || !(fabsf(s2 - 1.f) <= 1e-4f);
    }
    const float sunStrengthExposed = P.light->sunStrengthExposed;

    uint32_t out[4] = {0u, 0u, 0u, 0u};
    int footprint = 0x7fffffff; // i0 of the froxel columns held in colL / colR
    vec3 colL(0.f), colR(0.f);
    float alphaL = 1.f, alphaR = 1.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (!(sky & (1u << i))) continue;
        const float fx = (float)(x0 + i) + 0.5f;
        const float u = fx * B.invResX;
        const vec3 V = unit(rowRay + (B.tanX * (u * 2.f - 1.f)) * B.right);
        vec3 color = fastm::sampleSkyLut(V, P.skyLut);
        // ditherRGB8
        {
            const float ux = (float)(int32_t)(fx * resX);
            const uint32_t qxA = (uint32_t)(int32_t)(float)(uint32_t)(ux * time), qxB = (uint32_t)(int32_t)(float)(uint32_t)((ux + 165.f) * time);
            const uint32_t mA = (qxA * UI0) ^ nyA ^ (qxA * UI2), mB = (qxB * UI0) ^ nyB ^ (qxB * UI2);
            const float UIF = 1.0f / (float)0xffffffffu;
            const vec3 noise = (vec3((float)(mA * UI0), (float)(mA * UI1), (float)(mA * UI2)) + vec3((float)(mB * UI0), (float)(mB * UI1), (float)(mB * UI2))) * UIF - 1.f;
            color = color + noise * (1.f / 255.f);
        }
        // froxel in-scattering and transmittance
        {
            int i0; float wx;
            linearCoord(u * (float)vol.w, &i0, &wx);
            if (i0 != footprint) {
                footprint = i0;
                const int xl = clampi(i0, vol.w), xr = clampi(i0 + 1, vol.w);
                colL = vec3(0.f); colR = vec3(0.f); alphaL = 0.f; alphaR = 0.f;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float al, ar;
                    const vec3 l = halves4xyz(vrow[r][xl], &al), rr = halves4xyz(vrow[r][xr], &ar);
                    colL = colL + l * wrow[r]; colR = colR + rr * wrow[r];
                    alphaL += al * wrow[r]; alphaR += ar * wrow[r];
                }
            }
            const vec3 inscattering = colL + (colR - colL) * wx;
            const float transmittance = alphaL + (alphaR - alphaL) * wx;
            color = color * transmittance + inscattering;
        }
        uint32_t stored = packR11G11B10(color);
        if (sunTile) { // workgroup-uniform
            const float cosT = dot(V, S);
            if (cosT > 0.f) {
                const vec3 q = V / cosT;
                const vec3 off = q - S; // (not 1 - cosT^2: that loses half the mantissa at a quarter of a degree)
                const float d2 = dot(off, off) * (1.f / (kSunSpriteScale * kSunSpriteScale));
                if (!(d2 > 1.f)) {
                    const vec3 Vt = unit(q + vec3(0.f, kSunBias, 0.f));
                    const vec3 transmission = sampleLinear2D<F_R11G11B10, CLAMP>(P.transmissionLut, vec2(0.f, -Vt.y * 0.5f + 0.5f)).xyz();
                    const float logMu = __builtin_amdgcn_logf(__builtin_amdgcn_sqrtf(1.f - d2)); // log2; mu = 0: -inf, the powers are 0
                    const vec3 limb(__builtin_amdgcn_exp2f(PLR_SKY_LIMB_R * logMu), __builtin_amdgcn_exp2f(PLR_SKY_LIMB_G * logMu), __builtin_amdgcn_exp2f(PLR_SKY_LIMB_B * logMu));
                    const float alpha = (1.f - d2) * (1.f - d2);
                    stored = packR11G11B10(unpackR11G11B10(stored) + (sunStrengthExposed * transmission * limb) * alpha);
                }
            }
        }
        out[i] = stored;
    }
    // ---- stores: sky pixels only. Four sky pixels of an aligned row go out as one 16-byte store, anything else texel by texel
    uint32_t* crow = (uint32_t*)P.color.ptr + (size_t)y * (size_t)P.color.w;
    if (sky == 15u && (P.color.w & 3) == 0) *(uint4*)(crow + x0) = make_uint4(out[0], out[1], out[2], out[3]);
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (sky & (1u << i)) crow[x0 + i] = out[i];
    }
}

static int launchSkyAndSunSpriteFast(const PassCtx& c) {
    Params P{};
    if (int rc = fillParams(c, &P)) return rc;
    // built for: a depth buffer of the colour target's size (one row index for both) and images below 2^24 texels a side (fastm::texelIndex)
    if (P.depth.w != P.color.w || P.depth.h != P.color.h) return kUseGeneralKernel;
    if (P.skyLut.w >= (1 << 24) || P.skyLut.h >= (1 << 24) || P.skyLut.d != 1 || P.transmissionLut.d != 1) return kUseGeneralKernel;
    if (P.coverW <= P.xBase || P.coverH <= P.yBase) return 0;
    skyAndSunSpriteFastKernel<<<dim3(divUp((unsigned)(P.coverW - P.xBase), 256u), divUp((unsigned)(P.coverH - P.yBase), 4u)), 256, 0, c.stream>>>(P);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace skybg
static int sky_and_sun_sprite_fast_launch(const PassCtx& c) { return skybg::launchSkyAndSunSpriteFast(c); }
PLR_REGISTER_SHADER_FAST("skyAndSunSprite.comp", sky_and_sun_sprite_fast_launch);
} // namespace plr
