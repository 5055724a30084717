// "skyAndSunSprite.comp": the sky behind geometry and the sun disc as ONE compute pass over the colour buffer, right after the deferred shade - the
// re-expression of the reference's two raster passes of Sky::renderSky (Techniques/Sky.cpp:318-353; sky.vert / sky.frag, sunSprite.vert / sunSprite.frag)
// the way "deferredShading.comp" stands in for triangle.frag. This is the general kernel: the reference's statements in the reference's order, IEEE
// arithmetic (no contraction), serving PLR_MATH_EXACT and every execution the fast kernel declines (kernels_fast/sky_background_fast.hip).
//
// Both raster passes test GreaterEqual at z = 0 under reverse-Z, so they touch exactly the pixels whose depth texel is 0; a pixel with geometry is neither
// read nor written here. The sky cube only supplies a view ray and the sun quad is a disc whose fragment inputs are closed-form functions of that ray and
// g_sunDirection (DESIGN.md "Sky and sun disc as a compute pass").
#include <algorithm>

#include "../backend.h"
#include "../device/sky_background.h"

namespace plr {
namespace skybg {

__global__ __launch_bounds__(256) void skyAndSunSpriteKernel(Params P) {
    const int px = P.xBase + (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int py = P.yBase + (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (px >= P.coverW || py >= P.coverH) return;
    if (texelFetch2D<F_D32>(P.depth, px, py).x != 0.f) return;
    const GlobalUbo* g = P.g;
    // the ray of the deferred pass' sky stand-in (kernels_exact/shading.hip): the pixel centre under the unjittered camera
    const vec2 screenRes((float)g->screenResolution[0], (float)g->screenResolution[1]);
    const vec2 fragCoord((float)px + 0.5f, (float)py + 0.5f);
    const vec2 screenUV = fragCoord / screenRes;
    const vec2 pixelNDC(screenUV.x * 2.f - 1.f, screenUV.y * 2.f - 1.f);
    const vec3 V = -calculateViewDirectionFromPixel(pixelNDC, ld3(g->cameraForward), ld3(g->cameraUp), ld3(g->cameraRight), g->cameraTanFovHalf, g->cameraAspectRatio);

    // ---- sky.frag:20-33
    vec3 color = sampleSkyLut(V, P.skyLut);
    // ditherRGB8(color, ivec2(gl_FragCoord.xy * g_screenResolution)) (sic)
    const vec2 ditherCoord = fragCoord * screenRes;
    color = color + ditherRGB8Noise((float)(int32_t)ditherCoord.x, (float)(int32_t)ditherCoord.y, g->time);
    // volumeTextureLookup(screenUV, maxVolumetricLightingDepth, ...) + applyInscatteringTransmittance (volumetricFroxelLighting.inc:33-53)
    const float linear = kMaxVolumetricLightingDepth / P.vol->maxDistance;
    const float uvZ = det_logf(linear * (det_expf(kFroxelK) - 1.f) + 1.f) / kFroxelK;
    const vec4 it = sampleLinear3D<F_RGBA16F, CLAMP>(P.volume, vec3(screenUV.x, screenUV.y, uvZ));
    color = color * it.w + it.xyz();
    uint32_t stored = packR11G11B10(color); // the sky pass' render target value; the sun sprite is blended onto it

    // ---- sunSprite.vert / .frag with Sky::issueSkyDrawcalls' model matrix (Sky.cpp:237-258): the quad's centre is g_sunDirection, its plane is
    // perpendicular to it at distance 1, passWorldPos is the ray's point on that plane and passQuadPos that point's offset from the centre in sprite radii
    const vec3 S = ld3(g->sunDirection);
    const float cosT = dot(V, S);
    if (cosT > 0.f) {
        const vec3 q = V / cosT;
        const vec3 off = q - S;
        const float distanceFromCenter = dot(off, off) / (kSunSpriteScale * kSunSpriteScale);
        if (!(distanceFromCenter > 1.f)) {
            const vec3 Vt = normalize(q + vec3(0.f, kSunBias, 0.f));
            // computeLutUV(0, 100, vec3(0, -1, 0), V) (sky.inc:105-110)
            const vec2 lutUV(0.f / 100.f, dot(vec3(0.f, -1.f, 0.f), Vt) * 0.5f + 0.5f);
            const vec3 transmission = sampleLinear2D<F_R11G11B10, CLAMP>(P.transmissionLut, lutUV).xyz();
            const float mu = sqrtf(1.f - distanceFromCenter);
            const vec3 limb(det_powf(mu, PLR_SKY_LIMB_R), det_powf(mu, PLR_SKY_LIMB_G), det_powf(mu, PLR_SKY_LIMB_B));
            const vec3 sun = P.light->sunStrengthExposed * transmission * limb;
            float alpha = 1.f - distanceFromCenter;
            alpha *= alpha;
            // "Additive" blend state (Backend/RenderPass.cpp:117-123): src.rgb * src.a + dst.rgb * dst.a, and an R11G11B10 target reads alpha 1
            stored = packR11G11B10(unpackR11G11B10(stored) + sun * alpha);
        }
    }
    ((uint32_t*)P.color.ptr)[(size_t)py * (size_t)P.color.w + px] = stored;
}

// bindings and the covered rectangle; shared with the fast launcher
int fillParams(const PassCtx& c, Params* P) {
    if (int rc = c.needGlobal()) return rc;
    if (int rc = c.needStorage(kColorBinding, F_R11G11B10, "skyAndSunSprite colour target")) return rc;
    if (int rc = c.needSampled(kDepthBinding, F_D32, "skyAndSunSprite depth")) return rc;
    if (int rc = c.needSampled(kSkyLutBinding, F_R11G11B10, "skyAndSunSprite skyLut")) return rc;
    if (int rc = c.needSampled(kVolumeBinding, F_RGBA16F, "skyAndSunSprite volumetricLightingLUT")) return rc;
    if (int rc = c.needSampled(kTransmissionBinding, F_R11G11B10, "skyAndSunSprite transmissionLut")) return rc;
    if (int rc = c.needUbuf(kSettingsBinding, kSettingsBytes, "skyAndSunSprite volumetric settings")) return rc;
    if (int rc = c.needSbuf(kLightBinding, sizeof(LightBuffer), "skyAndSunSprite lightBuffer")) return rc;
    P->color = c.storage[kColorBinding]; P->depth = c.sampled[kDepthBinding]; P->skyLut = c.sampled[kSkyLutBinding]; P->volume = c.sampled[kVolumeBinding];
    P->transmissionLut = c.sampled[kTransmissionBinding];
    P->vol = (const VolumetricLightingSettings*)c.ubuf[kSettingsBinding].ptr; P->light = (const LightBuffer*)c.sbuf[kLightBinding].ptr; P->g = c.global;
    for (const ImgView* v : {&P->skyLut, &P->volume, &P->transmissionLut})
        if (v->w < 1 || v->h < 1 || v->d < 1) return c.fail(-4, "skyAndSunSprite: an empty lookup image");
    // invocations exist for dispatch * 8 pixels; stores outside the target are dropped and a depth fetch outside the depth image reads 0 in the reference, which
    // would make everything beyond it sky: the covered region is clipped to both images (as the tonemap clips to source and target)
    const PassCtx::RowSpan rs = c.rowSpan(std::min(P->color.h, P->depth.h));
    const PassCtx::ColSpan cs = c.colSpan(std::min(P->color.w, P->depth.w));
    P->coverW = cs.x1; P->xBase = cs.x0; P->coverH = rs.y1; P->yBase = rs.y0;
    return 0;
}

static int launchSkyAndSunSprite(const PassCtx& c) {
    Params P{};
    if (int rc = fillParams(c, &P)) return rc;
    if (P.coverW <= P.xBase || P.coverH <= P.yBase) return 0;
    skyAndSunSpriteKernel<<<dim3(divUp((unsigned)(P.coverW - P.xBase), 64u), divUp((unsigned)(P.coverH - P.yBase), 4u)), 256, 0, c.stream>>>(P);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace skybg
static int sky_and_sun_sprite_launch(const PassCtx& c) { return skybg::launchSkyAndSunSprite(c); }
PLR_REGISTER_SHADER("skyAndSunSprite.comp", sky_and_sun_sprite_launch);
} // namespace plr
