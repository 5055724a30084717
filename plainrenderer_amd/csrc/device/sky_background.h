// "skyAndSunSprite.comp": what the two kernels of the pass share (kernels/sky_background.hip, kernels_fast/sky_background_fast.hip). The pass is the
// compute form of Sky::renderSky (Techniques/Sky.cpp:318-353; sky.frag, sunSprite.vert / .frag) on the depth == 0 pixels of the colour buffer: DESIGN.md
// "Sky and sun disc as a compute pass".
#pragma once
#include "shading_common.h"

namespace plr {
struct PassCtx;
namespace skybg {

// bindings (extensions)
constexpr int kColorBinding = 0;        // storage image, R11G11B10
constexpr int kDepthBinding = 1;        // sampled, D32
constexpr int kSkyLutBinding = 2;       // sampled, R11G11B10
constexpr int kVolumeBinding = 3;       // sampled, RGBA16F 3D: volumetricIntegrationVolume
constexpr int kTransmissionBinding = 4; // sampled, R11G11B10
constexpr int kSettingsBinding = 5;     // uniform buffer: VolumetricLightingSettings
constexpr int kLightBinding = 6;        // storage buffer, read-only: LightBuffer
constexpr size_t kSettingsBytes = 52;   // std140 size of VolumetricLightingSettings

// spriteScale = tan(radians(sunAngularDiameter / 2)), sunAngularDiameter = 0.535 degrees (Sky.cpp:240-241), evaluated in fp32 like glm does
constexpr float kSunSpriteScale = 0x1.31f94cp-8f;
// chord 2 sin(atan(spriteScale) / 2) of the disc's angular radius on the unit sphere, rounded up (the fast kernel's tile test)
constexpr float kSunChord = 0.00466876f;
constexpr float kMaxVolumetricLightingDepth = 30.f; // volumetricFroxelLighting.inc:4
constexpr float kFroxelK = 3.f;                     // volumetricFroxelLighting.inc:20
constexpr float kSunBias = 0.002f;                  // sunSprite.frag:36

struct Params {
    ImgView color, depth, skyLut, volume, transmissionLut;
    const VolumetricLightingSettings* vol;
    const LightBuffer* light;
    const GlobalUbo* g;
    int coverW, coverH, yBase, xBase; // columns [xBase, coverW), rows [yBase, coverH)
};

// checks the bindings and fills the views and the covered rectangle (kernels/sky_background.hip); 0 or the error recorded on the context
int fillParams(const PassCtx& c, Params* P);

// limbDarkening's coefficients (sunSprite.frag:24)
#define PLR_SKY_LIMB_R 0.482f
#define PLR_SKY_LIMB_G 0.511f
#define PLR_SKY_LIMB_B 0.643f

} // namespace skybg
} // namespace plr
