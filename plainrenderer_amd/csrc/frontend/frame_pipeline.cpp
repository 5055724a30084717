// See frame_pipeline.h. Pass order, bindings, specialisation constants and dispatch counts follow the cited reference code.
#include "frame_pipeline.h"
#include "../device/depth_prepass_raster.h"
#include "../device/debug_geometry.h"
#include "../device/draw_culling.h"
#include "../device/noise.h"
#include "../device/scene_sdf.h"
#include "../device/sun_shadow_raster.h"
#include "../device/texture_build.h"

#include "../../../include/plr_image_io.h"
#include "../../../include/plr_sdf_bake.h"

#include <hip/hip_runtime_api.h> // hipGetDevice: the device the scene's SDF volumes are baked on

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace plrhost {

// ------------------------------------------------------------------ small math (the reference uses glm)
static Vec3 operator+(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static Vec3 operator-(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static Vec3 operator*(Vec3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
static Vec3 normalize(Vec3 a) { const float l = std::sqrt(dot(a, a)); return {a.x / l, a.y / l, a.z / l}; }
static Mat4 mul(const Mat4& a, const Mat4& b) {
    Mat4 r{};
    for (int c = 0; c < 4; c++)
        for (int row = 0; row < 4; row++) {
            float s = 0.f;
            for (int k = 0; k < 4; k++) s += a.m[k * 4 + row] * b.m[c * 4 + k];
            r.m[c * 4 + row] = s;
        }
    return r;
}
static Mat4 identity() { Mat4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.f; return r; }

// Camera.cpp:4-12
static Mat4 viewMatrixFromCameraExtrinsic(const CameraExtrinsic& e) {
    Mat4 rot = identity(); // rows = right, up, -forward
    rot.m[0] = e.right.x; rot.m[4] = e.right.y; rot.m[8] = e.right.z;
    rot.m[1] = e.up.x; rot.m[5] = e.up.y; rot.m[9] = e.up.z;
    rot.m[2] = -e.forward.x; rot.m[6] = -e.forward.y; rot.m[10] = -e.forward.z;
    Mat4 t = identity();
    t.m[12] = -e.position.x; t.m[13] = -e.position.y; t.m[14] = -e.position.z;
    return mul(rot, t);
}
// Camera.cpp:14-27: glm::perspective (RH, -1..1) then the Vulkan Y flip / reverse-Z correction
static Mat4 projectionMatrixFromCameraIntrinsic(const CameraIntrinsic& in) {
    const float f = 1.f / std::tan(in.fov * 3.14159265358979f / 180.f * 0.5f);
    Mat4 p{};
    p.m[0] = f / in.aspectRatio;
    p.m[5] = f;
    p.m[10] = -(in.far + in.near) / (in.far - in.near);
    p.m[11] = -1.f;
    p.m[14] = -(2.f * in.far * in.near) / (in.far - in.near);
    Mat4 corr{};
    corr.m[0] = 1.f; corr.m[5] = -1.f; corr.m[10] = -0.5f; corr.m[14] = 0.5f; corr.m[15] = 1.f;
    return mul(corr, p);
}

// Common/Utilities/MathUtils.cpp:17-23
static uint32_t mipCountFromResolution(uint32_t w, uint32_t h, uint32_t d) { return 1 + (uint32_t)std::floor(std::log2((float)std::max(std::max(w, h), d))); }
static void resolutionFromMip(int w, int h, int mip, int* ow, int* oh) { *ow = std::max(w / (1 << mip), 1); *oh = std::max(h / (1 << mip), 1); }
// MathUtils.cpp:25-60
static float radicalInverseBase2(uint32_t in) {
    uint32_t out = (in << 16) | (in >> 16);
    out = ((out & 0x00ff00ff) << 8) | ((out & 0xff00ff00) >> 8);
    out = ((out & 0x0f0f0f0f) << 4) | ((out & 0xf0f0f0f0) >> 4);
    out = ((out & 0x33333333) << 2) | ((out & 0xcccccccc) >> 2);
    out = ((out & 0x55555555) << 1) | ((out & 0xaaaaaaaa) >> 1);
    return float(out) * (float)2.3283064365386963e-10;
}
static float radicalInverseBase3(uint32_t in) {
    const uint32_t base = 3;
    const float inverseBase = 1.f / (float)base;
    uint32_t reversedDigits = 0, current = in;
    float inverseBasePowerN = 1;
    while (current) {
        const uint32_t next = current / base;
        const uint32_t digit = current - next * base;
        reversedDigits = reversedDigits * base + digit;
        inverseBasePowerN *= inverseBase;
        current = next;
    }
    return reversedDigits * inverseBasePowerN;
}

template <class T> static SpecialisationConstant spec(uint32_t location, const T& v) { return {location, dataToCharArray(&v, sizeof(T))}; }

static ImageDescription desc2D(uint32_t w, uint32_t h, ImageFormat f, ImageUsageFlags usage = ImageUsageFlags::Storage | ImageUsageFlags::Sampled,
                               MipCount mips = MipCount::One, uint32_t manual = 1) {
    ImageDescription d;
    d.width = w; d.height = h; d.depth = 1; d.type = ImageType::Type2D; d.format = f; d.usageFlags = usage; d.mipCount = mips; d.manualMipCount = manual;
    return d;
}
// 8x8 workgroups over a w x h image; rows restricts the dispatch to the workgroup rows touching [rows.begin, rows.end)
// cols (tile rendering) does the same for the workgroup columns
static void dispatch8(ComputePassExecution& exe, uint32_t w, uint32_t h, RowRange rows = {}, ColRange cols = {}) {
    const uint32_t lo = std::min(rows.begin, h), hi = std::min(rows.end, h);
    const uint32_t cl = std::min(cols.begin, w), ch = std::min(cols.end, w);
    exe.dispatchBase[0] = cl / 8;
    exe.dispatchCount[0] = ch > cl ? (ch + 7) / 8 - cl / 8 : 0;
    exe.dispatchBase[1] = lo / 8;
    exe.dispatchCount[1] = hi > lo ? (hi + 7) / 8 - lo / 8 : 0;
    exe.dispatchCount[2] = 1;
}

void recordRows(RenderBackend& be, ComputePassExecution& exe, uint32_t w, uint32_t h, RowRange rows, uint32_t halo, const std::function<void()>& edgesDone, bool rowsFirst, ColRange cols) {
    const uint32_t r0 = std::min(rows.begin, h), r1 = std::min(rows.end, h);
    const uint32_t c0 = std::min(cols.begin, w), c1 = std::min(cols.end, w);
    const bool tiled = c0 > 0 || c1 < w;
    // (a tile's producers are one execution each: the split into an edge and an interior execution of round 3 exists for whole rows only)
    if (!edgesDone || halo == 0 || r1 <= r0 || c1 <= c0 || (tiled && !rowsFirst)) {
        dispatch8(exe, w, h, rows, cols);
        be.setComputePassExecution(exe);
        if (edgesDone) edgesDone();
        return;
    }
    // rows the band above / below needs first; a pass's result does not depend on how its rows are split over dispatches
    // (edges rounded up to 16 rows: the coarsest launch granularity of a pass, two 8-row workgroups of the trace)
    halo = (halo + 15u) & ~15u;
    // split points on 16-row boundaries of the image; no edge on a side without a neighbouring band (first / last rows of the image)
    const uint32_t topEnd = r0 == 0 ? r0 : std::min((r0 + halo + 15u) & ~15u, r1);
    const uint32_t bottomBegin = r1 >= h ? r1 : std::max((r1 > halo ? r1 - halo : 0u) & ~15u, topEnd);
    // the same for the columns of a tile: no edge on a side without a neighbouring tile (first / last columns of the image)
    const uint32_t leftEnd = c0 == 0 ? c0 : std::min((c0 + halo + 15u) & ~15u, c1);
    const uint32_t rightBegin = c1 >= w ? c1 : std::max((c1 > halo ? c1 - halo : 0u) & ~15u, leftEnd);
    if (rowsFirst && (topEnd > r0 || bottomBegin < r1 || leftEnd > c0 || rightBegin < c1)) {
        // one launch: the kernel takes the edge rows (and columns) first and the backend raises its edge signal when they are written (plr.h first_rows / first_cols,
        // workgroup rows / columns of 8)
        ComputePassExecution e = exe;
        dispatch8(e, w, h, RowRange{r0, r1}, cols);
        e.firstRows[0] = topEnd / 8u;
        e.firstRows[1] = bottomBegin / 8u;
        if (tiled) { e.firstCols[0] = leftEnd / 8u; e.firstCols[1] = rightBegin / 8u; }
        be.setComputePassExecution(e);
        edgesDone();
        return;
    }
    if (tiled) { // (edges asked for, none needed: a tile without neighbours)
        dispatch8(exe, w, h, rows, cols);
        be.setComputePassExecution(exe);
        edgesDone();
        return;
    }
    auto part = [&](uint32_t a, uint32_t b) {
        if (b <= a) return;
        ComputePassExecution e = exe;
        dispatch8(e, w, h, RowRange{a, b});
        be.setComputePassExecution(e);
    };
    part(r0, topEnd);
    part(bottomBegin, r1);
    edgesDone();
    part(topEnd, bottomBegin);
}
static RowRange scaleRows(RowRange r, uint32_t divisor) { // the rows of a 1/divisor resolution image that cover r
    if (r.end == 0xffffffffu && r.begin == 0) return r;
    return {r.begin / divisor, (r.end + divisor - 1) / divisor};
}

// ------------------------------------------------------------------ TAA (Techniques/TAA.cpp)
static ShaderDescription temporalFilterShaderDescription(const TAASettings& s) { // TAA.cpp:204-233
    ShaderDescription d;
    d.srcPathRelative = "temporalFilter.comp";
    d.specialisationConstants = {spec(0, s.useClipping), spec(1, s.useMotionVectorDilation), spec(2, s.historySamplingTech), spec(3, s.filterUseTonemapping)};
    return d;
}
void TAA::init(RenderBackend& be, int w, int h, const TAASettings& settings) { // TAA.cpp:7-67
    ComputePassDescription d;
    d.name = "Temporal filtering";
    d.shaderDescription = temporalFilterShaderDescription(settings);
    m_temporalFilterPass = be.createComputePass(d);
    for (int i = 0; i < 2; i++) m_historyBuffers[i] = be.createImage(desc2D(w, h, ImageFormat::R11G11B10_uFloat), nullptr, 0);
    for (int i = 0; i < 2; i++) m_sceneLuminance[i] = be.createImage(desc2D(w, h, ImageFormat::R8), nullptr, 0); // TAA.cpp:38-53
    {
        ComputePassDescription sd; // TAA.cpp:20-36, 235-245
        sd.name = "Temporal supersampling";
        sd.shaderDescription.srcPathRelative = "temporalSupersampling.comp";
        sd.shaderDescription.specialisationConstants = {spec(0, settings.supersampleUseTonemapping)};
        m_temporalSupersamplingPass = be.createComputePass(sd);
        ComputePassDescription ld;
        ld.name = "Color to Luminance";
        ld.shaderDescription.srcPathRelative = "colorToLuminance.comp";
        m_colorToLuminancePass = be.createComputePass(ld);
    }
    UniformBufferDescription ub;
    ub.size = sizeof(float) * 9;
    for (auto& b : m_taaResolveWeightBuffers) b = be.createUniformBuffer(ub);
    m_taaResolveWeightBuffer = m_taaResolveWeightBuffers[0];
}
void TAA::resizeImages(RenderBackend& be, int w, int h) { // TAA.cpp:69-78
    be.resizeImages({m_historyBuffers[0], m_historyBuffers[1], m_sceneLuminance[0], m_sceneLuminance[1]}, w, h);
}
void TAA::updateSettings(RenderBackend& be, const TAASettings& settings) { // TAA.cpp:80-83
    be.updateComputePassShaderDescription(m_temporalFilterPass, temporalFilterShaderDescription(settings));
    ShaderDescription sd;
    sd.srcPathRelative = "temporalSupersampling.comp";
    sd.specialisationConstants = {spec(0, settings.supersampleUseTonemapping)};
    be.updateComputePassShaderDescription(m_temporalSupersamplingPass, sd);
}
void TAA::computeTemporalFilter(RenderBackend& be, const FrameIndexCounter& fi, ImageHandle colorSrc, const FrameRenderTargets& currentFrame, ImageHandle target,
                                RowRange rows, uint32_t edgeRows, const std::function<void()>& edgesDone, bool rowsFirst, ColRange cols) const {
    // TAA.cpp:139-166
    const size_t frameIndexMod2 = fi.mod2();
    const ImageHandle historySrc = m_historyBuffers[frameIndexMod2];
    const ImageHandle historyDst = m_historyBuffers[(frameIndexMod2 + 1) % 2];
    const ImageDescription td = be.getImageDescription(target);
    ComputePassExecution exe;
    exe.genericInfo.handle = m_temporalFilterPass;
    exe.genericInfo.resources.storageImages = {ImageResource(target, 0, 1), ImageResource(historyDst, 0, 2)};
    exe.genericInfo.resources.sampledImages = {ImageResource(colorSrc, 0, 0), ImageResource(historySrc, 0, 3), ImageResource(currentFrame.motionBuffer, 0, 4),
                                               ImageResource(currentFrame.depthBuffer, 0, 5)};
    exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_taaResolveWeightBuffer, 6)};
    // experiment switch (profiles/r04_cross_frame_overlap.txt): the resolve as part of the frame's asynchronous tail, i.e. beside the NEXT frame's
    // exposure chain / depth pyramid / culling / trace, which read nothing it writes. Whole-frame rendering only.
    static const bool onTail = std::getenv("PLR_TAA_ON_TAIL") && std::atoi(std::getenv("PLR_TAA_ON_TAIL")) != 0;
    exe.asyncTail = onTail && !edgesDone && rows.begin == 0 && rows.end == 0xffffffffu;
    recordRows(be, exe, td.width, td.height, rows, edgeRows, edgesDone, rowsFirst, cols);
}
void TAA::computeTemporalSuperSampling(RenderBackend& be, const FrameIndexCounter& fi, const FrameRenderTargets& currentFrame, const FrameRenderTargets& lastFrame,
                                       ImageHandle target, RowRange rows) const { // TAA.cpp:85-137
    const ImageDescription td = be.getImageDescription(target);
    const size_t frameIndexMod2 = fi.mod2();
    const ImageHandle currentLuminance = m_sceneLuminance[frameIndexMod2];
    const ImageHandle historyLuminance = m_sceneLuminance[(frameIndexMod2 + 1) % 2];
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_colorToLuminancePass;
        exe.genericInfo.resources.storageImages = {ImageResource(currentLuminance, 0, 1)};
        exe.genericInfo.resources.sampledImages = {ImageResource(currentFrame.colorBuffer, 0, 0)};
        dispatch8(exe, td.width, td.height, rows);
        be.setComputePassExecution(exe);
    }
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_temporalSupersamplingPass;
        exe.genericInfo.resources.storageImages = {ImageResource(target, 0, 3)};
        exe.genericInfo.resources.sampledImages = {ImageResource(currentFrame.colorBuffer, 0, 1), ImageResource(lastFrame.colorBuffer, 0, 2), ImageResource(currentFrame.motionBuffer, 0, 4),
                                                   ImageResource(currentFrame.depthBuffer, 0, 5), ImageResource(lastFrame.depthBuffer, 0, 6), ImageResource(currentLuminance, 0, 7),
                                                   ImageResource(historyLuminance, 0, 8)};
        dispatch8(exe, td.width, td.height, rows);
        be.setComputePassExecution(exe);
    }
}
void TAA::jitterInPixels(const FrameIndexCounter& fi, float out[2]) const { // TAA.cpp:168-170
    const uint32_t i = (uint32_t)fi.mod8();
    out[0] = 2.f * radicalInverseBase2(i) - 1.f;
    out[1] = 2.f * radicalInverseBase3(i) - 1.f;
}
void TAA::updateTaaResolveWeights(RenderBackend& be, const float j[2]) { // TAA.cpp:181-202
    std::array<float, 9> weights = {};
    int index = 0;
    float totalWeight = 0.f;
    for (int y = -1; y <= 1; y++)
        for (int x = -1; x <= 1; x++) {
            const float dx = j[0] - (float)x, dy = j[1] - (float)y;
            const float d = std::sqrt(dx * dx + dy * dy);
            const float w = std::exp(-2.29f * d * d);
            weights[index++] = w;
            totalWeight += w;
        }
    for (float& w : weights) w /= totalWeight;
    be.setUniformBufferData(m_taaResolveWeightBuffer, &weights[0], sizeof(float) * 9);
}

// ------------------------------------------------------------------ Bloom (Techniques/Bloom.cpp)
static const int bloomMipCount = 6; // Bloom.cpp:6
void Bloom::init(RenderBackend& be) { // Bloom.cpp:8-40
    for (int i = 0; i < bloomMipCount - 1; i++) {
        ComputePassDescription d;
        d.name = "Bloom downsample mip " + std::to_string(i + 1);
        d.shaderDescription.srcPathRelative = "bloomDownsample.comp";
        m_bloomDownsamplePasses.push_back(be.createComputePass(d));
    }
    for (int i = 0; i < bloomMipCount - 1; i++) {
        ComputePassDescription d;
        d.name = "Bloom Upsample mip " + std::to_string(bloomMipCount - 2 - i);
        d.shaderDescription.srcPathRelative = "bloomUpsample.comp";
        const bool isLowestMip = i == 0;
        d.shaderDescription.specialisationConstants = {spec(0, isLowestMip)};
        m_bloomUpsamplePasses.push_back(be.createComputePass(d));
    }
    ComputePassDescription d;
    d.name = "Apply bloom";
    d.shaderDescription.srcPathRelative = "applyBloom.comp";
    m_applyBloomPass = be.createComputePass(d);
}
// Band rendering: which rows of every level does the bloom of `applyRows` depend on? (the dependency cone of the chain, in each level's own rows)
//   up[t] row y reads up[t+1] at y/2 + 0.25 +- 0.5 texel and down[t+1] at y/2 + 0.25 +- radius, each through a bilinear footprint
//   (bloomUpsample.comp:29-55); down[m+1] row y reads down[m] rows 2y-1 .. 2y+3 (bloomDownsample.comp:21-50; the outermost rows enter with weight 0,
//   but must hold finite values).
// Recording every level over "band +- 320 rows" (the sum of all footprints) cost a middle band 59 % extra bloom work; with the cone the full-resolution
// target has no halo at all and only the cheap coarse levels carry the wide ones.
Bloom::Cone Bloom::dependencyCone(RowRange applyRows, uint32_t height, float radius) {
    Cone c;
    if (applyRows.begin == 0 && applyRows.end == 0xffffffffu) return c; // whole image: every level whole
    auto levelRows = [&](int level) { return std::max(height >> level, 1u); };
    auto grow = [&](RowRange r, uint32_t k, int level) { return RowRange{r.begin > k ? r.begin - k : 0u, std::min(r.end + k, levelRows(level))}; };
    auto half = [](RowRange r) { return RowRange{r.begin / 2, (r.end + 1) / 2}; };
    auto twice = [](RowRange r) { return RowRange{r.begin * 2, r.end * 2}; };
    auto unite = [](RowRange a, RowRange b) { return RowRange{std::min(a.begin, b.begin), std::max(a.end, b.end)}; };
    const uint32_t tent = (uint32_t)std::ceil(radius + 0.25f) + 1u;
    c.up[0] = RowRange{std::min(applyRows.begin, height), std::min(applyRows.end, height)};
    for (int t = 0; t + 1 < bloomMipCount - 1; t++) c.up[t + 1] = grow(half(c.up[t]), 2, t + 1);
    c.down[bloomMipCount - 1] = grow(half(c.up[bloomMipCount - 2]), tent, bloomMipCount - 1);
    for (int m = bloomMipCount - 2; m >= 1; m--) c.down[m] = unite(grow(half(c.up[m - 1]), tent, m), grow(twice(c.down[m + 1]), 2, m));
    c.source = grow(twice(c.down[1]), 2, 0);
    return c;
}
uint32_t Bloom::requiredSourceHalo(uint32_t height, float radius) {
    // widest reach over bands in the middle of the image (64-row aligned begin / end do not change the cone's width)
    const uint32_t b0 = (height / 2) & ~63u, b1 = std::min(b0 + 64u, height);
    const Cone c = dependencyCone(RowRange{b0, b1}, height, radius);
    return std::max(b0 - c.source.begin, c.source.end - b1);
}

void Bloom::computeBloom(RenderBackend& be, ImageHandle targetImage, const BloomSettings& settings, RowRange chainRows, RowRange applyRows, bool asyncTail, ColRange chainCols,
                         ColRange applyCols) const { // Bloom.cpp:56-143
    const ImageDescription td = be.getImageDescription(targetImage);
    const int width = (int)td.width, height = (int)td.height;
    // chainRows = rows of the target that hold valid colour (band + exchanged halo); the chain itself only covers the dependency cone of applyRows
    const Cone cone = dependencyCone(applyRows, td.height, settings.radius);
    const bool banded = !(applyRows.begin == 0 && applyRows.end == 0xffffffffu);
    // tile rendering: the cone of the tile's columns (the footprints are the same in x and y: dependencyCone of a column range and the width)
    const Cone coneX = dependencyCone(applyCols, td.width, settings.radius);
    const bool tiled = !(applyCols.begin == 0 && applyCols.end == 0xffffffffu);
    auto levelCols = [&](ColRange coneCols, int level) {
        const ColRange valid = scaleRows(chainCols, 1u << level);
        return ColRange{std::max(coneCols.begin, valid.begin), std::min(coneCols.end, valid.end)};
    };
    // a halo smaller than the cone (BandSettings::postHalo < requiredSourceHalo): levels stop at the rows derived from valid colour, rows
    // beyond keep what an earlier frame left there (the documented limit of a too-small halo; the default halo covers the cone)
    auto levelRows = [&](RowRange coneRows, int level) {
        const RowRange valid = scaleRows(chainRows, 1u << level);
        return RowRange{std::max(coneRows.begin, valid.begin), std::min(coneRows.end, valid.end)};
    };
    const ImageDescription desc = desc2D(width, height, ImageFormat::R11G11B10_uFloat, ImageUsageFlags::Sampled | ImageUsageFlags::Storage, MipCount::Manual, bloomMipCount);
    const ImageHandle downscaleTexture = be.createTemporaryImage(desc);
    for (int i = 0; i < (int)m_bloomDownsamplePasses.size(); i++) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_bloomDownsamplePasses[i];
        const int sourceMip = i, targetMip = i + 1;
        exe.genericInfo.resources.storageImages = {ImageResource(downscaleTexture, targetMip, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(i == 0 ? targetImage : downscaleTexture, sourceMip, 1)};
        int tw, th;
        resolutionFromMip(width, height, targetMip, &tw, &th);
        dispatch8(exe, tw, th, banded ? levelRows(cone.down[targetMip], targetMip) : RowRange{}, tiled ? levelCols(coneX.down[targetMip], targetMip) : ColRange{});
        exe.asyncTail = asyncTail;
        be.setComputePassExecution(exe);
    }
    const ImageHandle upscaleTexture = be.createTemporaryImage(desc);
    for (int i = 0; i < (int)m_bloomUpsamplePasses.size(); i++) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_bloomUpsamplePasses[i];
        const int targetMip = bloomMipCount - 2 - i, sourceMip = targetMip + 1;
        exe.genericInfo.resources.storageImages = {ImageResource(upscaleTexture, targetMip, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(upscaleTexture, sourceMip, 1), ImageResource(downscaleTexture, sourceMip, 2)};
        int tw, th;
        resolutionFromMip(width, height, targetMip, &tw, &th);
        dispatch8(exe, tw, th, banded ? levelRows(cone.up[targetMip], targetMip) : RowRange{}, tiled ? levelCols(coneX.up[targetMip], targetMip) : ColRange{});
        exe.pushConstants = dataToCharArray(&settings.radius, sizeof(settings.radius));
        exe.asyncTail = asyncTail;
        be.setComputePassExecution(exe);
    }
    ComputePassExecution exe;
    exe.genericInfo.handle = m_applyBloomPass;
    exe.genericInfo.resources.storageImages = {ImageResource(targetImage, 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(upscaleTexture, 0, 1)};
    dispatch8(exe, width, height, applyRows, applyCols);
    exe.pushConstants = dataToCharArray(&settings.strength, sizeof(settings.strength));
    exe.asyncTail = asyncTail;
    be.setComputePassExecution(exe);
}

// ------------------------------------------------------------------ SDFGI (Techniques/SDFGI.cpp)
static const size_t sdfCameraCullingTileSize = 32; // SDFGI.cpp:10
static const size_t maxSdfObjectsPerTile = 100;    // SDFGI.cpp:11
static const size_t sdfInstanceSize = 96;          // sizeof(SDFInstance), SDFGI.h:31-37

// the reference sizes the culled-tile buffer for 1920x1080 only (SDFGI.cpp:145-151); sized here for the tile-index range the shaders
// produce: stride = ceil(screenW / 32) (full-res, sdfCulling.inc:17-20) times the trace image's tile rows
static size_t culledTilesBytes(int screenW, int screenH, uint32_t th) {
    const size_t strideX = (size_t)std::ceil(screenW / float(sdfCameraCullingTileSize));
    // (the debug visualisation culls at full resolution, SDFGI.cpp:340-350: rows for the full screen height)
    const size_t rows = (size_t)std::ceil(std::max<uint32_t>(th, (uint32_t)screenH) / float(sdfCameraCullingTileSize));
    const size_t tileSize = maxSdfObjectsPerTile * sizeof(uint32_t) + sizeof(uint32_t);
    return strideX * std::max<size_t>(rows, 1) * tileSize;
}
static ShaderDescription sdfDebugShaderDescription(const SDFDebugSettings& ds, int sunShadowCascadeIndex) { // createSDFDebugShaderDescription, SDFGI.cpp:13-28
    ShaderDescription d;
    d.srcPathRelative = "sdfDebugVisualisation.comp";
    d.specialisationConstants = {spec(0, ds.visualisationMode), spec(1, sunShadowCascadeIndex)};
    return d;
}
static ShaderDescription sdfDiffuseTraceShaderDescription(const SDFTraceSettings& ts, int sunShadowCascadeIndex) { // createSDFDiffuseTraceShaderDescription, SDFGI.cpp:30-46
    ShaderDescription d;
    d.srcPathRelative = "sdfDiffuseTrace.comp";
    d.specialisationConstants = {spec(0, ts.strictInfluenceRadiusCutoff), spec(1, sunShadowCascadeIndex)};
    return d;
}

void SDFGI::init(RenderBackend& be, int screenW, int screenH, const SDFTraceSettings& ts, const SDFDebugSettings& ds, int sunShadowCascadeIndex, uint32_t maxInstances) { // SDFGI.cpp:48-258
    const uint32_t tw = ts.halfResTrace ? screenW / 2 : screenW, th = ts.halfResTrace ? screenH / 2 : screenH;
    for (int i = 0; i < 2; i++) {
        m_indirectDiffuse_Y_SH[i] = be.createImage(desc2D(tw, th, ImageFormat::RGBA16_sFloat), nullptr, 0);
        m_indirectDiffuse_CoCg[i] = be.createImage(desc2D(tw, th, ImageFormat::RG16_sFloat), nullptr, 0);
        m_indirectDiffuseHistory_Y_SH[i] = be.createImage(desc2D(tw, th, ImageFormat::RGBA16_sFloat), nullptr, 0);
        m_indirectDiffuseHistory_CoCg[i] = be.createImage(desc2D(tw, th, ImageFormat::RG16_sFloat), nullptr, 0);
    }
    m_indirectLightingFullRes_Y_SH = be.createImage(desc2D(screenW, screenH, ImageFormat::RGBA16_sFloat), nullptr, 0);
    m_indirectLightingFullRes_CoCg = be.createImage(desc2D(screenW, screenH, ImageFormat::RG16_sFloat), nullptr, 0);
    StorageBufferDescription sb;
    sb.size = maxInstances * sdfInstanceSize + sizeof(uint32_t) * 4;
    m_sdfInstanceBuffer = be.createStorageBuffer(sb);
    sb.size = maxInstances * sizeof(uint32_t) + sizeof(uint32_t);
    m_sdfCameraFrustumCulledInstances = be.createStorageBuffer(sb);
    UniformBufferDescription ub;
    ub.size = 12 * 4 * sizeof(float);
    m_cameraFrustumBuffer = be.createUniformBuffer(ub);
    sb.size = maxInstances * 2 * 4 * sizeof(float);
    m_sdfInstanceWorldBBBuffer = be.createStorageBuffer(sb);
    sb.size = culledTilesBytes(screenW, screenH, th);
    m_sdfCameraCulledTiles = be.createStorageBuffer(sb);
    ub.size = sizeof(float);
    m_sdfTraceInfluenceRangeBuffer = be.createUniformBuffer(ub);
    {
        ComputePassDescription d;
        d.name = "Visualize SDF";
        d.shaderDescription = sdfDebugShaderDescription(ds, sunShadowCascadeIndex);
        m_sdfDebugVisualisationPass = be.createComputePass(d);
    }
    {
        ComputePassDescription d;
        d.name = "Indirect diffuse SDF trace";
        d.shaderDescription = sdfDiffuseTraceShaderDescription(ts, sunShadowCascadeIndex);
        m_diffuseSDFTracePass = be.createComputePass(d);
    }
    for (int i = 0; i < 2; i++) {
        // the request-list exchange of a partitioned frame (GiBand::requested; no reference counterpart): which texels outside this GPU's rectangle do the disc samples
        // of spatial filter pass i land on?
        ComputePassDescription d;
        d.name = i == 0 ? "Indirect diffuse sample requests (filter 0)" : "Indirect diffuse sample requests (filter 1)";
        d.shaderDescription.srcPathRelative = "giSampleRequests.comp";
        d.shaderDescription.specialisationConstants = {spec(0, i)};
        m_giSampleRequestPass[i] = be.createComputePass(d);
        m_giRequestRowWords = (tw + 31u) / 32u;
        StorageBufferDescription rb;
        rb.size = (size_t)m_giRequestRowWords * th * sizeof(uint32_t);
        m_giRequestBitmap[i] = be.createStorageBuffer(rb);
    }
    for (int i = 0; i < 2; i++) {
        ComputePassDescription d;
        d.name = "Indirect diffuse spatial filter";
        d.shaderDescription.srcPathRelative = "filterIndirectDiffuseSpatial.comp";
        d.shaderDescription.specialisationConstants = {spec(0, i)};
        m_indirectDiffuseFilterSpatialPass[i] = be.createComputePass(d);
    }
    {
        ComputePassDescription d;
        d.name = "Indirect diffuse temporal filter";
        d.shaderDescription.srcPathRelative = "filterIndirectDiffuseTemporal.comp";
        m_indirectDiffuseFilterTemporalPass = be.createComputePass(d);
        d.name = "Indirect lighting upscale";
        d.shaderDescription.srcPathRelative = "indirectLightUpscale.comp";
        m_indirectLightingUpscale = be.createComputePass(d);
        d.name = "SDF camera frustum culling";
        d.shaderDescription.srcPathRelative = "sdfCameraFrustumCulling.comp";
        m_sdfCameraFrustumCulling = be.createComputePass(d);
    }
    for (int hiz = 0; hiz < 2; hiz++) {
        ComputePassDescription d;
        d.name = "SDF camera tile culling";
        d.shaderDescription.srcPathRelative = "sdfCameraTileCulling.comp";
        const bool useHiZ = hiz == 1;
        d.shaderDescription.specialisationConstants = {spec(0, useHiZ)};
        (useHiZ ? m_sdfCameraTileCullingHiZ : m_sdfCameraTileCulling) = be.createComputePass(d);
    }
}

void SDFGI::resize(RenderBackend& be, int screenW, int screenH, const SDFTraceSettings& ts) { // SDFGI.cpp:237-258
    const uint32_t tw = ts.halfResTrace ? screenW / 2 : screenW, th = ts.halfResTrace ? screenH / 2 : screenH;
    be.resizeImages({m_indirectDiffuse_Y_SH[0], m_indirectDiffuse_Y_SH[1], m_indirectDiffuse_CoCg[0], m_indirectDiffuse_CoCg[1], m_indirectDiffuseHistory_Y_SH[0],
                     m_indirectDiffuseHistory_Y_SH[1], m_indirectDiffuseHistory_CoCg[0], m_indirectDiffuseHistory_CoCg[1]}, tw, th);
    be.resizeImages({m_indirectLightingFullRes_Y_SH, m_indirectLightingFullRes_CoCg}, screenW, screenH);
    be.resizeStorageBuffer(m_sdfCameraCulledTiles, culledTilesBytes(screenW, screenH, th));
    m_giRequestRowWords = (tw + 31u) / 32u;
    for (int i = 0; i < 2; i++) be.resizeStorageBuffer(m_giRequestBitmap[i], (size_t)m_giRequestRowWords * th * sizeof(uint32_t));
}
void SDFGI::updateSettings(RenderBackend& be, const SDFTraceSettings& ts, const SDFDebugSettings& ds, int sunShadowCascadeIndex) { // SDFGI.cpp:371-378
    be.updateComputePassShaderDescription(m_sdfDebugVisualisationPass, sdfDebugShaderDescription(ds, sunShadowCascadeIndex));
    be.updateComputePassShaderDescription(m_diffuseSDFTracePass, sdfDiffuseTraceShaderDescription(ts, sunShadowCascadeIndex));
}

void SDFGI::updateSDFScene(RenderBackend& be, const void* instanceData, size_t instanceBytes, const void* bbData, size_t bbBytes) { // SDFGI.cpp:260-313
    if (instanceBytes >= 4) std::memcpy(&m_sdfInstanceCount, instanceData, 4);
    be.setStorageBufferData(m_sdfInstanceBuffer, instanceData, instanceBytes);
    be.setStorageBufferData(m_sdfInstanceWorldBBBuffer, bbData, bbBytes);
}

SDFGI::IndirectLightingImages SDFGI::getIndirectLightingResults(bool tracedHalfRes) const { // SDFGI.cpp:315-326
    if (tracedHalfRes) return {m_indirectLightingFullRes_Y_SH, m_indirectLightingFullRes_CoCg};
    return {m_indirectDiffuseHistory_Y_SH[0], m_indirectDiffuseHistory_CoCg[0]};
}

void SDFGI::sampleRequests(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const {
    // recorded like the spatial filter executions they precede: the same rectangle; what is "valid" is the rectangle itself, every sample beyond it is a request
    const ImageDescription td = be.getImageDescription(m_indirectDiffuse_Y_SH[1]);
    for (int i = 0; i < 2; i++) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_giSampleRequestPass[i];
        exe.genericInfo.resources.sampledImages = {ImageResource(s.halfResTrace ? deps.depthHalfRes : deps.currentFrame.depthBuffer, 0, 4)};
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_giRequestBitmap[i], false, 6)};
        dispatch8(exe, td.width, td.height, band->traceRows, band->traceCols);
        exe.validRows[0] = std::min(band->traceRows.begin, td.height); exe.validRows[1] = std::min(band->traceRows.end, td.height);
        const uint32_t c0 = std::min(band->traceCols.begin, td.width), c1 = std::min(band->traceCols.end, td.width);
        if (c0 > 0 || c1 < td.width) { exe.validCols[0] = c0; exe.validCols[1] = c1; }
        be.setComputePassExecution(exe);
    }
}

void SDFGI::computeIndirectLighting(RenderBackend& be, const FrameIndexCounter&, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const {
    if (band && band->requested) {
        // where the two spatial filter passes' samples land depends on depth, camera and frame index only: asked for now, traded while the trace runs
        sampleRequests(be, deps, s, band);
        band->exchangePoint(band->user, ExchangeGiRequests);
    }
    diffuseSDFTrace(be, deps, s, band);
    filterIndirectDiffuse(be, deps, s, band);
}

void SDFGI::renderSDFVisualization(RenderBackend& be, ImageHandle target, const SDFTraceDependencies& deps, const SDFDebugSettings& ds, const SDFTraceSettings& ts) const {
    // SDFGI.cpp:334-369
    const float sdfInfluenceRadius = ds.useInfluenceRadiusForDebug ? ts.traceInfluenceRadius : 0.f;
    const ImageDescription td = be.getImageDescription(m_indirectLightingFullRes_CoCg);
    const bool useHiZCulling = ds.visualisationMode == SDFVisualisationMode::CameraTileUsage && ds.showCameraTileUsageWithHiZ;
    sdfInstanceCulling(be, deps, (int)td.width, (int)td.height, sdfInfluenceRadius, useHiZCulling, nullptr);
    ComputePassExecution exe;
    exe.genericInfo.handle = m_sdfDebugVisualisationPass;
    exe.genericInfo.resources.storageImages = {ImageResource(target, 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(deps.skyLut, 0, 2), ImageResource(deps.shadowMap, 0, 7)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(deps.lightBuffer, true, 1), StorageBufferResource(m_sdfInstanceBuffer, true, 3),
                                                StorageBufferResource(m_sdfCameraCulledTiles, true, 4), StorageBufferResource(m_sdfCameraFrustumCulledInstances, true, 5),
                                                StorageBufferResource(deps.sunShadowInfoBuffer, true, 6)};
    dispatch8(exe, td.width, td.height);
    be.setComputePassExecution(exe);
}

void SDFGI::sdfInstanceCulling(RenderBackend& be, const SDFTraceDependencies& deps, int targetW, int targetH, float influenceRadius, bool hiZCulling, const GiBand* band) const {
    // SDFGI.cpp:538-630
    {
        struct GPUFrustumData { float points[6][4]; float normal[6][4]; } frustumData;
        std::memcpy(frustumData.points, deps.frustumPoints, sizeof(frustumData.points));
        std::memcpy(frustumData.normal, deps.frustumNormals, sizeof(frustumData.normal));
        be.setUniformBufferData(m_cameraFrustumBuffer, &frustumData, sizeof(frustumData));
        uint32_t zero = 0;
        be.setStorageBufferData(m_sdfCameraFrustumCulledInstances, &zero, sizeof(zero));
        ComputePassExecution exe;
        exe.genericInfo.handle = m_sdfCameraFrustumCulling;
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sdfInstanceBuffer, true, 0), StorageBufferResource(m_sdfCameraFrustumCulledInstances, false, 2),
                                                    StorageBufferResource(m_sdfInstanceWorldBBBuffer, true, 3)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_cameraFrustumBuffer, 1), UniformBufferResource(m_sdfTraceInfluenceRangeBuffer, 4)};
        exe.dispatchCount[0] = uint32_t(std::ceil(m_sdfInstanceCount / 64.f));
        exe.dispatchCount[1] = 1;
        exe.dispatchCount[2] = 1;
        be.setComputePassExecution(exe);
    }
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = hiZCulling ? m_sdfCameraTileCullingHiZ : m_sdfCameraTileCulling;
        const uint32_t tileCount[2] = {(uint32_t)std::ceil(targetW / float(sdfCameraCullingTileSize)), (uint32_t)std::ceil(targetH / float(sdfCameraCullingTileSize))};
        const uint32_t localGroupSize = 8;
        exe.dispatchCount[0] = uint32_t(std::ceil(tileCount[0] / float(localGroupSize)));
        exe.dispatchCount[1] = uint32_t(std::ceil(tileCount[1] / float(localGroupSize)));
        exe.dispatchCount[2] = 1;
        if (band) { // only the workgroups (8 tile rows each) that hold tiles of the band's trace rows
            const uint32_t tileRows = (uint32_t)sdfCameraCullingTileSize * localGroupSize;
            const uint32_t lo = std::min(band->traceRows.begin, (uint32_t)targetH), hi = std::min(band->traceRows.end, (uint32_t)targetH);
            exe.dispatchBase[1] = lo / tileRows;
            exe.dispatchCount[1] = hi > lo ? (hi + tileRows - 1) / tileRows - lo / tileRows : 0;
            // tile rendering: and the workgroups (8 tile columns each) that hold tiles of the tile's trace columns
            const uint32_t cl = std::min(band->traceCols.begin, (uint32_t)targetW), ch = std::min(band->traceCols.end, (uint32_t)targetW);
            exe.dispatchBase[0] = cl / tileRows;
            exe.dispatchCount[0] = ch > cl ? (ch + tileRows - 1) / tileRows - cl / tileRows : 0;
        }
        exe.pushConstants = dataToCharArray(&tileCount, sizeof(tileCount));
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sdfCameraFrustumCulledInstances, true, 0), StorageBufferResource(m_sdfInstanceWorldBBBuffer, true, 1),
                                                    StorageBufferResource(m_sdfCameraCulledTiles, false, 2)};
        be.setUniformBufferData(m_sdfTraceInfluenceRangeBuffer, &influenceRadius, sizeof(influenceRadius));
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_sdfTraceInfluenceRangeBuffer, 3)};
        const int depthPyramidMipLevel = (int)std::log2(std::ceil(float(sdfCameraCullingTileSize))) - 1; // = 4
        exe.genericInfo.resources.sampledImages = {ImageResource(deps.depthMinMaxPyramid, depthPyramidMipLevel, 4)};
        be.setComputePassExecution(exe);
    }
}

void SDFGI::diffuseSDFTrace(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const { // SDFGI.cpp:380-419
    const ImageDescription td = be.getImageDescription(m_indirectDiffuse_CoCg[0]);
    sdfInstanceCulling(be, deps, td.width, td.height, s.traceInfluenceRadius, true, band);
    ComputePassExecution exe;
    exe.genericInfo.handle = m_diffuseSDFTracePass;
    exe.genericInfo.resources.storageImages = {ImageResource(m_indirectDiffuse_Y_SH[0], 0, 0), ImageResource(m_indirectDiffuse_CoCg[0], 0, 1)};
    exe.genericInfo.resources.sampledImages = {ImageResource(deps.currentFrame.depthBuffer, 0, 2), ImageResource(deps.worldSpaceNormals, 0, 3), ImageResource(deps.skyLut, 0, 4),
                                               ImageResource(deps.shadowMap, 0, 10)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(deps.lightBuffer, true, 5), StorageBufferResource(m_sdfInstanceBuffer, true, 6),
                                                StorageBufferResource(m_sdfCameraCulledTiles, true, 7), StorageBufferResource(deps.sunShadowInfoBuffer, true, 9)};
    exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_sdfTraceInfluenceRangeBuffer, 8)};
    if (band && band->requested && band->requestedBegin) {
        recordRows(be, exe, td.width, td.height, band->traceRows, 0, nullptr, false, band->traceCols);
        band->requestedBegin(band->user, ExchangeGiTrace); // the owners gather what was asked of them as soon as their trace is done
        return;
    }
    if (band && band->exchangeBegin)
        recordRows(be, exe, td.width, td.height, band->traceRows, band->giHalo, [&] { band->exchangeBegin(band->user, ExchangeGiTrace); }, band->rowsFirst, band->traceCols);
    else recordRows(be, exe, td.width, td.height, band ? band->traceRows : RowRange{}, 0, nullptr, false, band ? band->traceCols : ColRange{});
    if (band && band->exchangePoint) band->exchangePoint(band->user, ExchangeGiTrace); // spatial pass 0 reads neighbouring bands' rays
}

void SDFGI::filterIndirectDiffuse(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const { // SDFGI.cpp:421-536
    const ImageHandle depthSrc = s.halfResTrace ? deps.depthHalfRes : deps.currentFrame.depthBuffer;
    const ImageDescription td = be.getImageDescription(m_indirectDiffuse_Y_SH[1]);
    const RowRange rows = band ? band->traceRows : RowRange{};
    const ColRange cols = band ? band->traceCols : ColRange{};
    // band rendering: the spatial filter's inputs are valid on the band's rows and the giHalo rows received from each neighbour; a disc sample
    // beyond them is treated like an off-screen sample (ComputePassExecution::validRows, plr.h) instead of reading rows nobody sent
    // a spatial filter execution; with request lists + overlap: the waves that need no requested texel, the wait for the exchange, the others (push constant: the phase)
    auto recordSpatial = [&](ComputePassExecution& exe, int exchangeId) {
        if (band && band->requested && band->requestedEnd) {
            const int32_t phase1 = 1, phase2 = 2;
            exe.pushConstants = dataToCharArray(&phase1, sizeof(phase1));
            be.setComputePassExecution(exe);
            band->requestedEnd(band->user, exchangeId);
            exe.pushConstants = dataToCharArray(&phase2, sizeof(phase2));
            be.setComputePassExecution(exe);
            return;
        }
        be.setComputePassExecution(exe);
    };
    auto setValidRows = [&](ComputePassExecution& exe, int filterIndex) {
        if (!band) return;
        if (band->requested) { // every texel a sample can land on is either this rectangle's or has been requested and received: nothing is masked (plr.h: {0, 0} = all valid)
            exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_giRequestBitmap[filterIndex], true, 6));
            return;
        }
        const uint32_t r0 = std::min(rows.begin, td.height), r1 = std::min(rows.end, td.height);
        exe.validRows[0] = r0 > band->giHalo ? r0 - band->giHalo : 0u;
        exe.validRows[1] = std::min(r1 + band->giHalo, td.height);
        // tile rendering: the same for the columns (plr.h valid_cols)
        const uint32_t c0 = std::min(cols.begin, td.width), c1 = std::min(cols.end, td.width);
        if (c0 > 0 || c1 < td.width) {
            exe.validCols[0] = c0 > band->giHalo ? c0 - band->giHalo : 0u;
            exe.validCols[1] = std::min(c1 + band->giHalo, td.width);
        }
    };
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_indirectDiffuseFilterSpatialPass[0];
        exe.genericInfo.resources.storageImages = {ImageResource(m_indirectDiffuse_Y_SH[1], 0, 0), ImageResource(m_indirectDiffuse_CoCg[1], 0, 1)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_indirectDiffuse_Y_SH[0], 0, 2), ImageResource(m_indirectDiffuse_CoCg[0], 0, 3), ImageResource(depthSrc, 0, 4),
                                                   ImageResource(deps.worldSpaceNormals, 0, 5)};
        dispatch8(exe, td.width, td.height, rows, cols);
        setValidRows(exe, 0);
        recordSpatial(exe, ExchangeGiTrace);
    }
    {
        // always History[0] -> History[1]; the reference computes historySrc/DstIndex but never uses them (SDFGI.cpp:457-458)
        ComputePassExecution exe;
        exe.genericInfo.handle = m_indirectDiffuseFilterTemporalPass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_indirectDiffuse_Y_SH[0], 0, 0), ImageResource(m_indirectDiffuse_CoCg[0], 0, 1),
                                                   ImageResource(m_indirectDiffuseHistory_Y_SH[1], 0, 2), ImageResource(m_indirectDiffuseHistory_CoCg[1], 0, 3)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_indirectDiffuse_Y_SH[1], 0, 4), ImageResource(m_indirectDiffuse_CoCg[1], 0, 5),
                                                   ImageResource(m_indirectDiffuseHistory_Y_SH[0], 0, 6), ImageResource(m_indirectDiffuseHistory_CoCg[0], 0, 7),
                                                   ImageResource(deps.currentFrame.motionBuffer, 0, 8), ImageResource(deps.previousFrame.motionBuffer, 0, 9)};
        if (band && band->requested && band->requestedBegin) { recordRows(be, exe, td.width, td.height, rows, 0, nullptr, false, cols); band->requestedBegin(band->user, ExchangeGiTemporal); }
        else if (band && band->exchangeBegin) recordRows(be, exe, td.width, td.height, rows, band->giHalo, [&] { band->exchangeBegin(band->user, ExchangeGiTemporal); }, band->rowsFirst, cols);
        else recordRows(be, exe, td.width, td.height, rows, 0, nullptr, false, cols);
    }
    if (band && band->exchangePoint && !(band->requested && band->requestedBegin)) band->exchangePoint(band->user, ExchangeGiTemporal); // spatial pass 1 reads neighbouring rows of History[1]
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_indirectDiffuseFilterSpatialPass[1];
        exe.genericInfo.resources.storageImages = {ImageResource(m_indirectDiffuseHistory_Y_SH[0], 0, 0), ImageResource(m_indirectDiffuseHistory_CoCg[0], 0, 1)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_indirectDiffuseHistory_Y_SH[1], 0, 2), ImageResource(m_indirectDiffuseHistory_CoCg[1], 0, 3),
                                                   ImageResource(depthSrc, 0, 4), ImageResource(deps.worldSpaceNormals, 0, 5)};
        setValidRows(exe, 1);
        dispatch8(exe, td.width, td.height, rows, cols);
        recordSpatial(exe, ExchangeGiTemporal);
    }
    // (this exchange is small - 16 rows - and its producer launches a packing pre-pass per dispatch: it is not split / overlapped)
    if (band && band->exchangeWhole) band->exchangeWhole(band->user, ExchangeGiHistory);
    else if (band && band->exchangePoint) band->exchangePoint(band->user, ExchangeGiHistory); // upscale + next frame's reprojection read History[0]
    if (s.halfResTrace) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_indirectLightingUpscale;
        exe.genericInfo.resources.storageImages = {ImageResource(m_indirectLightingFullRes_Y_SH, 0, 0), ImageResource(m_indirectLightingFullRes_CoCg, 0, 1)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_indirectDiffuseHistory_Y_SH[0], 0, 2), ImageResource(m_indirectDiffuseHistory_CoCg[0], 0, 3),
                                                   ImageResource(deps.currentFrame.depthBuffer, 0, 4), ImageResource(deps.depthHalfRes, 0, 5)};
        const ImageDescription fd = be.getImageDescription(m_indirectLightingFullRes_Y_SH);
        dispatch8(exe, fd.width, fd.height, band ? band->upscaleRows : RowRange{}, band ? band->upscaleCols : ColRange{});
        be.setComputePassExecution(exe);
    }
}

// ------------------------------------------------------------------ FramePipeline (RenderFrontend.cpp)
static const uint32_t nHistogramBins = 128;       // RenderFrontend.cpp:46
static const uint32_t histogramTileSizeX = 32, histogramTileSizeY = 32;
static const float histogramMinValue = 0.001f, histogramMaxValue = 200000.f; // RenderFrontend.cpp:1066-1067
static const uint32_t noiseTextureWidth = 32, noiseTextureHeight = 32;       // RenderFrontend.cpp:52-54
static const int maxSunShadowCascadeCount = 4;

// RenderFrontend::computeSinglePassMipChainDispatchCount, RenderFrontend.cpp:1807-1827
static void singlePassMipChainDispatchCount(uint32_t width, uint32_t height, uint32_t mipCount, uint32_t maxMipCount, uint32_t out[2]) {
    const uint32_t unusedMips = maxMipCount - mipCount;
    if (unusedMips >= 6) { out[0] = out[1] = 1; return; }
    const uint32_t localThreadGroupExtent = 32 / (uint32_t)std::pow((uint32_t)2, unusedMips);
    out[0] = (uint32_t)std::ceil(float(width) / localThreadGroupExtent);
    out[1] = (uint32_t)std::ceil(float(height) / localThreadGroupExtent);
}

static const uint32_t bandAlignment = 64;      // HiZ tile (64 px), culling tile (32 trace px), histogram tile (32 px), 2^5 bloom texel
static const uint32_t bandPyramidMipCount = 6; // per-tile levels of the HiZ kernel; the hot path reads mip 4 (SDFGI.cpp:567)
static const uint32_t maxPyramidMipCount = 11; // depthHiZPyramid.comp binds at most 11 levels (pyramid base <= 2048)
// A band builds only the levels one 64x64-pixel tile yields: the rest of the chain needs every band and has no consumer on this path.
// A frame whose full chain would exceed the shader's 11 levels (8K un-tiled; the reference cannot render it) gets the same per-tile pyramid.
static bool perTilePyramid(const FramePipelineSettings& s) { return s.band.enabled() || mipCountFromResolution(s.width / 2, s.height / 2, 1) > maxPyramidMipCount; }
static uint32_t pyramidMipCount(const FramePipelineSettings& s) { return perTilePyramid(s) ? bandPyramidMipCount : mipCountFromResolution(s.width / 2, s.height / 2, 1); }

// createForwardPassShaderDescription, RenderFrontend.cpp:1093-1131, as the deferred compute pass
static ShaderDescription forwardPassShaderDescription(const ShadingConfig& c) {
    ShaderDescription d;
    d.srcPathRelative = "deferredShading.comp";
    d.specialisationConstants = {spec(0, c.diffuseBRDF), spec(1, c.directMultiscatter), spec(2, c.useGeometryAA), spec(3, c.indirectLightingTech), spec(4, c.sunShadowCascadeCount)};
    return d;
}
static ShaderDescription brdfLutShaderDescription(const ShadingConfig& c) { // createBRDFLutShaderDescription
    ShaderDescription d;
    d.srcPathRelative = "brdfLut.comp";
    d.specialisationConstants = {spec(0, c.diffuseBRDF)};
    return d;
}
// createDepthPyramidShaderDescription, RenderFrontend.cpp:1770-1805; sets m_depthPyramidThreadgroupCount
ShaderDescription FramePipeline::depthPyramidShaderDescription() {
    const uint32_t W = settings.width, H = settings.height;
    ShaderDescription d;
    d.srcPathRelative = "depthHiZPyramid.comp";
    const uint32_t pw = W / 2, ph = H / 2;
    const uint32_t depthMipCount = pyramidMipCount(settings);
    uint32_t dc[2];
    singlePassMipChainDispatchCount(pw, ph, depthMipCount, 11, dc);
    m_depthPyramidThreadgroupCount = dc[0] * dc[1];
    d.specialisationConstants = {spec(0, depthMipCount), spec(1, W), spec(2, H), spec(3, m_depthPyramidThreadgroupCount)};
    return d;
}
static ImageDescription depthPyramidDescription(const FramePipelineSettings& s) {
    return perTilePyramid(s)
        ? desc2D(s.width / 2, s.height / 2, ImageFormat::RG32_sFloat, ImageUsageFlags::Storage | ImageUsageFlags::Sampled, MipCount::Manual, bandPyramidMipCount)
        : desc2D(s.width / 2, s.height / 2, ImageFormat::RG32_sFloat, ImageUsageFlags::Storage | ImageUsageFlags::Sampled, MipCount::FullChain);
}
static uint32_t histogramTileCount(uint32_t W, uint32_t H) { return (uint32_t)std::ceil(W / float(histogramTileSizeX)) * (uint32_t)std::ceil(H / float(histogramTileSizeY)); }
static ShaderDescription histogramPerTileShaderDescription(uint32_t W, uint32_t H) {
    ShaderDescription d;
    d.srcPathRelative = "histogramPerTile.comp";
    d.specialisationConstants = {spec(0, nHistogramBins), spec(1, histogramMinValue), spec(2, histogramMaxValue), spec(3, (int)histogramTileCount(W, H))};
    return d;
}
static ShaderDescription histogramCombineShaderDescription(uint32_t W, uint32_t H) {
    ShaderDescription d;
    d.srcPathRelative = "histogramCombineTiles.comp";
    d.specialisationConstants = {spec(0, nHistogramBins), spec(1, (int)histogramTileCount(W, H))};
    return d;
}

FramePipeline::FramePipeline(const FramePipelineSettings& s) : settings(s), m_requestedSettings(s), m_targetWidth(s.width), m_targetHeight(s.height) {
    const uint32_t W = s.width, H = s.height;
    if (s.band.enabled()) {
        const BandSettings& b = s.band;
        if (b.rowEnd > H || b.rowBegin % bandAlignment != 0 || (b.rowEnd % bandAlignment != 0 && b.rowEnd != H))
            throw std::runtime_error("band rows must lie inside the frame and start/end on multiples of 64 (or at the last row)");
        if (b.tiled() && (b.colEnd > W || b.colBegin % bandAlignment != 0 || (b.colEnd % bandAlignment != 0 && b.colEnd != W)))
            throw std::runtime_error("tile columns must lie inside the frame and start/end on multiples of 64 (or at the last column)");
    } else if (s.band.tiled()) throw std::runtime_error("tile columns without band rows: set rowBegin / rowEnd too");
    if (s.runSky && !s.runShading) throw std::runtime_error("run_sky needs run_shading: the sky pass completes the colour buffer the deferred shade writes");
    // a halo never needs to be larger than the image (PLRF_HALO_WHOLE_IMAGE: the exact mode of a partitioned frame, every GI texel a denoiser sample can
    // reach is exchanged); clamping here keeps the row arithmetic below in 32 bits
    if (settings.band.giHalo == 0xfffffffeu) { // PLRF_HALO_REQUESTED
        if (!s.sdfTrace.halfResTrace) throw std::runtime_error("band_gi_halo = PLRF_HALO_REQUESTED needs the half-resolution trace (the packed-texel spatial filter)");
        settings.band.giRequested = true;
        settings.band.giHalo = 0;
    }
    settings.band.giHalo = std::min(settings.band.giHalo, std::max(W, H));
    settings.band.giHistoryHalo = std::min(settings.band.giHistoryHalo, std::max(W, H));
    for (int i = 0; i < ExchangeCount; i++) {
        m_exchangeCtx[i] = {this, i};
        m_exchangeCtx[ExchangeCount + i] = {this, i | ExchangeBegin};
        m_exchangeCtx[2 * ExchangeCount + i] = {this, i | ExchangeEnd};
    }
    // the backend is set up by the caller (plr_setup), like gRenderBackend.setup in the reference's main(); match the swapchain
    const ImageDescription sw = m_be.getImageDescription(m_be.getSwapchainInputImage());
    if (sw.width != W || sw.height != H) m_be.recreateSwapchain(W, H);
    m_cameraIntrinsic.aspectRatio = (float)W / (float)H;

    // ---- initBuffers (RenderFrontend.cpp:1449-1500)
    StorageBufferDescription sb;
    sb.size = nHistogramBins * sizeof(uint32_t);
    m_histogramBuffer = m_be.createStorageBuffer(sb);
    float lightInit[5] = {0, 0, 0, 0, 0};
    sb.size = sizeof(lightInit); sb.initialData = lightInit;
    m_lightBuffer = m_be.createStorageBuffer(sb);
    sb.initialData = nullptr;
    const uint32_t tileCount = histogramTileCount(W, H);
    sb.size = (size_t)tileCount * nHistogramBins * sizeof(uint32_t); // the reference allocates for 1920x1080 only (:1069-1070)
    m_histogramPerTileBuffer = m_be.createStorageBuffer(sb);
    sb.size = sizeof(uint32_t);
    m_depthPyramidSyncBuffer = m_be.createStorageBuffer(sb);
    sb.size = 16 + 64 * maxSunShadowCascadeCount + 8 * maxSunShadowCascadeCount;
    m_sunShadowInfoBuffer = m_be.createStorageBuffer(sb);
    UniformBufferDescription ub;
    ub.size = sizeof(GlobalShaderInfo);
    m_globalUniformBuffer = m_be.createUniformBuffer(ub);
    ub.size = 64;
    m_volumetricsInfoBuffer = m_be.createUniformBuffer(ub);
    RenderPassResources globalResources;
    globalResources.uniformBuffers = {UniformBufferResource(m_globalUniformBuffer, 0)};
    m_be.setGlobalDescriptorSetResources(globalResources);

    // ---- initImages (RenderFrontend.cpp:1186-1447): G-buffer + colour targets, two sets
    for (int i = 0; i < 2; i++) {
        m_postProcessBuffers[i] = m_be.createImage(desc2D(W, H, ImageFormat::R11G11B10_uFloat), nullptr, 0);
        m_frameRenderTargets[i].colorBuffer = m_be.createImage(desc2D(W, H, ImageFormat::R11G11B10_uFloat), nullptr, 0);
        m_frameRenderTargets[i].motionBuffer = m_be.createImage(desc2D(W, H, ImageFormat::RG16_sNorm), nullptr, 0);
        m_frameRenderTargets[i].depthBuffer = m_be.createImage(desc2D(W, H, ImageFormat::Depth32), nullptr, 0);
    }
    m_worldSpaceNormalImage = m_be.createImage(desc2D(W, H, ImageFormat::RGBA8), nullptr, 0);
    m_albedoImage = m_be.createImage(desc2D(W, H, ImageFormat::RGBA8), nullptr, 0);
    m_specularImage = m_be.createImage(desc2D(W, H, ImageFormat::RGBA8), nullptr, 0);
    m_minMaxDepthPyramid = m_be.createImage(depthPyramidDescription(s), nullptr, 0);
    // band rendering: the depth range of the whole frame (lightMatrix.comp's "lowest mip"), reduced from the band's per-tile pyramids and all-reduced
    m_bandDepthApex = m_be.createImage(desc2D(1, 1, ImageFormat::RG32_sFloat), nullptr, 0);
    m_depthHalfRes = m_be.createImage(desc2D(W / 2, H / 2, ImageFormat::R16_sFloat), nullptr, 0);
    m_brdfLut = m_be.createImage(desc2D(s.brdfLutRes, s.brdfLutRes, ImageFormat::RGBA16_sFloat), nullptr, 0);
    m_skyLut = m_be.createImage(desc2D(200, 100, ImageFormat::R11G11B10_uFloat), nullptr, 0);          // Sky.cpp sky LUT
    m_transmissionLut = m_be.createImage(desc2D(128, 128, ImageFormat::R11G11B10_uFloat), nullptr, 0); // Sky.cpp transmission LUT
    {
        ImageDescription d; // Volumetrics.cpp:8-16
        d.width = (uint32_t)std::ceil(W / 8.f); d.height = (uint32_t)std::ceil(H / 8.f); d.depth = s.froxelDepth;
        d.type = ImageType::Type3D; d.format = ImageFormat::RGBA16_sFloat; d.usageFlags = ImageUsageFlags::Storage | ImageUsageFlags::Sampled;
        m_volumetricIntegrationVolume = m_be.createImage(d, nullptr, 0);
    }
    for (int i = 0; i < maxSunShadowCascadeCount; i++)
        m_shadowMaps[i] = m_be.createImage(desc2D(s.shadowMapRes, s.shadowMapRes, ImageFormat::Depth16, ImageUsageFlags::Storage | ImageUsageFlags::Sampled), nullptr, 0); // (storage: sunShadowRaster.comp writes them while casters are set)
    for (int i = 0; i < 4; i++) {
        m_noiseTextures[i] = m_be.createImage(desc2D(noiseTextureWidth, noiseTextureHeight, ImageFormat::RG8, ImageUsageFlags::Sampled), nullptr, 0);
        m_globalShaderInfo.noiseTextureIndices[i] = (int32_t)m_be.getImageGlobalTextureArrayIndex(m_noiseTextures[i]);
    }

    // ---- initRenderpasses (RenderFrontend.cpp:1618-1760)
    {
        ComputePassDescription d;
        d.name = "Histogram per tile";
        d.shaderDescription = histogramPerTileShaderDescription(W, H);
        m_histogramPerTilePass = m_be.createComputePass(d);
        d.name = "Histogram reset";
        d.shaderDescription.srcPathRelative = "histogramReset.comp";
        d.shaderDescription.specialisationConstants = {spec(0, nHistogramBins)};
        m_histogramResetPass = m_be.createComputePass(d);
        d.name = "Histogram combine tiles";
        d.shaderDescription = histogramCombineShaderDescription(W, H);
        m_histogramCombinePass = m_be.createComputePass(d);
        d.name = "Pre-expose lights";
        d.shaderDescription.srcPathRelative = "preExposeLights.comp";
        d.shaderDescription.specialisationConstants = {spec(0, (int)nHistogramBins), spec(1, histogramMinValue), spec(2, histogramMaxValue)};
        m_preExposeLightsPass = m_be.createComputePass(d);
        d.name = "Tonemap";
        d.shaderDescription.srcPathRelative = "tonemapping.comp";
        d.shaderDescription.specialisationConstants = {};
        m_tonemappingPass = m_be.createComputePass(d);
        d.name = "Depth downscale";
        d.shaderDescription.srcPathRelative = "depthDownscale.comp";
        m_depthDownscalePass = m_be.createComputePass(d);
        d.name = "BRDF Lut creation";
        d.shaderDescription = brdfLutShaderDescription(s.shading);
        m_brdfLutPass = m_be.createComputePass(d);
    }
    {
        ComputePassDescription d;
        d.name = "Depth min/max pyramid";
        d.shaderDescription = depthPyramidShaderDescription();
        m_depthPyramidPass = m_be.createComputePass(d);
    }
    {
        ComputePassDescription d;
        d.name = "Forward shading (deferred)";
        d.shaderDescription = forwardPassShaderDescription(s.shading);
        m_deferredShadingPass = m_be.createComputePass(d);
    }
    {
        ComputePassDescription d; // RenderFrontend.cpp:1730-1740
        d.name = "Compute light matrix";
        d.shaderDescription.srcPathRelative = "lightMatrix.comp";
        d.shaderDescription.specialisationConstants = {spec(0, (uint32_t)s.shading.sunShadowCascadeCount)};
        m_lightMatrixPass = m_be.createComputePass(d);
        d.name = "Depth pyramid apex of the band";
        d.shaderDescription.srcPathRelative = "depthPyramidApex.comp"; // no reference shader: see kernels/hiz.hip
        d.shaderDescription.specialisationConstants = {};
        m_depthApexPass = m_be.createComputePass(d);
    }
    {
        // Sky::init (Techniques/Sky.cpp:5-64, 196-258): LUT sizes 128^2, 32^2, 200x100; the transmission and sky LUT images are the ones the
        // shade / trace / exposure passes already read
        m_skyMultiscatterLut = m_be.createImage(desc2D(32, 32, ImageFormat::R11G11B10_uFloat), nullptr, 0);
        UniformBufferDescription aub;
        aub.size = sizeof(AtmosphereSettings);
        m_atmosphereSettingsBuffer = m_be.createUniformBuffer(aub);
        ComputePassDescription d;
        d.name = "Sky transmission lut";
        d.shaderDescription.srcPathRelative = "skyTransmissionLut.comp";
        m_skyTransmissionLutPass = m_be.createComputePass(d);
        d.name = "Sky multiscatter lut";
        d.shaderDescription.srcPathRelative = "skyMultiscatterLut.comp";
        m_skyMultiscatterLutPass = m_be.createComputePass(d);
        d.name = "Sky lut";
        d.shaderDescription.srcPathRelative = "skyLut.comp";
        m_skyLutPass = m_be.createComputePass(d);
        d.name = "Sky and sun sprite"; // Sky::renderSky's two raster passes as one compute pass (no reference shader: kernels/sky_background.hip)
        d.shaderDescription.srcPathRelative = "skyAndSunSprite.comp";
        m_skyAndSunSpritePass = m_be.createComputePass(d);
    }
    {
        // Volumetrics::init (Techniques/Volumetrics.cpp:19-117): froxel volumes of the integration volume's size; the 32^3 R8 Perlin noise is an
        // input (generate3DPerlinNoise is asset code): uploaded by the caller into "perlinNoise3D", or written by generateNoise
        ImageDescription fd = m_be.getImageDescription(m_volumetricIntegrationVolume);
        m_scatteringTransmittanceVolume = m_be.createImage(fd, nullptr, 0);
        m_volumetricLightingHistory[0] = m_be.createImage(fd, nullptr, 0);
        m_volumetricLightingHistory[1] = m_be.createImage(fd, nullptr, 0);
        m_volumeMaterialVolume = m_be.createImage(fd, nullptr, 0);
        ImageDescription nd;
        nd.width = nd.height = nd.depth = 32; nd.type = ImageType::Type3D; nd.format = ImageFormat::R8; nd.usageFlags = ImageUsageFlags::Sampled;
        m_perlinNoise3D = m_be.createImage(nd, nullptr, 0);
        ComputePassDescription d;
        d.name = "Froxel volume material"; d.shaderDescription.srcPathRelative = "froxelVolumeMaterial.comp";
        m_froxelVolumeMaterialPass = m_be.createComputePass(d);
        d.name = "Froxel light scattering"; d.shaderDescription.srcPathRelative = "froxelLightScattering.comp";
        m_froxelScatteringTransmittancePass = m_be.createComputePass(d);
        d.name = "Volumetric light integration"; d.shaderDescription.srcPathRelative = "volumetricLightingIntegration.comp";
        m_volumetricLightingIntegration = m_be.createComputePass(d);
        d.name = "Volumetric lighting reprojection"; d.shaderDescription.srcPathRelative = "volumeLightingReprojection.comp";
        m_volumetricLightingReprojection = m_be.createComputePass(d);
    }
    m_taa.init(m_be, W, H, s.taa);
    m_bloom.init(m_be);
    m_sdfGi.init(m_be, W, H, s.sdfTrace, s.sdfDebug, s.shading.sunShadowCascadeCount - 1, s.maxSdfInstances);
    const float influence = s.sdfTrace.traceInfluenceRadius;
    (void)influence;
}

ImageHandle FramePipeline::image(const std::string& n) const {
    if (n == "color0") return m_frameRenderTargets[0].colorBuffer;
    if (n == "color1") return m_frameRenderTargets[1].colorBuffer;
    if (n == "motion0") return m_frameRenderTargets[0].motionBuffer;
    if (n == "motion1") return m_frameRenderTargets[1].motionBuffer;
    if (n == "depth0") return m_frameRenderTargets[0].depthBuffer;
    if (n == "depth1") return m_frameRenderTargets[1].depthBuffer;
    if (n == "post0") return m_postProcessBuffers[0];
    if (n == "post1") return m_postProcessBuffers[1];
    if (n == "normal") return m_worldSpaceNormalImage;
    if (n == "shadingNormal") return m_shadingNormalCreated ? m_shadingNormalImage : ImageHandle{}; // (exists once normal maps were set)
    if (n == "albedo") return m_albedoImage;
    if (n == "specular") return m_specularImage;
    if (n == "pyramid") return m_minMaxDepthPyramid;
    if (n == "depthHalfRes") return m_depthHalfRes;
    if (n == "brdfLut") return m_brdfLut;
    if (n == "skyLut") return m_skyLut;
    if (n == "skyMultiscatterLut") return m_skyMultiscatterLut;
    if (n == "perlinNoise3D") return m_perlinNoise3D;
    if (n == "volumetricHistory0") return m_volumetricLightingHistory[0];
    if (n == "volumetricHistory1") return m_volumetricLightingHistory[1];
    if (n == "scatteringTransmittanceVolume") return m_scatteringTransmittanceVolume;
    if (n == "volumeMaterialVolume") return m_volumeMaterialVolume;
    if (n == "transmissionLut") return m_transmissionLut;
    if (n == "volumetricIntegrationVolume") return m_volumetricIntegrationVolume;
    if (n.size() == 7 && n.compare(0, 6, "shadow") == 0) return m_shadowMaps[(n[6] - '0') & 3];
    if (n.size() == 6 && n.compare(0, 5, "noise") == 0) return m_noiseTextures[(n[5] - '0') & 3];
    if (n == "taaHistory0") return m_taa.m_historyBuffers[0];
    if (n == "taaHistory1") return m_taa.m_historyBuffers[1];
    if (n == "sceneLuminance0") return m_taa.m_sceneLuminance[0];
    if (n == "sceneLuminance1") return m_taa.m_sceneLuminance[1];
    if (n == "giYSH0") return m_sdfGi.m_indirectDiffuse_Y_SH[0];
    if (n == "giYSH1") return m_sdfGi.m_indirectDiffuse_Y_SH[1];
    if (n == "giCoCg0") return m_sdfGi.m_indirectDiffuse_CoCg[0];
    if (n == "giCoCg1") return m_sdfGi.m_indirectDiffuse_CoCg[1];
    if (n == "giHistoryYSH0") return m_sdfGi.m_indirectDiffuseHistory_Y_SH[0];
    if (n == "giHistoryYSH1") return m_sdfGi.m_indirectDiffuseHistory_Y_SH[1];
    if (n == "giHistoryCoCg0") return m_sdfGi.m_indirectDiffuseHistory_CoCg[0];
    if (n == "giHistoryCoCg1") return m_sdfGi.m_indirectDiffuseHistory_CoCg[1];
    if (n == "giFullResYSH") return m_sdfGi.m_indirectLightingFullRes_Y_SH;
    if (n == "giFullResCoCg") return m_sdfGi.m_indirectLightingFullRes_CoCg;
    if (n == "swapchain") return const_cast<RenderBackend&>(m_be).getSwapchainInputImage();
    return ImageHandle{};
}

bool FramePipeline::storageBuffer(const std::string& n, StorageBufferHandle* out) const {
    if (n == "histogram") *out = m_histogramBuffer;
    else if (n == "histogramPerTile") *out = m_histogramPerTileBuffer;
    else if (n == "light") *out = m_lightBuffer;
    else if (n == "sunShadowInfo") *out = m_sunShadowInfoBuffer;
    else if (n == "mainPassMatrices" && m_sceneMatrices.bytes) *out = m_sceneMatrices.handle; // (exists once a scene was set)
    else if (n == "sceneCulledDraws" && m_sceneCulledDraws.bytes) *out = m_sceneCulledDraws.handle; // (the cull buffers exist once culling was on with the mesh set present)
    else if (n == "sceneCullStats" && m_sceneCullStats.bytes) *out = m_sceneCullStats.handle;
    else if (n == "casterCullStats" && m_casterCullStats.bytes) *out = m_casterCullStats.handle; // 32 bytes per cascade
    else if (n.size() == 18 && n.compare(0, 17, "casterCulledDraws") == 0 && n[17] >= '0' && n[17] <= '3' && m_casterCulledDraws[n[17] - '0'].bytes) *out = m_casterCulledDraws[n[17] - '0'].handle;
    else if (n == "sceneBounds" && m_sceneBoundsOnGpu) *out = m_sceneBounds.handle; // 6 floats per draw, once draw culling or the debug boxes asked for them
    else if (n == "debugGeometryStats" && m_debugStats.bytes) *out = m_debugStats.handle; // 8 uint32, once setDebugGeometry set a flag
    else if (n == "sdfInstances") *out = m_sdfGi.m_sdfInstanceBuffer;
    else if (n == "sdfCulledInstances") *out = m_sdfGi.m_sdfCameraFrustumCulledInstances;
    else if (n == "sdfCulledTiles") *out = m_sdfGi.m_sdfCameraCulledTiles;
    else if (n == "sdfWorldBBs") *out = m_sdfGi.m_sdfInstanceWorldBBBuffer;
    else return false;
    return true;
}

bool FramePipeline::uniformBuffer(const std::string& n, UniformBufferHandle* out) const {
    if (n == "global") *out = m_globalUniformBuffer;
    else if (n == "volumetricSettings") *out = m_volumetricsInfoBuffer;
    else if (n == "taaResolveWeights") *out = m_taa.m_taaResolveWeightBuffer;
    else if (n == "sdfCameraFrustum") *out = m_sdfGi.m_cameraFrustumBuffer;
    else if (n == "sdfInfluenceRange") *out = m_sdfGi.m_sdfTraceInfluenceRangeBuffer;
    else return false;
    return true;
}

uint32_t FramePipeline::addSdfVolume(uint32_t res, const void* halfData, size_t bytes) {
    ImageDescription d;
    d.width = d.height = d.depth = res;
    d.type = ImageType::Type3D; d.format = ImageFormat::R16_sFloat; d.usageFlags = ImageUsageFlags::Sampled;
    const ImageHandle h = m_be.createImage(d, halfData, bytes);
    m_sdfVolumes.push_back(h);
    return m_be.getImageGlobalTextureArrayIndex(h);
}

uint32_t FramePipeline::addSdfVolumeFromDds(const std::string& path, ImageDescription* outDesc) {
    plr_image_desc cd{};
    size_t size = 0;
    if (plr_load_dds_file(path.c_str(), &cd, nullptr, 0, &size) != PLR_OK) throw std::runtime_error(plr_last_error());
    if (cd.format != PLR_FORMAT_R16_SFLOAT || cd.type != PLR_IMAGE_3D) throw std::runtime_error("SDF texture must be a 3D R16_sFloat DDS: " + path);
    std::vector<uint8_t> data(size);
    if (plr_load_dds_file(path.c_str(), &cd, data.data(), data.size(), &size) != PLR_OK) throw std::runtime_error(plr_last_error());
    ImageDescription d;
    d.width = cd.width; d.height = cd.height; d.depth = cd.depth;
    d.type = ImageType::Type3D; d.format = ImageFormat::R16_sFloat; d.usageFlags = ImageUsageFlags::Sampled;
    d.mipCount = cd.manual_mip_count > 1 ? MipCount::Manual : MipCount::One; d.manualMipCount = cd.manual_mip_count;
    if ((size_t)d.width * d.height * d.depth * 2 > size) throw std::runtime_error("DDS file holds fewer texels than its header declares: " + path);
    const ImageHandle h = m_be.createImage(d, data.data(), data.size());
    m_sdfVolumes.push_back(h);
    if (outDesc) *outDesc = d;
    return m_be.getImageGlobalTextureArrayIndex(h);
}

void FramePipeline::setSdfScene(const void* inst, size_t instBytes, const void* bb, size_t bbBytes) {
    if (m_sceneSdfSet)
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSdfScene: a scene SDF is set (setSceneSdf): sdfInstances and sdfWorldBBs are written by sdfInstanceUpdate.comp every frame; remove it first");
    m_sdfGi.updateSDFScene(m_be, inst, instBytes, bb, bbBytes);
}
void FramePipeline::setSunDirection(const float d[3]) { m_globalShaderInfo.sunDirection[0] = d[0]; m_globalShaderInfo.sunDirection[1] = d[1]; m_globalShaderInfo.sunDirection[2] = d[2]; m_globalShaderInfo.sunDirection[3] = 0.f; }
void FramePipeline::setCameraIntrinsic(float fov, float n, float f) { m_cameraIntrinsic.fov = fov; m_cameraIntrinsic.near = n; m_cameraIntrinsic.far = f; }

void FramePipeline::computeColorBufferHistogram(ImageHandle lastFrameColor) { // RenderFrontend.cpp:707-754
    const StorageBufferResource histogramPerTileResource(m_histogramPerTileBuffer, false, 0);
    const StorageBufferResource histogramResource(m_histogramBuffer, false, 1);
    const uint32_t W = settings.width, H = settings.height;
    const RowRange tileRows = scaleRows(bandRows(0), histogramTileSizeY);
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_histogramPerTilePass;
        exe.genericInfo.resources.storageBuffers = {histogramPerTileResource, StorageBufferResource(m_lightBuffer, true, 3)};
        exe.genericInfo.resources.sampledImages = {ImageResource(lastFrameColor, 0, 2)};
        exe.dispatchCount[0] = uint32_t(std::ceil((float)W / float(histogramTileSizeX)));
        exe.dispatchCount[1] = uint32_t(std::ceil((float)H / float(histogramTileSizeY)));
        exe.dispatchCount[2] = 1;
        if (settings.band.enabled()) { // the band's tile rows; the global histogram is the sum over bands (ExchangeHistogram)
            exe.dispatchBase[1] = tileRows.begin;
            exe.dispatchCount[1] = tileRows.end - tileRows.begin;
            if (settings.band.tiled()) { // and the tile's tile columns
                const ColRange tileCols = scaleRows(bandCols(0), histogramTileSizeX);
                exe.dispatchBase[0] = tileCols.begin;
                exe.dispatchCount[0] = tileCols.end - tileCols.begin;
            }
        }
        m_be.setComputePassExecution(exe);
    }
    const float binsPerDispatch = 64.f;
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_histogramResetPass;
        exe.genericInfo.resources.storageBuffers = {histogramResource};
        exe.dispatchCount[0] = uint32_t(std::ceil(float(nHistogramBins) / binsPerDispatch));
        m_be.setComputePassExecution(exe);
    }
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_histogramCombinePass;
        exe.genericInfo.resources.storageBuffers = {histogramPerTileResource, histogramResource};
        exe.dispatchCount[0] = (uint32_t)std::ceil(W / float(histogramTileSizeX)) * (uint32_t)std::ceil(H / float(histogramTileSizeY));
        exe.dispatchCount[1] = uint32_t(std::ceil(float(nHistogramBins) / binsPerDispatch));
        if (settings.band.enabled()) {
            // (tile rendering: the per-tile buffer is indexed with the whole frame's stride, so a tile's entries are not one range of it; the combine runs over the
            //  whole width of the tile's tile rows and the entries of other GPUs' tiles stay what the buffer was created with - zeros: an integer sum)
            const uint32_t tilesX = (uint32_t)std::ceil(W / float(histogramTileSizeX));
            exe.dispatchBase[0] = tileRows.begin * tilesX;
            exe.dispatchCount[0] = (tileRows.end - tileRows.begin) * tilesX;
        }
        m_be.setComputePassExecution(exe);
    }
}

void FramePipeline::computeExposure() { // RenderFrontend.cpp:776-790
    ComputePassExecution exe;
    exe.genericInfo.handle = m_preExposeLightsPass;
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_histogramBuffer, false, 1), StorageBufferResource(m_lightBuffer, false, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(m_transmissionLut, 0, 2)};
    m_be.setComputePassExecution(exe);
}

void FramePipeline::computeDepthPyramid(ImageHandle depthBuffer) { // RenderFrontend.cpp:804-838
    ComputePassExecution exe;
    exe.genericInfo.handle = m_depthPyramidPass;
    const uint32_t width = settings.width / 2, height = settings.height / 2, maxMipCount = 11;
    const uint32_t mipCount = pyramidMipCount(settings);
    uint32_t dc[2];
    singlePassMipChainDispatchCount(width, height, mipCount, maxMipCount, dc);
    exe.dispatchCount[0] = dc[0]; exe.dispatchCount[1] = dc[1]; exe.dispatchCount[2] = 1;
    if (perTilePyramid(settings)) { // one workgroup per 32x32 texels of pyramid mip 0 = 64 full-resolution rows
        exe.dispatchCount[0] = (width + 31) / 32;
        exe.dispatchCount[1] = (height + 31) / 32;
        if (settings.band.enabled()) {
            const RowRange groups = scaleRows(bandRows(0), 64);
            exe.dispatchBase[1] = groups.begin;
            exe.dispatchCount[1] = groups.end - groups.begin;
            if (settings.band.tiled()) {
                const ColRange groupsX = scaleRows(bandCols(0), 64);
                exe.dispatchBase[0] = groupsX.begin;
                exe.dispatchCount[0] = groupsX.end - groupsX.begin;
            }
        }
    }
    exe.genericInfo.resources.sampledImages = {ImageResource(depthBuffer, 0, 13), ImageResource(m_minMaxDepthPyramid, 0, 15)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_depthPyramidSyncBuffer, false, 16)};
    const uint32_t unusedMipCount = maxMipCount - mipCount;
    for (uint32_t i = 0; i < maxMipCount; i++) {
        const uint32_t mipLevel = i >= unusedMipCount ? i - unusedMipCount : 0;
        exe.genericInfo.resources.storageImages.push_back(ImageResource(m_minMaxDepthPyramid, mipLevel, i));
    }
    m_be.setComputePassExecution(exe);
}

void FramePipeline::downscaleDepth(const FrameRenderTargets& currentTarget) { // RenderFrontend.cpp:873-892
    ComputePassExecution exe;
    exe.genericInfo.handle = m_depthDownscalePass;
    // band: the spatial filters sample half-res depth up to giHalo trace rows away, the upscale one more
    const uint32_t depthHalo = 2 * (settings.band.giHalo + settings.band.giHistoryHalo) + 16;
    dispatch8(exe, settings.width / 2, settings.height / 2, bandRows(depthHalo, 2), bandCols(depthHalo, 2));
    exe.genericInfo.resources.storageImages = {ImageResource(m_depthHalfRes, 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(currentTarget.depthBuffer, 0, 1)};
    m_be.setComputePassExecution(exe);
}

void FramePipeline::computeDeferredShading(ImageHandle colorTarget, const FrameRenderTargets& current) { // renderForwardShading, RenderFrontend.cpp:894-929
    ComputePassExecution exe;
    exe.genericInfo.handle = m_deferredShadingPass;
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_lightBuffer, true, 7), StorageBufferResource(m_sunShadowInfoBuffer, true, 8)};
    const SDFGI::IndirectLightingImages indirectLight = m_sdfGi.getIndirectLightingResults(settings.sdfTrace.halfResTrace);
    exe.genericInfo.resources.storageImages = {ImageResource(colorTarget, 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(m_brdfLut, 0, 3), ImageResource(indirectLight.Y_SH, 0, 15), ImageResource(indirectLight.CoCg, 0, 16),
                                               ImageResource(m_volumetricIntegrationVolume, 0, 18),
                                               // (triangle.frag:180-196 lights with the normal-mapped normal; the trace and the GI filters keep the vertex normal)
                                               ImageResource(current.depthBuffer, 0, 20), ImageResource(normalMapped() ? m_shadingNormalImage : m_worldSpaceNormalImage, 0, 21),
                                               ImageResource(m_albedoImage, 0, 22), ImageResource(m_specularImage, 0, 23), ImageResource(m_skyLut, 0, 24)};
    for (uint32_t i = 0; i < (uint32_t)maxSunShadowCascadeCount; i++) exe.genericInfo.resources.sampledImages.push_back(ImageResource(m_shadowMaps[i], 0, 9 + i));
    exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 19)};
    dispatch8(exe, settings.width, settings.height, bandRows(settings.band.colorHalo), bandCols(settings.band.colorHalo));
    m_be.setComputePassExecution(exe);
}

// Sky::renderSky (Techniques/Sky.cpp:318-353) on the pixels the forward pass left at depth 0: same rows and columns as the shade, so a band / tile has its
// sky wherever it has shaded colour and needs no exchange for it
void FramePipeline::computeSkyAndSunSprite(ImageHandle colorTarget, const FrameRenderTargets& current) {
    ComputePassExecution exe;
    exe.genericInfo.handle = m_skyAndSunSpritePass;
    exe.genericInfo.resources.storageImages = {ImageResource(colorTarget, 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(current.depthBuffer, 0, 1), ImageResource(m_skyLut, 0, 2), ImageResource(m_volumetricIntegrationVolume, 0, 3),
                                               ImageResource(m_transmissionLut, 0, 4)};
    exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 5)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_lightBuffer, true, 6)};
    dispatch8(exe, settings.width, settings.height, bandRows(settings.band.colorHalo), bandCols(settings.band.colorHalo));
    m_be.setComputePassExecution(exe);
}

void FramePipeline::computeTonemapping(ImageHandle src) { // RenderFrontend.cpp:931-945
    ComputePassExecution exe;
    exe.genericInfo.handle = m_tonemappingPass;
    exe.genericInfo.resources.storageImages = {ImageResource(m_be.getSwapchainInputImage(), 0, 0)};
    exe.genericInfo.resources.sampledImages = {ImageResource(src, 0, 1)};
    dispatch8(exe, settings.width, settings.height, bandRows(0), bandCols(0));
    exe.asyncTail = asyncPostTail();
    m_be.setComputePassExecution(exe);
}

// band rendering / a frame too large for one pyramid: the top level of the per-tile pyramid (one texel per 64 x 64 pixels), the band's rows of it, reduced to
// one texel; with an exchange callback the bands' texels are then combined (min on .r, max on .g) - SURVEY 8e's second collective
void FramePipeline::computeDepthApexOfTiles() {
    ComputePassExecution exe;
    exe.genericInfo.handle = m_depthApexPass;
    const uint32_t top = bandPyramidMipCount - 1;
    const uint32_t levelRows = std::max((settings.height / 2) >> top, 1u);
    RowRange rows{0, levelRows};
    if (settings.band.enabled()) {
        rows = scaleRows(bandRows(0), 64); // 64 full-resolution rows per texel of that level
        rows.end = std::min(rows.end, levelRows);
    }
    exe.dispatchCount[0] = 1; exe.dispatchCount[2] = 1; // (one workgroup from column 0: whole rows)
    exe.dispatchBase[1] = rows.begin;
    exe.dispatchCount[1] = rows.end - rows.begin;
    if (settings.band.enabled() && settings.band.tiled()) { // the tile's texel columns of that level
        const uint32_t levelCols = std::max((settings.width / 2) >> top, 1u);
        ColRange cols = scaleRows(bandCols(0), 64);
        cols.end = std::min(cols.end, levelCols);
        exe.dispatchBase[0] = cols.begin;
        exe.dispatchCount[0] = cols.end - cols.begin;
        const int32_t columnRange = 1; // the x range is a range of texel columns, also when it is one column from column 0
        exe.pushConstants = dataToCharArray(&columnRange, sizeof(columnRange));
    }
    exe.genericInfo.resources.sampledImages = {ImageResource(m_minMaxDepthPyramid, top, 0)};
    exe.genericInfo.resources.storageImages = {ImageResource(m_bandDepthApex, 0, 1)};
    m_be.setComputePassExecution(exe);
    if (settings.band.enabled() && m_exchangeFn) {
        m_be.setHostCallbackExecution(&FramePipeline::exchangeTrampoline, &m_exchangeCtx[ExchangeDepthApex], "Exchange: depth range all-reduce (min, max)", {m_bandDepthApex}, {});
    }
}

void FramePipeline::computeSunLightMatrices() { // RenderFrontend.cpp:840-872
    ComputePassExecution exe;
    exe.genericInfo.handle = m_lightMatrixPass;
    exe.dispatchCount[0] = exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
    const uint32_t depthPyramidMipCount = mipCountFromResolution(settings.width / 2, settings.height / 2, 1);
    if (perTilePyramid(settings)) exe.genericInfo.resources.storageImages = {ImageResource(m_bandDepthApex, 0, 1)};
    else exe.genericInfo.resources.storageImages = {ImageResource(m_minMaxDepthPyramid, depthPyramidMipCount - 1, 1)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sunShadowInfoBuffer, false, 0)};
    struct LightMatrixPushConstants { float highestCascadePaddingSize; float highestCascadeMinFarPlane; } pc;
    pc.highestCascadePaddingSize = settings.sdfTrace.traceInfluenceRadius;
    pc.highestCascadeMinFarPlane = settings.volumetricsMaxDistance;
    // if strict cutoff enabled all hits outside influence radius are discarded anyways
    if (!settings.sdfTrace.strictInfluenceRadiusCutoff) pc.highestCascadePaddingSize += settings.sdfTrace.additionalSunShadowMapPadding;
    exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
    m_be.setComputePassExecution(exe);
}

// the scene and caster calls on a partitioned pipeline: refused unless it was created with band.raster
static bool partitionedWithoutRaster(const FramePipelineSettings& s) { return (s.band.enabled() || s.band.tiled()) && !s.band.raster; }

// THE RASTER WINDOW (DESIGN.md "Rasterising in a partition"). Which full-resolution texels of the G-buffer images - the current frame's depth, motion, normal,
// albedo, specular and shadingNormal, last frame's depth and motion - does a recorder of this file read outside the owned rectangle? Per recorder, in pixels:
//   computeDepthPyramid / computeDepthApexOfTiles: workgroups of 64 x 64 pixels over scaleRows(bandRows(0), 64): inside the rectangle rounded out to 64 - reach 0
//     after the rounding below
//   downscaleDepth: half-resolution texels bandRows(depthHalo, 2) with depthHalo = 2 (giHalo + giHistoryHalo) + 16, each from a 2 x 2 footprint; the range's end is
//     rounded up to a whole half-resolution texel: depthHalo + 1
//   SDFGI: the camera-tile culling reads the pyramid only; the trace, both spatial filters (normal at the centre texel; depth from depthHalfRes, or with a
//     full-resolution trace from depth at the disc samples the valid rows admit: giHalo + 1 with the pRight / pUp taps) and the request passes run over
//     bandRows(0, div) and read the full-resolution images at the 2 x 2 footprint of their own texel: 1; a requested texel arrives with its depthHalfRes texel.
//     The temporal GI filter reads last frame's motion bilinearly at uv + motion, which is unbounded; but the value read decides something only where the
//     pixel's own motion is at most 3 pixels on both axes - above that threshold the filter takes alpha = alphaMin whatever last frame's motion is, and a
//     reprojection off the frame takes alpha = 0 (gi_filters.hip temporalGiFilterKernel, pixelThreshold; the fast set's kernel in stream_fast.hip has the same
//     rule). So: the trace texel's own 2 x 2 footprint, 3 pixels of motion, one texel of the bilinear footprint: 3 + 2. A change of that threshold changes this
//     term (kTemporalGiMotionThresholdPixels below)
//   the upscale, computeDeferredShading, computeSkyAndSunSprite: their own pixel over bandRows(colorHalo): colorHalo
//   TAA::computeTemporalFilter: over bandRows(0), the 3 x 3 neighbourhood of depth and motion (the motion vector dilation): 1; the window keeps that 1 on top of
//     colorHalo, so that a temporal filter recorded over the shaded rows stays inside it: colorHalo + 1
//   bloom, tonemap, histogram: no G-buffer image
// The window is the rectangle grown by the largest of these on every side that has a neighbour, rounded out to 64 and clipped to the frame. A whole-image halo
// (giHalo clamped to max(width, height)) makes it the whole frame.
// THE WRAP STRIPS. One read does not fit a rectangle: the temporal GI filter samples last frame's motion with REPEAT addressing (sic, the reference's
// linearRepeat), so a reprojection within half a texel of a frame edge reads the texel column (row) at the OPPOSITE edge (found by the bounded-halo test of
// tests/test_band_raster.py: a handful of pixels next to the frame's edge differed, and only with the far edge's motion poisoned). A window that touches a frame
// edge without spanning the frame in that direction therefore gets a strip: the opposite edge's tile column over the window's tile rows, the opposite edge's
// tile row over its tile columns, and the tile in the opposite corner where both hold. renderDepthPrepass records one more execution per strip.
void rasterWindowTiles(const FramePipelineSettings& s, uint32_t outTiles[4]) {
    const uint64_t W = s.width, H = s.height, T = bandAlignment;
    const uint64_t gridX = (W + T - 1) / T, gridY = (H + T - 1) / T;
    outTiles[0] = outTiles[1] = 0u; outTiles[2] = (uint32_t)gridX; outTiles[3] = (uint32_t)gridY;
    const BandSettings& b = s.band;
    if (!b.enabled()) return;
    const uint64_t cap = std::max(W, H); // the constructor's clamps
    const uint64_t giHalo = b.giRequested || b.giHalo == 0xfffffffeu ? 0u : std::min<uint64_t>(b.giHalo, cap), giHistoryHalo = std::min<uint64_t>(b.giHistoryHalo, cap);
    uint64_t reach = 1u;                                                   // the trace's and the filters' own texel, the temporal filter's 3 x 3
    reach = std::max(reach, 2u * (giHalo + giHistoryHalo) + 16u + 1u);      // downscaleDepth
    reach = std::max(reach, giHalo + 1u);                                  // the spatial filters of a full-resolution trace
    const uint64_t kTemporalGiMotionThresholdPixels = 3u;                  // pixelThreshold of the temporal GI filter kernels
    reach = std::max(reach, kTemporalGiMotionThresholdPixels + 2u);        // the temporal GI filter: last frame's motion, where its value matters
    reach = std::max(reach, (uint64_t)b.colorHalo + 1u);                   // upscale, shade, sky; the motion dilation on top
    auto grow = [&](uint64_t begin, uint64_t end, uint64_t size, uint64_t grid, uint32_t* t0, uint32_t* t1) {
        const uint64_t lo = begin > 0u ? (begin > reach ? begin - reach : 0u) : 0u;
        const uint64_t hi = end < size ? std::min(end + reach, size) : size;
        *t0 = (uint32_t)(lo / T);
        *t1 = (uint32_t)std::min((hi + T - 1) / T, grid);
    };
    grow(b.rowBegin, std::min<uint64_t>(b.rowEnd, H), H, gridY, &outTiles[1], &outTiles[3]);
    if (b.tiled()) grow(b.colBegin, std::min<uint64_t>(b.colEnd, W), W, gridX, &outTiles[0], &outTiles[2]);
}

uint32_t rasterWrapStrips(const FramePipelineSettings& s, uint32_t outTiles[12]) {
    uint32_t w[4];
    rasterWindowTiles(s, w);
    const uint32_t gridX = (s.width + bandAlignment - 1) / bandAlignment, gridY = (s.height + bandAlignment - 1) / bandAlignment;
    // the far tile column / row a wrapped read lands in: none where the window spans the frame in that direction (it holds both edges) or touches no edge
    const bool spansX = w[0] == 0 && w[2] == gridX, spansY = w[1] == 0 && w[3] == gridY;
    const int farX = spansX ? -1 : w[0] == 0 ? (int)gridX - 1 : w[2] == gridX ? 0 : -1;
    const int farY = spansY ? -1 : w[1] == 0 ? (int)gridY - 1 : w[3] == gridY ? 0 : -1;
    uint32_t n = 0;
    auto add = [&](uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { outTiles[4 * n] = x0; outTiles[4 * n + 1] = y0; outTiles[4 * n + 2] = x1; outTiles[4 * n + 3] = y1; n++; };
    if (farX >= 0) add((uint32_t)farX, w[1], (uint32_t)farX + 1, w[3]);
    if (farY >= 0) add(w[0], (uint32_t)farY, w[2], (uint32_t)farY + 1);
    if (farX >= 0 && farY >= 0) add((uint32_t)farX, (uint32_t)farY, (uint32_t)farX + 1, (uint32_t)farY + 1);
    return n;
}

// ---- RenderFrontend::renderSunShadowCascades (RenderFrontend.cpp:760-774, pass :1565-1590) as one compute execution per cascade ("sunShadowRaster.comp",
// kernels/sun_shadow_raster.hip). The reference's coarse CPU frustum culling of the draws (:611-646) is "drawCulling.comp" here, while setDrawCulling has
// kCullShadowCasters set: one execution for all cascades, behind computeSunLightMatrices and against the matrices it fitted, writes a culled copy of the draw
// array per cascade, and each cascade binds its copy at the draw binding. Everything else of a cascade's record is what it is without culling.
void FramePipeline::renderSunShadowCascades() {
    if (m_casterDrawCount == 0) return;
    const bool culled = cullCasters();
    if (culled) recordDrawCulling(true);
    for (int c = 0; c < settings.shading.sunShadowCascadeCount; c++) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_sunShadowRasterPass[c];
        exe.dispatchCount[0] = exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
        exe.genericInfo.resources.storageImages = {ImageResource(m_shadowMaps[c], 0, plr::sunraster::kMapBinding)};
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sunShadowInfoBuffer, true, plr::sunraster::kSunShadowInfoBinding),
                                                    StorageBufferResource(m_casterTransforms.handle, true, plr::sunraster::kTransformBinding),
                                                    StorageBufferResource(m_casterPositions.handle, true, plr::sunraster::kPositionBinding),
                                                    StorageBufferResource(m_casterIndices.handle, true, plr::sunraster::kIndexBinding),
                                                    StorageBufferResource(culled ? m_casterCulledDraws[c].handle : m_casterDraws.handle, true, plr::sunraster::kDrawBinding),
                                                    StorageBufferResource(m_casterScratch[c].handle, false, plr::sunraster::kScratchBinding)};
        // without cutouts, or while every cutoff is 0: the 8-byte record
        const bool tested = m_casterAlphaTested && m_casterTextureCount;
        // a store with a compressed entry: the 16-byte record and binding 14; every other tested one is the 12-byte record it was
        const bool formatted = tested && m_casterCompressed;
        const plr::sunraster::FormatPushConstants pc{m_casterDrawCount, m_casterTriangleCount, tested ? m_casterTextureCount : 0u, formatted ? 1u : 0u};
        exe.pushConstants = dataToCharArray(&pc, formatted ? sizeof(pc) : tested ? sizeof(plr::sunraster::CutoutPushConstants) : sizeof(plr::sunraster::PushConstants));
        if (formatted) exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_casterTextureFormats.handle, true, plr::sunraster::kTextureFormatBinding));
        if (tested) {
            auto& buffers = exe.genericInfo.resources.storageBuffers;
            buffers.push_back(StorageBufferResource(m_casterUvs.handle, true, plr::sunraster::kUvBinding));
            buffers.push_back(StorageBufferResource(m_casterMaterials.handle, true, plr::sunraster::kCasterMaterialBinding));
            buffers.push_back(StorageBufferResource(m_casterTextures.handle, true, plr::sunraster::kTextureBinding));
            buffers.push_back(StorageBufferResource(m_casterTexels.handle, true, plr::sunraster::kTexelBinding));
        }
        m_casterPushBytes = (uint32_t)exe.pushConstants.size();
        m_casterBufferCount = (uint32_t)exe.genericInfo.resources.storageBuffers.size();
        m_be.setComputePassExecution(exe);
    }
}

// a buffer that holds `bytes`: a new, larger one when the current is too small (the backend has no call that frees a buffer; meshes change with the scene, not
// per frame; it never shrinks), then the contents as a queued fill (applied in call order at the next frame). data null: the size only
void FramePipeline::fillBuffer(GrowableBuffer& buffer, const void* data, size_t bytes) {
    if (buffer.bytes < bytes) {
        StorageBufferDescription sb;
        sb.size = (bytes + 255) & ~(size_t)255;
        buffer.handle = m_be.createStorageBuffer(sb);
        buffer.bytes = sb.size;
    }
    if (data) m_be.setStorageBufferData(buffer.handle, data, bytes);
}

void FramePipeline::setShadowCasters(const ShadowCasterMesh* meshes, uint32_t meshCount, const ShadowCasterDraw* draws, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setShadowCasters: a band / tile pipeline cannot rasterise shadow casters (every partition would draw every cascade)");
    if (drawCount == 0) {
        m_casterDrawCount = m_casterTriangleCount = 0;
        dropCasterCutouts();
        m_casterMeshVertexCounts.clear();
        m_casterBoundsHost.clear();
        m_casterBoundsUploaded = m_casterCullRecorded = false;
        return;
    }
    const PackedCasters packed = packShadowCasters(meshes, meshCount, draws, drawCount); // validates everything before anything is changed
    if (!m_casterPassesCreated) {
        for (uint32_t c = 0; c < 4; c++) {
            ComputePassDescription d; // RenderFrontend.cpp:1565-1590, one pass per cascade (sunShadow.vert:8 cascadeIndex)
            d.name = "Sun shadow cascade " + std::to_string(c);
            d.shaderDescription.srcPathRelative = "sunShadowRaster.comp";
            d.shaderDescription.specialisationConstants = {spec(plr::sunraster::kCascadeIndexConstant, c)};
            m_sunShadowRasterPass[c] = m_be.createComputePass(d);
        }
        m_casterPassesCreated = true;
    }
    fillBuffer(m_casterPositions, packed.positions);
    fillBuffer(m_casterIndices, packed.indices);
    fillBuffer(m_casterDraws, packed.draws);
    fillBuffer(m_casterTransforms, packed.models);
    for (int c = 0; c < settings.shading.sunShadowCascadeCount; c++) fillBuffer(m_casterScratch[c], nullptr, plr::sunraster::scratchBytes(packed.triangleCount));
    m_casterDrawCount = drawCount; m_casterTriangleCount = packed.triangleCount;
    m_casterMeshVertexCounts = packed.meshVertexCounts;
    dropCasterCutouts();
    m_casterBoundsHost = packed.drawBounds; // they live and die with the meshes
    m_casterBoundsUploaded = m_casterCullRecorded = false;
    prepareDrawCulling(); // (the removal has nothing to prepare: a view without its mesh set is off)
}

void FramePipeline::setShadowCasterCutouts(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setShadowCasterCutouts: a band / tile pipeline cannot rasterise shadow casters");
    if (textureCount == 0) { dropCasterCutouts(); return; }
    const PackedShadowCutouts packed = packShadowCasterCutouts(textures, textureCount, meshUvs, meshCount, cutouts, drawCount, m_casterMeshVertexCounts.data(),
                                                               (uint32_t)m_casterMeshVertexCounts.size(), m_casterDrawCount); // validates everything before anything is changed
    fillBuffer(m_casterUvs, packed.uvs);
    fillBuffer(m_casterMaterials, packed.materials);
    fillBuffer(m_casterTextures, packed.textures);
    fillBuffer(m_casterTexels, packed.texels);
    for (int c = 0; c < settings.shading.sunShadowCascadeCount; c++) // a tested execution's records are larger
        fillBuffer(m_casterScratch[c], nullptr, plr::sunraster::cutoutScratchBytes(m_casterTriangleCount));
    m_casterTextureCount = textureCount;
    m_casterAlphaTested = packed.tested;
    m_casterCompressed = false; // (the store of a formatted call is replaced)
}

void FramePipeline::setShadowCasterCutoutsFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts,
                                                    uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setShadowCasterCutoutsFormatted: a band / tile pipeline cannot rasterise shadow casters");
    if (textureCount == 0) { dropCasterCutouts(); return; }
    const PackedFormattedShadowCutouts packed = packShadowCasterCutoutsFormatted(textures, textureCount, meshUvs, meshCount, cutouts, drawCount, m_casterMeshVertexCounts.data(),
                                                                                 (uint32_t)m_casterMeshVertexCounts.size(), m_casterDrawCount); // validates everything before anything is changed
    fillBuffer(m_casterUvs, packed.uvs);
    fillBuffer(m_casterMaterials, packed.materials);
    fillBuffer(m_casterTextures, packed.textures);
    fillBuffer(m_casterTexels, packed.texels);
    if (packed.compressed) fillBuffer(m_casterTextureFormats, packed.formats); // (an all-RGBA8 store is setShadowCasterCutouts': no binding 14)
    for (int c = 0; c < settings.shading.sunShadowCascadeCount; c++) // a tested execution's records are larger; a format-aware one's have the same size
        fillBuffer(m_casterScratch[c], nullptr, plr::sunraster::cutoutScratchBytes(m_casterTriangleCount));
    m_casterTextureCount = textureCount;
    m_casterAlphaTested = packed.tested;
    m_casterCompressed = packed.compressed;
}

void FramePipeline::setShadowCasterTransforms(const float* matrices16, uint32_t drawCount) {
    if (drawCount != m_casterDrawCount)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setShadowCasterTransforms: transform count " + std::to_string(drawCount) + " differs from the draw count " +
                                   std::to_string(m_casterDrawCount) + " of the casters");
    if (drawCount == 0) return;
    if (!matrices16) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setShadowCasterTransforms: matrices are null");
    for (uint32_t d = 0; d < drawCount; d++) refuseUnlessAffine(matrices16 + (size_t)d * 16u, d, "setShadowCasterTransforms");
    m_be.setStorageBufferData(m_casterTransforms.handle, matrices16, (size_t)drawCount * 64u);
}

ShadowRasterStats FramePipeline::shadowRasterStats(uint32_t cascade) {
    if (cascade >= (uint32_t)settings.shading.sunShadowCascadeCount)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "shadowRasterStats: cascade " + std::to_string(cascade) + " of " + std::to_string(settings.shading.sunShadowCascadeCount));
    ShadowRasterStats out;
    if (m_casterScratch[cascade].bytes == 0) return out;
    plr::sunraster::ScratchHeader h{};
    if (plr_download_storage_buffer(m_casterScratch[cascade].handle.index, &h, 0, sizeof(h)) != PLR_OK) throw std::runtime_error(plr_last_error());
    out.trianglesSubmitted = h.submitted; out.trianglesDrawn = h.drawn; out.guardBandRejects = h.guardBandRejects;
    return out;
}

// ---- RenderFrontend::renderDepthPrepass (RenderFrontend.cpp:792-802, pass :1717-1735) as one compute execution ("depthPrepassRaster.comp",
// kernels/depth_prepass_raster.hip). The reference's frustum culling of the draws on the host (:565-569) is "drawCulling.comp" here, while setDrawCulling has
// kCullScene set: one execution in front of the pass writes a culled copy of the draw array, against the whole frame's jittered mvp (never a partition's
// window), and the pass - every wrap strip of a band / tile pipeline included - binds the copy at the draw binding. Everything else of the record, drawCount and
// triangleCount included, is what it is without culling: the set-up kernel still clips and rejects per triangle.
void FramePipeline::renderDepthPrepass(const FrameRenderTargets& current) {
    if (m_sceneDrawCount == 0) return;
    const bool culled = cullScene();
    if (culled) recordDrawCulling(false);
    namespace pp = plr::prepass;
    ComputePassExecution exe;
    exe.genericInfo.handle = m_depthPrepassRasterPass;
    exe.dispatchCount[0] = exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
    exe.genericInfo.resources.storageImages = {ImageResource(current.depthBuffer, 0, pp::kDepthBinding), ImageResource(current.motionBuffer, 0, pp::kMotionBinding),
                                               ImageResource(m_worldSpaceNormalImage, 0, pp::kNormalImageBinding), ImageResource(m_albedoImage, 0, pp::kAlbedoBinding),
                                               ImageResource(m_specularImage, 0, pp::kSpecularBinding)};
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sceneMatrices.handle, true, pp::kTransformBinding), StorageBufferResource(m_scenePositions.handle, true, pp::kPositionBinding),
                                                StorageBufferResource(m_sceneNormals.handle, true, pp::kNormalBinding), StorageBufferResource(m_sceneIndices.handle, true, pp::kIndexBinding),
                                                StorageBufferResource(culled ? m_sceneCulledDraws.handle : m_sceneDraws.handle, true, pp::kDrawBinding),
                                                StorageBufferResource(m_sceneScratch.handle, false, pp::kScratchBinding)};
    const bool alphaTested = m_sceneAlphaTested && m_sceneTextureCount;
    const bool compressed = m_sceneTexturesCompressed && m_sceneTextureCount;
    const bool anisotropic = m_sceneMaxAnisotropy >= 2u && m_sceneTextureCount;
    const pp::AnisoPushConstants pc{m_sceneDrawCount, m_sceneTriangleCount, m_sceneTextureCount, alphaTested ? 1u : 0u, normalMapped() ? m_sceneNormalDecode : 0u, compressed ? 1u : 0u,
                                    anisotropic ? m_sceneMaxAnisotropy : 0u};
    // without textures: the 8-byte record; without a cutoff other than 0: the 12-byte one; without normal maps: the 16-byte one; without a compressed texture: the 20-byte one;
    // without anisotropic filtering: the 24-byte one (with it and an all-RGBA8 store: 28 bytes with word 6 at 0, and no binding 14)
    exe.pushConstants = dataToCharArray(&pc, anisotropic ? sizeof(pc) : compressed ? sizeof(pp::FormatPushConstants) : normalMapped() ? sizeof(pp::NormalPushConstants) : alphaTested ? sizeof(pp::AlphaPushConstants) : m_sceneTextureCount ? sizeof(pp::TexturedPushConstants) : sizeof(pp::PushConstants));
    if (m_sceneTextureCount) {
        auto& buffers = exe.genericInfo.resources.storageBuffers;
        buffers.push_back(StorageBufferResource(m_sceneUvs.handle, true, pp::kUvBinding)); buffers.push_back(StorageBufferResource(m_sceneMaterials.handle, true, pp::kMaterialBinding));
        buffers.push_back(StorageBufferResource(m_sceneTextures.handle, true, pp::kTextureBinding)); buffers.push_back(StorageBufferResource(m_sceneTexels.handle, true, pp::kTexelBinding));
        if (alphaTested) buffers.push_back(StorageBufferResource(m_sceneAlphaCutoffs.handle, true, pp::kAlphaCutoffBinding));
        if (compressed) buffers.push_back(StorageBufferResource(m_sceneTextureFormats.handle, true, pp::kTextureFormatBinding));
        if (normalMapped()) {
            buffers.push_back(StorageBufferResource(m_sceneTangents.handle, true, pp::kTangentBinding)); buffers.push_back(StorageBufferResource(m_sceneBitangents.handle, true, pp::kBitangentBinding));
            buffers.push_back(StorageBufferResource(m_sceneNormalMaterials.handle, true, pp::kNormalMaterialBinding));
            exe.genericInfo.resources.storageImages.push_back(ImageResource(m_shadingNormalImage, 0, pp::kShadingNormalBinding));
        }
    }
    if (settings.band.enabled()) { // (only with band.raster: a scene cannot be set otherwise) the 44-byte record: words 0 - 6 as above, then this rank's raster window
        uint32_t w[4];
        rasterWindowTiles(settings, w);
        pp::WindowPushConstants wpc{pc.drawCount, pc.triangleCount, pc.textureCount, pc.alphaTest, pc.normalMap, pc.textureFormats, pc.maxAnisotropy, w[0], w[1], w[2], w[3]};
        exe.pushConstants = dataToCharArray(&wpc, sizeof(wpc));
        // the wrap strips (rasterWrapStrips): the same record with another window, in front of the main execution - the counters each leaves are the same
        uint32_t strips[12];
        const uint32_t stripCount = rasterWrapStrips(settings, strips);
        for (uint32_t k = 0; k < stripCount; k++) {
            ComputePassExecution strip = exe;
            wpc.windowTileX0 = strips[4 * k]; wpc.windowTileY0 = strips[4 * k + 1]; wpc.windowTileX1 = strips[4 * k + 2]; wpc.windowTileY1 = strips[4 * k + 3];
            strip.pushConstants = dataToCharArray(&wpc, sizeof(wpc));
            m_be.setComputePassExecution(strip);
        }
    }
    m_be.setComputePassExecution(exe);
    m_sceneRecorded = true;
}

// ---- "drawCulling.comp" (kernels/draw_culling.hip; DESIGN.md "Frustum culling of draws")
void FramePipeline::setDrawCulling(uint32_t flags) {
    if (flags & ~(kCullScene | kCullShadowCasters))
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDrawCulling: unknown flag bits " + std::to_string(flags & ~(kCullScene | kCullShadowCasters)) + " (1: the scene's draws, 2: the shadow casters)");
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setDrawCulling: a band / tile pipeline cannot rasterise scene meshes or shadow casters, so there is nothing to cull");
    if ((flags ^ m_cullFlags) & kCullScene) m_sceneCullRecorded = false;
    if ((flags ^ m_cullFlags) & kCullShadowCasters) m_casterCullRecorded = false;
    m_cullFlags = flags;
    prepareDrawCulling();
}

// the passes and the buffers of the views that are on and have their mesh set: created or grown here, from the calls that change either, never while a frame is
// recorded. A view that is off allocates nothing
void FramePipeline::prepareDrawCulling() {
    namespace dc = plr::drawcull;
    if (!cullScene() && !cullCasters()) return;
    if (!m_cullPassesCreated) {
        for (int k = 0; k < 2; k++) {
            ComputePassDescription d;
            d.name = k == 0 ? "Draw culling, main view" : "Draw culling, shadow cascades";
            d.shaderDescription.srcPathRelative = "drawCulling.comp";
            m_drawCullingPass[k] = m_be.createComputePass(d);
        }
        m_cullPassesCreated = true;
    }
    if (cullScene() && !m_sceneBoundsUploaded) {
        uploadSceneBounds();
        fillBuffer(m_sceneCulledDraws, nullptr, (size_t)m_sceneDrawCount * sizeof(plr::prepass::Draw));
        fillBuffer(m_sceneCullStats, nullptr, dc::statsBytes(1));
        m_sceneBoundsUploaded = true;
    }
    if (cullCasters() && !m_casterBoundsUploaded) {
        fillBuffer(m_casterBounds, m_casterBoundsHost);
        for (int c = 0; c < settings.shading.sunShadowCascadeCount; c++) fillBuffer(m_casterCulledDraws[c], nullptr, (size_t)m_casterDrawCount * sizeof(plr::sunraster::Draw));
        fillBuffer(m_casterCullStats, nullptr, dc::statsBytes(dc::kMaxViews));
        m_casterBoundsUploaded = true;
    }
}

void FramePipeline::recordDrawCulling(bool shadowViews) {
    namespace dc = plr::drawcull;
    ComputePassExecution exe;
    exe.genericInfo.handle = m_drawCullingPass[shadowViews ? 1 : 0];
    exe.dispatchCount[0] = exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
    auto& buffers = exe.genericInfo.resources.storageBuffers;
    if (!shadowViews) {
        buffers = {StorageBufferResource(m_sceneDraws.handle, true, dc::kDrawBinding), StorageBufferResource(m_sceneBounds.handle, true, dc::kBoundsBinding),
                   StorageBufferResource(m_sceneMatrices.handle, true, dc::kTransformBinding), StorageBufferResource(m_sceneCullStats.handle, false, dc::kStatsBinding),
                   StorageBufferResource(m_sceneCulledDraws.handle, false, dc::kCulledDrawBinding)};
        const dc::PushConstants pc{m_sceneDrawCount, dc::kViewMain, 1u};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        m_sceneCullRecorded = true;
    } else {
        const uint32_t cascades = (uint32_t)settings.shading.sunShadowCascadeCount;
        buffers = {StorageBufferResource(m_casterDraws.handle, true, dc::kDrawBinding), StorageBufferResource(m_casterBounds.handle, true, dc::kBoundsBinding),
                   StorageBufferResource(m_casterTransforms.handle, true, dc::kTransformBinding), StorageBufferResource(m_sunShadowInfoBuffer, true, dc::kSunShadowInfoBinding),
                   StorageBufferResource(m_casterCullStats.handle, false, dc::kStatsBinding)};
        for (uint32_t c = 0; c < cascades; c++) buffers.push_back(StorageBufferResource(m_casterCulledDraws[c].handle, false, dc::kCulledDrawBinding + (int)c));
        const dc::PushConstants pc{m_casterDrawCount, dc::kViewShadow, cascades};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        m_casterCullRecorded = true;
    }
    m_be.setComputePassExecution(exe);
}

void FramePipeline::uploadSceneBounds() {
    if (m_sceneBoundsOnGpu || m_sceneDrawCount == 0) return;
    fillBuffer(m_sceneBounds, m_sceneBoundsHost);
    m_sceneBoundsOnGpu = true;
}

// ---- "debugGeometry.comp" (kernels/debug_geometry.hip; DESIGN.md "Debug geometry as a compute pass")
void FramePipeline::refuseDebugGeometryUnsupported(const char* call) const {
    if (m_requestedSettings.band.enabled())
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, std::string(call) + ": a band / tile pipeline cannot draw debug geometry (the pass writes depth and has no halo plan)");
    if (!m_requestedSettings.runShading)
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, std::string(call) + ": a pipeline without run_shading has no shaded colour buffer to draw debug geometry into");
}

void FramePipeline::setDebugGeometry(uint32_t flags) {
    const uint32_t known = kDebugDrawBoxes | kDebugSdfBoxes | kDebugLines;
    if (flags & ~known)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDebugGeometry: unknown flag bits " + std::to_string(flags & ~known) + " (1: draw boxes, 2: SDF boxes, 4: lines)");
    refuseDebugGeometryUnsupported("setDebugGeometry");
    m_debugFlags = flags;
    if (flags == 0) m_debugRecorded = false;
    prepareDebugGeometry();
}

void FramePipeline::setDebugLines(const DebugLine* lines, uint32_t count) {
    namespace dg = plr::debuggeo;
    if (count && !lines) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDebugLines: lines are null with a count of " + std::to_string(count));
    if (count > dg::kMaxLines) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDebugLines: " + std::to_string(count) + " lines, at most " + std::to_string(dg::kMaxLines) + " (2^20) are accepted");
    for (uint32_t l = 0; l < count; l++) {
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(lines[l].a[k]) || !std::isfinite(lines[l].b[k]))
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDebugLines: line " + std::to_string(l) + " has a non-finite coordinate");
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(lines[l].rgb[k]) || lines[l].rgb[k] < 0.f)
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setDebugLines: line " + std::to_string(l) + " has a non-finite or negative colour component");
    }
    refuseDebugGeometryUnsupported("setDebugLines");
    static_assert(sizeof(DebugLine) == dg::kLineFloats * sizeof(float), "a line is 9 floats");
    m_debugLinesHost.assign((const float*)lines, (const float*)lines + (size_t)count * dg::kLineFloats);
    m_debugLinesUploaded = false;
    prepareDebugGeometry();
}

// the pass and the buffers of the sources that are flagged and present: created or grown here, from the calls that change either, never while a frame is
// recorded. Flags 0 allocate nothing
void FramePipeline::prepareDebugGeometry() {
    if (m_debugFlags == 0) return;
    if (!m_debugPassCreated) {
        ComputePassDescription d; // RenderFrontend.cpp:1599-1617
        d.name = "Debug geometry";
        d.shaderDescription.srcPathRelative = "debugGeometry.comp";
        m_debugGeometryPass = m_be.createComputePass(d);
        const plr::debuggeo::Stats zero{};
        fillBuffer(m_debugStats, &zero, sizeof(zero));
        m_debugPassCreated = true;
    }
    if (m_debugFlags & kDebugDrawBoxes) uploadSceneBounds();
    if ((m_debugFlags & kDebugLines) && !m_debugLinesUploaded && !m_debugLinesHost.empty()) {
        fillBuffer(m_debugLines, m_debugLinesHost);
        m_debugLinesUploaded = true;
    }
}

// one execution behind the deferred shade. sdfBoxesWritten: this frame recorded "sdfInstanceUpdate.comp" in front of it (sdfWorldBBs holds the scene's boxes)
void FramePipeline::recordDebugGeometry(const FrameRenderTargets& current, bool sdfBoxesWritten) {
    namespace dg = plr::debuggeo;
    const bool drawBoxes = (m_debugFlags & kDebugDrawBoxes) && m_sceneDrawCount != 0 && m_sceneBoundsOnGpu;
    const bool sdfBoxes = (m_debugFlags & kDebugSdfBoxes) && sdfBoxesWritten && !m_sceneSdf.instanceDraws.empty();
    const bool lines = (m_debugFlags & kDebugLines) && m_debugLinesUploaded && !m_debugLinesHost.empty();
    const bool culled = drawBoxes && cullScene() && m_sceneRecorded; // (the prepass of this frame ran the cull in front of it)
    ComputePassExecution exe;
    exe.genericInfo.handle = m_debugGeometryPass;
    exe.dispatchCount[0] = exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
    exe.genericInfo.resources.storageImages = {ImageResource(current.colorBuffer, 0, dg::kColorBinding), ImageResource(current.depthBuffer, 0, dg::kDepthBinding)};
    auto& buffers = exe.genericInfo.resources.storageBuffers;
    if (drawBoxes)
        buffers = {StorageBufferResource(culled ? m_sceneCulledDraws.handle : m_sceneDraws.handle, true, dg::kDrawBinding), StorageBufferResource(m_sceneBounds.handle, true, dg::kBoundsBinding),
                   StorageBufferResource(m_sceneMatrices.handle, true, dg::kTransformBinding)};
    if (sdfBoxes) buffers.push_back(StorageBufferResource(m_sdfGi.m_sdfInstanceWorldBBBuffer, true, dg::kSdfBoxBinding));
    if (lines) buffers.push_back(StorageBufferResource(m_debugLines.handle, true, dg::kLineBinding));
    buffers.push_back(StorageBufferResource(m_debugStats.handle, false, dg::kStatsBinding));
    const dg::PushConstants pc{drawBoxes ? m_sceneDrawCount : 0u, sdfBoxes ? (uint32_t)m_sceneSdf.instanceDraws.size() : 0u,
                               lines ? (uint32_t)(m_debugLinesHost.size() / dg::kLineFloats) : 0u, culled ? 1u : 0u};
    exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
    m_be.setComputePassExecution(exe);
    m_debugRecorded = true;
}

FramePipeline::DebugGeometryStats FramePipeline::debugGeometryStats() {
    DebugGeometryStats out;
    if (!m_debugRecorded) return out;
    plr::debuggeo::Stats s{};
    if (plr_download_storage_buffer(m_debugStats.handle.index, &s, 0, sizeof(s)) != PLR_OK) throw std::runtime_error(plr_last_error());
    out.submitted = s.submitted; out.clipped = s.clipped; out.rejected = s.rejected; out.drawn = s.drawn; out.fragments = s.fragments; out.pixelsWritten = s.pixelsWritten;
    return out;
}

FramePipeline::DrawCullingStats FramePipeline::drawCullingStats(uint32_t view) {
    namespace dc = plr::drawcull;
    const uint32_t cascades = (uint32_t)settings.shading.sunShadowCascadeCount;
    if (view >= 1u + cascades)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "drawCullingStats: view " + std::to_string(view) + " of " + std::to_string(1u + cascades) + " (0: the main pass, 1 + c: cascade c)");
    DrawCullingStats out;
    const bool main = view == 0u;
    if (main ? !(cullScene() && m_sceneCullRecorded) : !(cullCasters() && m_casterCullRecorded)) return out;
    dc::ViewStats s{};
    const StorageBufferHandle buffer = main ? m_sceneCullStats.handle : m_casterCullStats.handle;
    if (plr_download_storage_buffer(buffer.index, &s, main ? 0u : (size_t)(view - 1u) * sizeof(s), sizeof(s)) != PLR_OK) throw std::runtime_error(plr_last_error());
    out.draws = main ? m_sceneDrawCount : m_casterDrawCount; out.triangles = main ? m_sceneTriangleCount : m_casterTriangleCount;
    out.visibleDraws = s.visibleDraws; out.visibleTriangles = s.visibleTriangles;
    for (uint32_t k = 0; k < dc::kPlaneCount; k++) out.culledByPlane[k] = s.culledByPlane[k];
    return out;
}

// MainPassMatrices per draw (RenderFrontend.cpp:581-585): {model, mvp = viewProjection * model, mvpPrevious = viewProjectionPrevious * previousModel}. A draw's
// previous model matrix is the one the last recorded frame used (obj.previousModelMatrix, :584); the current one on the first frame of a scene and on a camera cut
void FramePipeline::updateMainPassMatrices() {
    if (m_sceneDrawCount == 0) return;
    if (!m_scenePreviousValid || m_globalShaderInfo.cameraCut) m_scenePreviousModel = m_sceneModel;
    std::vector<plr::prepass::MainPassMatrices> matrices(m_sceneDrawCount);
    for (uint32_t d = 0; d < m_sceneDrawCount; d++) {
        Mat4 model, previous;
        std::memcpy(model.m, m_sceneModel.data() + (size_t)d * 16u, 64);
        std::memcpy(previous.m, m_scenePreviousModel.data() + (size_t)d * 16u, 64);
        const Mat4 mvp = mul(m_globalShaderInfo.viewProjection, model), mvpPrevious = mul(m_globalShaderInfo.viewProjectionPrevious, previous);
        std::memcpy(matrices[d].model, model.m, 64); std::memcpy(matrices[d].mvp, mvp.m, 64); std::memcpy(matrices[d].mvpPrevious, mvpPrevious.m, 64);
    }
    m_be.setStorageBufferData(m_sceneMatrices.handle, matrices.data(), matrices.size() * sizeof(matrices[0]));
    m_scenePreviousModel = m_sceneModel;
    m_scenePreviousValid = true;
}

void FramePipeline::setSceneMeshes(const SceneMesh* meshes, uint32_t meshCount, const SceneDraw* draws, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneMeshes: a band / tile pipeline cannot rasterise scene meshes (a partition would have to rasterise only its own rectangle)");
    if (drawCount == 0) {
        m_sceneDrawCount = m_sceneTriangleCount = 0;
        m_scenePreviousValid = m_sceneRecorded = false;
        dropSceneTextures();
        m_sceneMeshVertexCounts.clear(); m_sceneMeshHasNormals.clear(); m_sceneNormalsHost.clear();
        removeSceneSdf(); // its mesh indices named the scene that is gone
        m_scenePositionsHost.clear(); m_sceneIndicesHost.clear(); m_sceneDrawMeshes.clear(); m_sceneMeshFirstIndex.clear(); m_sceneMeshIndexCounts.clear();
        m_sceneBoundsHost.clear();
        m_sceneBoundsUploaded = m_sceneCullRecorded = m_sceneBoundsOnGpu = false;
        return;
    }
    const PackedScene packed = packSceneMeshes(meshes, meshCount, draws, drawCount); // validates everything before anything is changed
    removeSceneSdf(); // mesh indices no longer mean what they meant
    if (!m_scenePassCreated) {
        ComputePassDescription d; // RenderFrontend.cpp:1717-1735
        d.name = "Depth prepass";
        d.shaderDescription.srcPathRelative = "depthPrepassRaster.comp";
        m_depthPrepassRasterPass = m_be.createComputePass(d);
        m_scenePassCreated = true;
    }
    fillBuffer(m_scenePositions, packed.positions);
    fillBuffer(m_sceneNormals, packed.normals);
    fillBuffer(m_sceneIndices, packed.indices);
    fillBuffer(m_sceneDraws, packed.draws);
    fillBuffer(m_sceneMatrices, nullptr, (size_t)drawCount * sizeof(plr::prepass::MainPassMatrices)); // filled by every frame
    fillBuffer(m_sceneScratch, nullptr, plr::prepass::scratchBytes(packed.triangleCount));
    m_sceneModel = packed.models;
    m_scenePreviousValid = m_sceneRecorded = false;
    m_sceneDrawCount = drawCount; m_sceneTriangleCount = packed.triangleCount;
    m_sceneMeshVertexCounts = packed.meshVertexCounts;
    dropSceneTextures();
    m_sceneMeshHasNormals = packed.meshHasNormals;
    m_sceneNormalsHost = packed.normals;
    m_scenePositionsHost = packed.positions; m_sceneIndicesHost = packed.indices; // what a later setSceneSdf takes the local boxes and the bake from
    m_sceneDrawMeshes = packed.drawMeshes; m_sceneMeshFirstIndex = packed.meshFirstIndex; m_sceneMeshIndexCounts = packed.meshIndexCounts;
    m_sceneBoundsHost = packed.drawBounds; // they live and die with the meshes
    m_sceneBoundsUploaded = m_sceneCullRecorded = m_sceneBoundsOnGpu = false;
    prepareDrawCulling();
    prepareDebugGeometry();
}

void FramePipeline::setSceneTextures(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneTextures: a band / tile pipeline cannot rasterise scene meshes");
    if (textureCount == 0) { dropSceneTextures(); noteSceneTexturesChanged(0); return; } // (setSceneMeshes removes the scene's SDF instead: here it stays, its means stale)
    const PackedTextures packed = packSceneTextures(textures, textureCount, meshUvs, meshCount, materials, drawCount, m_sceneMeshVertexCounts.data(),
                                                    (uint32_t)m_sceneMeshVertexCounts.size(), m_sceneDrawCount); // validates everything before anything is changed
    takeSceneTextures(packed, textureCount, nullptr);
}

void FramePipeline::setSceneTexturesFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneTexturesFormatted: a band / tile pipeline cannot rasterise scene meshes");
    if (textureCount == 0) { dropSceneTextures(); noteSceneTexturesChanged(0); return; }
    const PackedFormattedTextures packed = packSceneTexturesFormatted(textures, textureCount, meshUvs, meshCount, materials, drawCount, m_sceneMeshVertexCounts.data(),
                                                                      (uint32_t)m_sceneMeshVertexCounts.size(), m_sceneDrawCount); // validates everything before anything is changed
    takeSceneTextures(packed, textureCount, packed.compressed ? &packed.formats : nullptr);
}

// ---- the texture store built on the GPU: "textureMipChain.comp" and "textureBlockEncode.comp" (kernels/texture_build.hip; DESIGN.md "Texture store built on the GPU")
void FramePipeline::buildSceneTextures(const SceneTextureSource* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "buildSceneTextures: a band / tile pipeline cannot rasterise scene meshes");
    if (textureCount == 0) { dropSceneTextures(); noteSceneTexturesChanged(0); return; }
    const PackedTextureBuild packed = packSceneTextureBuild(textures, textureCount, meshUvs, meshCount, materials, drawCount, m_sceneMeshVertexCounts.data(),
                                                            (uint32_t)m_sceneMeshVertexCounts.size(), m_sceneDrawCount); // validates everything before anything is changed
    if (!m_textureBuildPassesCreated) {
        ComputePassDescription d;
        d.name = "Texture mip chain";
        d.shaderDescription.srcPathRelative = "textureMipChain.comp";
        m_textureMipChainPass = m_be.createComputePass(d);
        d.name = "Texture block encode";
        d.shaderDescription.srcPathRelative = "textureBlockEncode.comp";
        m_textureBlockEncodePass = m_be.createComputePass(d);
        m_textureBuildPassesCreated = true;
    }
    takeSceneTextures(packed, textureCount, packed.compressed ? &packed.formats : nullptr);
    if (!packed.chainJobs.empty()) fillBuffer(m_textureChainJobs, packed.chainJobs);
    if (!packed.encodeJobs.empty()) fillBuffer(m_textureEncodeJobs, packed.encodeJobs);
    if (!packed.staging.empty()) { fillBuffer(m_textureStaging, packed.staging); m_textureStagingHeld = m_textureStagingQueued = true; }
    m_textureChainLaunches = packed.chainLaunches;
    m_textureEncodeJobCount = (uint32_t)(packed.encodeJobs.size() * 4u / sizeof(plr::texbuild::EncodeJob)); m_textureEncodeGroups = packed.encodeGroups;
    m_textureBuildPendingStats = TextureBuildStats{(uint32_t)packed.chainLaunches.size(), m_textureEncodeJobCount ? 1u : 0u, packed.chainTexels, packed.blocksEncoded,
                                                   packed.staging.size() * sizeof(uint32_t)};
    m_textureBuildPending = true; // (takeSceneTextures cleared it: the passes of a build that was replaced are never recorded)
}

void FramePipeline::recordTextureBuild() {
    releaseTextureStaging(); // of a build an earlier frame has run
    m_sceneStoreInFrame = m_sceneTextureCount != 0;
    m_textureStagingQueued = false; // this frame applies the fill
    if (!m_textureBuildPending) return;
    namespace tb = plr::texbuild;
    const bool staging = m_textureBuildPendingStats.stagingBytes != 0;
    for (const PackedTextureBuild::ChainLaunch& launch : m_textureChainLaunches) { // level by level: a level reads the one the execution before it wrote
        ComputePassExecution exe;
        exe.genericInfo.handle = m_textureMipChainPass;
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_textureChainJobs.handle, true, tb::kChainJobBinding), StorageBufferResource(m_sceneTexels.handle, false, tb::kChainStoreBinding)};
        if (staging) exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_textureStaging.handle, false, tb::kChainStagingBinding));
        const tb::ChainPushConstants pc{launch.firstJob, launch.jobCount, launch.groupCount, staging ? 1u : 0u};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        exe.dispatchCount[0] = launch.groupCount; exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
        m_be.setComputePassExecution(exe);
    }
    if (m_textureEncodeJobCount) {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_textureBlockEncodePass;
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_textureEncodeJobs.handle, true, tb::kEncodeJobBinding), StorageBufferResource(m_sceneTexels.handle, false, tb::kEncodeStoreBinding),
                                                    StorageBufferResource(m_textureStaging.handle, true, tb::kEncodeStagingBinding)};
        const tb::EncodePushConstants pc{m_textureEncodeJobCount, m_textureEncodeGroups};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        exe.dispatchCount[0] = m_textureEncodeGroups; exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
        m_be.setComputePassExecution(exe);
    }
    m_textureBuildStats = m_textureBuildPendingStats;
    m_textureBuildPending = false;
}

// the staging chains have served once the frame that recorded the build has run: the buffer shrinks to one line (the backend frees the memory; this waits for
// the GPU, once per build). Called at the start of the next frame and by the readback
void FramePipeline::releaseTextureStaging() {
    if (!m_textureStagingHeld || m_textureStagingQueued) return; // (queued: its fill waits for a frame, and a buffer with a queued fill cannot be resized)
    m_be.resizeStorageBuffer(m_textureStaging.handle, 256);
    m_textureStaging.bytes = 256;
    m_textureStagingHeld = false;
}

uint64_t FramePipeline::readSceneTextureStore(uint32_t* outWords, uint64_t capacityWords) {
    if (m_sceneTextureCount == 0) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "readSceneTextureStore: no texture store is set");
    if (m_textureBuildPending)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "readSceneTextureStore: the store is not built yet: no frame has run since plrf_build_scene_textures (the next plrf_frame records the build passes)");
    if (!m_sceneStoreInFrame)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "readSceneTextureStore: the store is not uploaded yet: no frame has run since the call that set it");
    if (outWords) {
        if (capacityWords < m_sceneTexelWords)
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "readSceneTextureStore: room for " + std::to_string(capacityWords) + " words, the store holds " + std::to_string(m_sceneTexelWords));
        if (m_sceneTexelWords && plr_download_storage_buffer(m_sceneTexels.handle.index, outWords, 0, (size_t)m_sceneTexelWords * 4u) != PLR_OK) throw std::runtime_error(plr_last_error());
        releaseTextureStaging(); // (the download waited for the GPU)
    }
    return m_sceneTexelWords;
}

void FramePipeline::takeSceneTextures(const PackedTextures& packed, uint32_t textureCount, const std::vector<uint32_t>* formats) {
    m_textureBuildPending = false; // a build that no frame has recorded is replaced with its store
    m_sceneStoreInFrame = false;
    m_sceneTexelWords = packed.texels.size();
    fillBuffer(m_sceneUvs, packed.uvs);
    fillBuffer(m_sceneMaterials, packed.materials);
    fillBuffer(m_sceneTextures, packed.textures);
    fillBuffer(m_sceneTexels, packed.texels);
    if (formats) fillBuffer(m_sceneTextureFormats, *formats);
    m_sceneTextureCount = textureCount;
    m_sceneTexturesCompressed = formats != nullptr;
    dropSceneAlphaCutoffs(); // of the materials that were replaced
    dropSceneNormalMaps();   // they named textures that were replaced
    uint32_t largest = 0;
    for (uint32_t t = 0; t < textureCount; t++) largest = std::max(largest, packed.textures[4u * t + 1u] * packed.textures[4u * t + 2u]);
    noteSceneTexturesChanged(largest);
}

void FramePipeline::setSceneNormalMaps(const float* const* meshTangents, const float* const* meshBitangents, uint32_t meshCount, const uint32_t* normalTextures, uint32_t drawCount,
                                       uint32_t decode) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneNormalMaps: a band / tile pipeline cannot rasterise scene meshes");
    if (drawCount == 0) { dropSceneNormalMaps(); return; }
    SceneNormalMapContext scene;
    scene.meshVertexCounts = m_sceneMeshVertexCounts.data(); scene.meshHasNormals = m_sceneMeshHasNormals.data(); scene.normals = m_sceneNormalsHost.data();
    scene.meshCount = (uint32_t)m_sceneMeshVertexCounts.size(); scene.drawCount = m_sceneDrawCount; scene.textureCount = m_sceneTextureCount;
    const PackedNormalMaps packed = packSceneNormalMaps(meshTangents, meshBitangents, meshCount, normalTextures, drawCount, decode, scene); // validates everything before anything is changed
    fillBuffer(m_sceneTangents, packed.tangents);
    fillBuffer(m_sceneBitangents, packed.bitangents);
    fillBuffer(m_sceneNormalMaterials, packed.normalMaterials);
    if (!m_shadingNormalCreated) { // at the size the other G-buffer images have now: a pending resize re-creates it with them
        m_shadingNormalImage = m_be.createImage(desc2D(settings.width, settings.height, ImageFormat::RGBA8), nullptr, 0);
        m_shadingNormalCreated = true;
    }
    m_sceneNormalDecode = packed.decode;
}

void FramePipeline::setSceneAlphaCutoffs(const uint32_t* cutoffs, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneAlphaCutoffs: a band / tile pipeline cannot rasterise scene meshes");
    if (drawCount == 0) { dropSceneAlphaCutoffs(); return; }
    const PackedAlphaCutoffs packed = packSceneAlphaCutoffs(cutoffs, drawCount, m_sceneDrawCount, m_sceneTextureCount); // validates everything before anything is changed
    fillBuffer(m_sceneAlphaCutoffs, packed.cutoffs);
    m_sceneAlphaTested = packed.tested;
}

void FramePipeline::setSceneAnisotropy(uint32_t maxAnisotropy) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneAnisotropy: a band / tile pipeline cannot rasterise scene meshes");
    if (maxAnisotropy > plr::prepass::kMaxAnisotropy)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setSceneAnisotropy: max anisotropy " + std::to_string(maxAnisotropy) + " is above 16 (0 or 1: off, 2 .. 16: on)");
    m_sceneMaxAnisotropy = maxAnisotropy;
}

void FramePipeline::setSceneMeshTransforms(const float* matrices16, uint32_t drawCount) {
    if (drawCount != m_sceneDrawCount)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setSceneMeshTransforms: transform count " + std::to_string(drawCount) + " differs from the draw count " +
                                   std::to_string(m_sceneDrawCount) + " of the scene");
    if (drawCount == 0) return;
    if (!matrices16) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "setSceneMeshTransforms: matrices are null");
    refuseNonFiniteMatrices(matrices16, drawCount, "setSceneMeshTransforms");
    if (m_sceneSdfSet) refuseSingularSceneSdfMatrices(matrices16, drawCount, m_sceneSdf, m_sceneDrawMeshes.data(), "setSceneMeshTransforms");
    m_sceneModel.assign(matrices16, matrices16 + (size_t)drawCount * 16u);
}

// ---- SDFGI::updateSDFScene (Techniques/SDFGI.cpp:260-313) as "sdfInstanceUpdate.comp", with computeMeanAlbedo (ModelImport.cpp:78-112) as "sceneMeanAlbedo.comp"
// (kernels/scene_sdf.hip; DESIGN.md "SDF instances from the scene")
// the backend has no call that frees an image: a released volume keeps its slot of the texture array with one texel (1 x 1 x 1 R16), for the next bake
static ImageDescription releasedSdfVolume() {
    ImageDescription released;
    released.width = released.height = released.depth = 1;
    released.type = ImageType::Type3D; released.format = ImageFormat::R16_sFloat; released.usageFlags = ImageUsageFlags::Sampled;
    return released;
}

void FramePipeline::removeSceneSdf() {
    if (!m_sceneSdfSet) return;
    m_sceneSdfSet = false;
    m_sceneSdf = PackedSceneSdf{};
    for (BakedVolume& v : m_sceneSdfVolumes)
        if (v.inUse) { m_be.recreateImage(v.image, releasedSdfVolume()); v.inUse = false; v.bytes = 0; }
    m_sdfGi.setInstanceCount(0);
    const uint32_t header[4] = {0, 0, 0, 0}; // the instance count is 0 until the caller uploads again (setSdfScene)
    m_be.setStorageBufferData(m_sdfGi.m_sdfInstanceBuffer, header, sizeof(header));
}

void FramePipeline::setSceneSdf(const uint32_t* sdfTextures, uint32_t meshCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneSdf: a band / tile pipeline cannot rasterise scene meshes, so it has no scene to take SDF instances from (band_raster)");
    if (meshCount == 0) { removeSceneSdf(); return; }
    SceneSdfContext scene;
    scene.positions = m_scenePositionsHost.data(); scene.meshVertexCounts = m_sceneMeshVertexCounts.data(); scene.drawMeshes = m_sceneDrawMeshes.data(); scene.models = m_sceneModel.data();
    scene.meshCount = (uint32_t)m_sceneMeshVertexCounts.size(); scene.drawCount = m_sceneDrawCount; scene.maxInstances = settings.maxSdfInstances;
    PackedSceneSdf packed = packSceneSdf(sdfTextures, meshCount, scene); // validates everything before anything is changed
    // the bakes, into host memory: the asset-pipeline boundary, once per scene (a failure here still changes nothing)
    struct Bake { ImageDescription desc; std::vector<uint16_t> voxels; };
    std::vector<Bake> bakes(packed.bakedMeshes.size());
    int device = 0;
    if (!bakes.empty() && hipGetDevice(&device) != hipSuccess) throw std::runtime_error("setSceneSdf: no current device for the bake");
    std::vector<size_t> vertexOffset(meshCount, 0);
    for (uint32_t m = 1; m < meshCount; m++) vertexOffset[m] = vertexOffset[m - 1] + m_sceneMeshVertexCounts[m - 1];
    for (size_t k = 0; k < bakes.size(); k++) {
        const uint32_t m = packed.bakedMeshes[k];
        plr_aabb bb;
        std::memcpy(bb.min, packed.meshBoxes.data() + (size_t)m * 6u, 12); std::memcpy(bb.max, packed.meshBoxes.data() + (size_t)m * 6u + 3u, 12);
        plr_image_desc cd{};
        if (plr_sdf_texture_description(&bb, &cd) != PLR_OK) throw std::runtime_error(plr_last_error());
        Bake& b = bakes[k];
        b.desc.width = cd.width; b.desc.height = cd.height; b.desc.depth = cd.depth;
        b.desc.type = ImageType::Type3D; b.desc.format = ImageFormat::R16_sFloat; b.desc.usageFlags = ImageUsageFlags::Sampled;
        b.voxels.resize((size_t)cd.width * cd.height * cd.depth);
        const plr_mesh_data mesh{m_scenePositionsHost.data() + vertexOffset[m] * 3u, m_sceneMeshVertexCounts[m], m_sceneIndicesHost.data() + m_sceneMeshFirstIndex[m], m_sceneMeshIndexCounts[m]};
        if (plr_compute_sdf(device, &mesh, &bb, cd.width, cd.height, cd.depth, b.voxels.data(), b.voxels.size() * 2u) != PLR_OK)
            throw std::runtime_error(std::string("setSceneSdf: baking mesh ") + std::to_string(m) + ": " + plr_last_error());
    }
    // the volumes of the SDF that is replaced are released; the new ones take their images first, so that repeated calls do not grow the image count
    std::vector<uint8_t> wasInUse(m_sceneSdfVolumes.size());
    for (size_t v = 0; v < m_sceneSdfVolumes.size(); v++) { wasInUse[v] = m_sceneSdfVolumes[v].inUse; m_sceneSdfVolumes[v].inUse = false; }
    std::vector<uint32_t> meshTextureIndices(packed.meshSdf);
    for (size_t k = 0; k < bakes.size(); k++) {
        const Bake& b = bakes[k];
        const size_t bytes = b.voxels.size() * 2u;
        size_t slot = 0;
        while (slot < m_sceneSdfVolumes.size() && m_sceneSdfVolumes[slot].inUse) slot++;
        if (slot == m_sceneSdfVolumes.size()) {
            BakedVolume v;
            v.image = m_be.createImage(b.desc, b.voxels.data(), bytes);
            m_sceneSdfVolumes.push_back(v);
            wasInUse.push_back(0);
        } else {
            m_be.recreateImage(m_sceneSdfVolumes[slot].image, b.desc);
            if (plr_upload_image(RenderBackend::toC(m_sceneSdfVolumes[slot].image), 0, b.voxels.data(), bytes) != PLR_OK) throw std::runtime_error(plr_last_error());
        }
        m_sceneSdfVolumes[slot].inUse = true; m_sceneSdfVolumes[slot].bytes = bytes;
        meshTextureIndices[packed.bakedMeshes[k]] = m_be.getImageGlobalTextureArrayIndex(m_sceneSdfVolumes[slot].image);
    }
    for (size_t v = 0; v < m_sceneSdfVolumes.size(); v++)
        if (wasInUse[v] && !m_sceneSdfVolumes[v].inUse) { m_be.recreateImage(m_sceneSdfVolumes[v].image, releasedSdfVolume()); m_sceneSdfVolumes[v].bytes = 0; }
    if (!m_sceneSdfPassesCreated) {
        ComputePassDescription d;
        d.name = "SDF instance update";
        d.shaderDescription.srcPathRelative = "sdfInstanceUpdate.comp";
        m_sdfInstanceUpdatePass = m_be.createComputePass(d);
        d.name = "Scene mean albedo";
        d.shaderDescription.srcPathRelative = "sceneMeanAlbedo.comp";
        m_sceneMeanAlbedoPass = m_be.createComputePass(d);
        m_sceneSdfPassesCreated = true;
    }
    const std::vector<uint32_t> table = sceneSdfInstanceTable(packed, m_sceneDrawMeshes.data(), meshTextureIndices.data());
    fillBuffer(m_sceneSdfTable, table.empty() ? nullptr : table.data(), std::max<size_t>(table.size() * sizeof(uint32_t), sizeof(plr::scenesdf::InstanceEntry)));
    const std::vector<float> derive((size_t)m_sceneDrawCount * 3u, std::nanf("")); // no overrides: every draw derives
    fillBuffer(m_sceneSdfOverrides, derive);
    m_sceneSdf = std::move(packed);
    m_sceneSdfSet = true;
    m_sdfGi.setInstanceCount((uint32_t)m_sceneSdf.instanceDraws.size());
    noteSceneTexturesChanged(0);
}

// the mean albedos belong to the texture store and the materials: stale whenever either changed, or the SDF was set. largestLevel0Texels 0: keep the group count
void FramePipeline::noteSceneTexturesChanged(uint32_t largestLevel0Texels) {
    // a group of 256 lanes takes 16 texels per lane and round at least; a texture gets at most 1024 groups (the kernel strides: the result does not depend on it)
    if (largestLevel0Texels) m_sceneSdfMeanGroups = std::min(1024u, std::max(1u, (largestLevel0Texels + 4095u) / 4096u));
    m_sceneSdfMeansStale = true;
    if (!m_sceneSdfSet || m_sceneTextureCount == 0) return;
    fillBuffer(m_sceneSdfMeans, nullptr, (size_t)m_sceneTextureCount * 16u);
    fillBuffer(m_sceneSdfMeanScratch, nullptr, plr::scenesdf::meanScratchBytes(m_sceneTextureCount));
}

void FramePipeline::setSceneSdfMeanAlbedo(const float* rgbOrNan, uint32_t drawCount) {
    if (partitionedWithoutRaster(m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setSceneSdfMeanAlbedo: a band / tile pipeline cannot rasterise scene meshes, so it has no scene SDF (band_raster)");
    if (drawCount == 0) {
        if (!m_sceneSdfSet) return;
        const std::vector<float> derive((size_t)m_sceneDrawCount * 3u, std::nanf(""));
        fillBuffer(m_sceneSdfOverrides, derive);
        return;
    }
    const std::vector<float> values = packSceneSdfMeanAlbedo(rgbOrNan, drawCount, m_sceneDrawCount, m_sceneSdfSet); // validates everything before anything is changed
    fillBuffer(m_sceneSdfOverrides, values);
}

FramePipeline::SceneSdfStats FramePipeline::sceneSdfStats() const {
    SceneSdfStats out;
    out.instances = m_sceneSdfSet ? (uint32_t)m_sceneSdf.instanceDraws.size() : 0u;
    for (const BakedVolume& v : m_sceneSdfVolumes)
        if (v.inUse) { out.volumesBaked++; out.volumeBytes += v.bytes; }
    return out;
}

void FramePipeline::updateSceneSdfInstances() {
    if (!m_sceneSdfSet) return;
    namespace ss = plr::scenesdf;
    const uint32_t textures = m_sceneTextureCount;
    if (textures && m_sceneSdfMeansStale) { // only in a frame after the texture store or the materials changed
        ComputePassExecution exe;
        exe.genericInfo.handle = m_sceneMeanAlbedoPass;
        exe.dispatchCount[0] = m_sceneSdfMeanGroups; exe.dispatchCount[1] = textures; exe.dispatchCount[2] = 1;
        const bool formats = m_sceneTexturesCompressed;
        const ss::MeanPushConstants pc{textures, m_sceneDrawCount, formats ? 1u : 0u};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sceneTextures.handle, true, ss::kMeanTextureBinding), StorageBufferResource(m_sceneTexels.handle, true, ss::kMeanTexelBinding),
                                                    StorageBufferResource(m_sceneMaterials.handle, true, ss::kMeanMaterialBinding),
                                                    StorageBufferResource(m_sceneSdfMeanScratch.handle, false, ss::kMeanScratchBinding),
                                                    StorageBufferResource(m_sceneSdfMeans.handle, false, ss::kMeanOutBinding)};
        if (formats) exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_sceneTextureFormats.handle, true, ss::kMeanFormatBinding));
        m_be.setComputePassExecution(exe);
    }
    m_sceneSdfMeansStale = false;
    const uint32_t instances = (uint32_t)m_sceneSdf.instanceDraws.size();
    ComputePassExecution exe;
    exe.genericInfo.handle = m_sdfInstanceUpdatePass;
    exe.dispatchCount[0] = (std::max(instances, 1u) + 63u) / 64u; exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
    const ss::InstancePushConstants pc{instances, m_sceneDrawCount, textures};
    exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
    exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sceneMatrices.handle, true, ss::kMatricesBinding), StorageBufferResource(m_sceneSdfTable.handle, true, ss::kTableBinding),
                                                StorageBufferResource(m_sceneDraws.handle, true, ss::kDrawBinding), StorageBufferResource(m_sceneSdfOverrides.handle, true, ss::kOverrideBinding),
                                                StorageBufferResource(m_sdfGi.m_sdfInstanceBuffer, false, ss::kInstanceBinding),
                                                StorageBufferResource(m_sdfGi.m_sdfInstanceWorldBBBuffer, false, ss::kWorldBBBinding)};
    if (textures) {
        exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_sceneMaterials.handle, true, ss::kMaterialBinding));
        exe.genericInfo.resources.storageBuffers.push_back(StorageBufferResource(m_sceneSdfMeans.handle, true, ss::kMeanAlbedoBinding));
    }
    m_be.setComputePassExecution(exe);
}

// ---- the frame's noise inputs: generateBlueNoiseTexture (Common/Noise.cpp:232-300; RenderFrontend.cpp:1251-1269) as "blueNoiseVoidAndCluster.comp" and
// generate3DPerlinNoise (Noise.cpp:422-497; Volumetrics.cpp:71-90) as "perlinNoise3D.comp" (kernels/noise.hip; DESIGN.md "Noise textures as compute passes")
void FramePipeline::generateNoise(uint32_t seed, uint32_t flags) {
    namespace nz = plr::noise;
    if (flags == 0 || (flags & ~(kNoiseBlue | kNoisePerlin)) != 0)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "generateNoise: flags are " + std::to_string(flags) + ", they must be PLRF_NOISE_BLUE (1), PLRF_NOISE_PERLIN (2) or both");
    if ((flags & kNoisePerlin) && m_perlinNoise3D.index == invalidIndex)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "generateNoise: PLRF_NOISE_PERLIN on a pipeline that has no perlinNoise3D image");
    // the tables first, in host memory: a failure here still changes nothing
    std::vector<float> gaussian, gradients;
    if (flags & kNoiseBlue) {
        gaussian.resize((size_t)noiseTextureWidth * noiseTextureHeight);
        if (plr_noise_gaussian_table(noiseTextureWidth, noiseTextureHeight, gaussian.data()) != PLR_OK) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, plr_last_error());
    }
    if (flags & kNoisePerlin) {
        gradients.resize((size_t)nz::kPerlinFrameCells * nz::kPerlinFrameCells * nz::kPerlinFrameCells * 4u);
        if (plr_noise_perlin_gradients(seed, nz::kPerlinFrameCells, gradients.data()) != PLR_OK) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, plr_last_error());
    }
    if (!m_noisePassesCreated) {
        ComputePassDescription d;
        d.name = "Blue noise void and cluster";
        d.shaderDescription.srcPathRelative = "blueNoiseVoidAndCluster.comp";
        m_blueNoisePass = m_be.createComputePass(d);
        d.name = "Perlin noise 3D";
        d.shaderDescription.srcPathRelative = "perlinNoise3D.comp";
        m_perlinNoisePass = m_be.createComputePass(d);
        StorageBufferDescription sb;
        sb.size = (size_t)noiseTextureWidth * noiseTextureHeight * sizeof(float);
        m_noiseGaussianTable = m_be.createStorageBuffer(sb);
        sb.size = (size_t)nz::kPerlinFrameCells * nz::kPerlinFrameCells * nz::kPerlinFrameCells * 4u * sizeof(float);
        m_noisePerlinGradients = m_be.createStorageBuffer(sb);
        sb.size = 2u * nz::kBlueStatusWords * sizeof(uint32_t);
        for (StorageBufferHandle& s : m_noiseStatus) s = m_be.createStorageBuffer(sb);
        m_noisePassesCreated = true;
    }
    if (flags & kNoiseBlue) { m_be.setStorageBufferData(m_noiseGaussianTable, gaussian.data(), gaussian.size() * sizeof(float)); m_noiseBlueSeed = seed; }
    if (flags & kNoisePerlin) m_be.setStorageBufferData(m_noisePerlinGradients, gradients.data(), gradients.size() * sizeof(float));
    m_noisePending |= flags;
}

void FramePipeline::recordNoiseGeneration() {
    if (m_noisePending == 0) return;
    namespace nz = plr::noise;
    if (m_noisePending & kNoiseBlue)
        for (uint32_t t = 0; t < 4; t++) { // texture t: streams 2 t (red) and 2 t + 1 (green)
            ComputePassExecution exe;
            exe.genericInfo.handle = m_blueNoisePass;
            exe.genericInfo.resources.storageImages = {ImageResource(m_noiseTextures[t], 0, nz::kBlueImageBinding)};
            exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_noiseGaussianTable, true, nz::kBlueTableBinding),
                                                        StorageBufferResource(m_noiseStatus[t], false, nz::kBlueStatusBinding)};
            const nz::BluePushConstants pc{m_noiseBlueSeed, 2u * t};
            exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
            exe.dispatchCount[0] = 2; exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
            m_be.setComputePassExecution(exe);
        }
    if (m_noisePending & kNoisePerlin) {
        const ImageDescription nd = m_be.getImageDescription(m_perlinNoise3D);
        ComputePassExecution exe;
        exe.genericInfo.handle = m_perlinNoisePass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_perlinNoise3D, 0, nz::kPerlinImageBinding)};
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_noisePerlinGradients, true, nz::kPerlinGradientBinding)};
        const nz::PerlinPushConstants pc{nz::kPerlinFrameCells};
        exe.pushConstants = dataToCharArray(&pc, sizeof(pc));
        exe.dispatchCount[0] = (nd.width * nd.height * nd.depth + nz::kPerlinThreads - 1u) / nz::kPerlinThreads; exe.dispatchCount[1] = exe.dispatchCount[2] = 1;
        m_be.setComputePassExecution(exe);
    }
    m_noisePending = 0;
}

FramePipeline::NoiseStats FramePipeline::noiseStats() {
    NoiseStats out;
    if (!m_noisePassesCreated) return out;
    for (uint32_t t = 0; t < 4; t++)
        if (plr_download_storage_buffer(m_noiseStatus[t].index, out.status[t], 0, sizeof(out.status[t])) != PLR_OK) throw std::runtime_error(plr_last_error());
    return out;
}

PrepassRasterStats FramePipeline::prepassRasterStats() {
    PrepassRasterStats out;
    if (m_sceneDrawCount == 0 || !m_sceneRecorded) return out; // no scene, or no frame since it was set: the scratch header is not this scene's
    plr::prepass::ScratchHeader h{};
    if (plr_download_storage_buffer(m_sceneScratch.handle.index, &h, 0, sizeof(h)) != PLR_OK) throw std::runtime_error(plr_last_error());
    out.trianglesSubmitted = h.submitted; out.trianglesClipped = h.clipped; out.subtrianglesDrawn = h.drawn; out.rejects = h.rejects;
    return out;
}

void FramePipeline::computeVolumetricLighting(float deltaTime) { // Volumetrics::computeVolumetricLighting, Techniques/Volumetrics.cpp:119-243
    m_volumetricsState.sampleOffset = radicalInverseBase2((uint32_t)m_frameIndex.mod8()) - 0.5f; // hammersley2D(frameIndexMod8).x - 0.5
    for (int i = 0; i < 3; i++) m_volumetricsState.windSampleOffset[i] += windSettings.vector[i] * windSettings.speed * deltaTime;
    VolumetricsBufferContents contents;
    contents.state = m_volumetricsState;
    contents.settings = volumetricsSettings;
    m_be.setUniformBufferData(m_volumetricsInfoBuffer, &contents, sizeof(contents));
    const ImageDescription md = m_be.getImageDescription(m_volumeMaterialVolume);
    auto groups = [&](ComputePassExecution& exe, float groupSize, bool flat) {
        exe.dispatchCount[0] = (uint32_t)std::ceil(md.width / groupSize);
        exe.dispatchCount[1] = (uint32_t)std::ceil(md.height / groupSize);
        exe.dispatchCount[2] = flat ? 1u : (uint32_t)std::ceil(md.depth / groupSize);
    };
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_froxelVolumeMaterialPass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_volumeMaterialVolume, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_perlinNoise3D, 0, 1)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 2)};
        groups(exe, 4.f, false);
        m_be.setComputePassExecution(exe);
    }
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_froxelScatteringTransmittancePass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_scatteringTransmittanceVolume, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_shadowMaps[settings.shading.sunShadowCascadeCount - 1], 0, 1), ImageResource(m_volumeMaterialVolume, 0, 2)};
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_sunShadowInfoBuffer, true, 3), StorageBufferResource(m_lightBuffer, true, 4)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 5)};
        groups(exe, 4.f, false);
        m_be.setComputePassExecution(exe);
    }
    const size_t frameIndexMod2 = m_frameIndex.mod2();
    const ImageHandle reprojectionTarget = m_volumetricLightingHistory[frameIndexMod2];
    const ImageHandle reprojectionHistory = m_volumetricLightingHistory[(frameIndexMod2 + 1) % 2];
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_volumetricLightingReprojection;
        exe.genericInfo.resources.storageImages = {ImageResource(reprojectionTarget, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_scatteringTransmittanceVolume, 0, 1), ImageResource(reprojectionHistory, 0, 2)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 3)};
        groups(exe, 4.f, false);
        m_be.setComputePassExecution(exe);
    }
    {
        ComputePassExecution exe;
        exe.genericInfo.handle = m_volumetricLightingIntegration;
        exe.genericInfo.resources.storageImages = {ImageResource(m_volumetricIntegrationVolume, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(reprojectionTarget, 0, 1)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_volumetricsInfoBuffer, 2)};
        groups(exe, 8.f, true);
        m_be.setComputePassExecution(exe);
    }
}

void FramePipeline::updateTransmissionLut() { // Sky::updateTransmissionLut, Techniques/Sky.cpp:260-272
    const uint32_t res = 128;
    ComputePassExecution exe;
    exe.genericInfo.handle = m_skyTransmissionLutPass;
    exe.genericInfo.resources.storageImages = {ImageResource(m_transmissionLut, 0, 0)};
    exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_atmosphereSettingsBuffer, 1)};
    exe.dispatchCount[0] = res / 8; exe.dispatchCount[1] = res / 8; exe.dispatchCount[2] = 1;
    m_be.setComputePassExecution(exe);
}

void FramePipeline::updateSkyLut() { // Sky::updateSkyLut, Techniques/Sky.cpp:274-316
    m_be.setUniformBufferData(m_atmosphereSettingsBuffer, &atmosphereSettings, sizeof(atmosphereSettings));
    {
        const uint32_t res = 32;
        ComputePassExecution exe;
        exe.genericInfo.handle = m_skyMultiscatterLutPass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_skyMultiscatterLut, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_transmissionLut, 0, 1)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_atmosphereSettingsBuffer, 3)};
        exe.dispatchCount[0] = res / 8; exe.dispatchCount[1] = res / 8; exe.dispatchCount[2] = 1;
        m_be.setComputePassExecution(exe);
    }
    {
        const uint32_t w = 200, h = 100; // sic: 100 / 8 = 12 workgroups, the last four rows of the LUT are never written (Sky.cpp:311-312)
        ComputePassExecution exe;
        exe.genericInfo.handle = m_skyLutPass;
        exe.genericInfo.resources.storageImages = {ImageResource(m_skyLut, 0, 0)};
        exe.genericInfo.resources.sampledImages = {ImageResource(m_transmissionLut, 0, 1), ImageResource(m_skyMultiscatterLut, 0, 2)};
        exe.genericInfo.resources.uniformBuffers = {UniformBufferResource(m_atmosphereSettingsBuffer, 4)};
        exe.genericInfo.resources.storageBuffers = {StorageBufferResource(m_lightBuffer, true, 5)};
        exe.dispatchCount[0] = w / 8; exe.dispatchCount[1] = h / 8; exe.dispatchCount[2] = 1;
        m_be.setComputePassExecution(exe);
    }
}

void FramePipeline::computeBRDFLut() { // RenderFrontend.cpp:1031-1042
    ComputePassExecution exe;
    exe.genericInfo.handle = m_brdfLutPass;
    exe.genericInfo.resources.storageImages = {ImageResource(m_brdfLut, 0, 0)};
    dispatch8(exe, settings.brdfLutRes, settings.brdfLutRes);
    m_be.setComputePassExecution(exe);
}

RowRange FramePipeline::bandRows(uint32_t halo, uint32_t divisor) const {
    if (!settings.band.enabled()) return {};
    const uint32_t lo = settings.band.rowBegin > halo ? settings.band.rowBegin - halo : 0;
    const uint32_t hi = std::min(settings.band.rowEnd + halo, settings.height);
    return {lo / divisor, (hi + divisor - 1) / divisor};
}

ColRange FramePipeline::bandCols(uint32_t halo, uint32_t divisor) const {
    if (!settings.band.enabled() || !settings.band.tiled()) return {};
    const uint32_t lo = settings.band.colBegin > halo ? settings.band.colBegin - halo : 0;
    const uint32_t hi = std::min(settings.band.colEnd + halo, settings.width);
    return {lo / divisor, (hi + divisor - 1) / divisor};
}

void FramePipeline::addExchangeItem(int id, ImageHandle image, uint32_t divisor, uint32_t haloRows) {
    const ImageDescription d = m_be.getImageDescription(image);
    ExchangeItem it;
    it.image = image;
    it.rowBegin = settings.band.rowBegin / divisor;
    it.rowEnd = std::min((settings.band.rowEnd + divisor - 1) / divisor, d.height);
    it.haloRows = haloRows;
    it.imageRows = d.height;
    size_t bytes = 0;
    void* ptr = nullptr;
    m_be.getImageDevicePointer(image, 0, &ptr, &bytes);
    it.rowBytes = (uint32_t)(bytes / d.height);
    it.imageCols = d.width;
    it.texelBytes = it.rowBytes / std::max(d.width, 1u);
    it.colBegin = settings.band.tiled() ? settings.band.colBegin / divisor : 0u;
    it.colEnd = settings.band.tiled() ? std::min((settings.band.colEnd + divisor - 1) / divisor, d.width) : d.width;
    m_exchangeItems[id].push_back(it);
}

int FramePipeline::exchangeTrampoline(void* user, void* stream) {
    const ExchangeCtx* ctx = (const ExchangeCtx*)user;
    return ctx->self->m_exchangeFn ? ctx->self->m_exchangeFn(ctx->self->m_exchangeUser, ctx->id, stream) : 0;
}

void FramePipeline::exchangePoint(int id, const char* label) {
    // id may carry a phase (ExchangeBegin / ExchangeEnd)
    const int phase = (id & ExchangeBegin) ? 1 : ((id & ExchangeEnd) ? 2 : 0);
    if (!m_exchangeFn) return;
    // what the exchange moves: the registered images' halo rows, or the histogram buffer (the backend orders the frame's asynchronous tail by it)
    std::vector<ImageHandle> images;
    std::vector<StorageBufferHandle> buffers;
    if ((id & ExchangeIdMask) == ExchangeHistogram) buffers.push_back(m_histogramBuffer);
    else if ((id & ExchangeIdMask) == ExchangeGiRequests) { buffers.push_back(m_sdfGi.m_giRequestBitmap[0]); buffers.push_back(m_sdfGi.m_giRequestBitmap[1]); }
    else for (const ExchangeItem& it : m_exchangeItems[id & ExchangeIdMask]) images.push_back(it.image);
    if (settings.band.giRequested && ((id & ExchangeIdMask) == ExchangeGiTrace || (id & ExchangeIdMask) == ExchangeGiTemporal)) {
        images.push_back(m_depthHalfRes); // the requested texels arrive with their depth
        buffers.push_back(m_sdfGi.m_giRequestBitmap[(id & ExchangeIdMask) == ExchangeGiTrace ? 0 : 1]);
    }
    m_be.setHostCallbackExecution(&FramePipeline::exchangeTrampoline, &m_exchangeCtx[phase * ExchangeCount + (id & ExchangeIdMask)], label, images, buffers);
}

void FramePipeline::prepareRenderpasses() { // RenderFrontend.cpp:313-406
    const FrameRenderTargets previousRenderTarget = m_frameRenderTargets[m_sceneRenderTargetIndex];
    m_sceneRenderTargetIndex = (m_sceneRenderTargetIndex + 1) % 2;
    const FrameRenderTargets currentRenderTarget = m_frameRenderTargets[m_sceneRenderTargetIndex];

    recordNoiseGeneration(); // only in the frame after generateNoise: in front of everything else
    recordTextureBuild();    // only in the frame after buildSceneTextures: likewise
    const bool bandMode = settings.band.enabled();
    if (settings.sdfDebug.visualisationMode != SDFVisualisationMode::None) { // RenderFrontend.cpp:321-340
        if (bandMode) throw std::runtime_error("the SDF debug visualisation is not supported in band rendering");
        for (auto& items : m_exchangeItems) items.clear();
        renderDepthPrepass(currentRenderTarget); // (RenderFrontend.cpp:322) only with scene meshes set; the uploaded G-buffer otherwise
        computeDepthPyramid(currentRenderTarget.depthBuffer);
        computeColorBufferHistogram(m_postProcessBuffers[0]);
        if (settings.runSkyLuts) updateTransmissionLut();
        computeExposure();
        if (settings.runSkyLuts) updateSkyLut();
        if (settings.runLightMatrix) computeSunLightMatrices();
        renderSunShadowCascades(); // (RenderFrontend.cpp:331) only with mesh casters set; the uploaded maps otherwise
        updateSceneSdfInstances(); // (SDFGI::updateSDFScene, called from renderScene every frame) only with a scene SDF set; the uploaded instances otherwise
        SDFTraceDependencies deps = m_frustumScratch;
        deps.currentFrame = currentRenderTarget;
        deps.previousFrame = previousRenderTarget;
        deps.depthHalfRes = m_depthHalfRes;
        deps.worldSpaceNormals = m_worldSpaceNormalImage;
        deps.skyLut = m_skyLut;
        deps.shadowMap = m_shadowMaps[settings.shading.sunShadowCascadeCount - 1];
        deps.lightBuffer = m_lightBuffer;
        deps.sunShadowInfoBuffer = m_sunShadowInfoBuffer;
        deps.depthMinMaxPyramid = m_minMaxDepthPyramid;
        m_sdfGi.renderSDFVisualization(m_be, m_postProcessBuffers[0], deps, settings.sdfDebug, settings.sdfTrace);
        computeTonemapping(m_postProcessBuffers[0]);
        return;
    }
    if (m_isBRDFLutShaderDescriptionStale) {
        computeBRDFLut();
        m_isBRDFLutShaderDescriptionStale = false;
    }
    const bool band = settings.band.enabled();
    for (auto& items : m_exchangeItems) items.clear();
    if (settings.runExposure) {
        computeColorBufferHistogram(previousRenderTarget.colorBuffer);
        if (band) exchangePoint(ExchangeHistogram, "Exchange: histogram all-reduce");
        if (settings.runSkyLuts) updateTransmissionLut(); // separate from the sky LUT: the exposure pass reads it, the other LUTs depend on the exposure
        computeExposure();
    } else if (settings.runSkyLuts) updateTransmissionLut();
    if (settings.runSkyLuts) updateSkyLut();
    renderDepthPrepass(currentRenderTarget); // (RenderFrontend.cpp:351) only with scene meshes set; the uploaded G-buffer otherwise
    if (settings.runHiZ) computeDepthPyramid(currentRenderTarget.depthBuffer);
    if (settings.runLightMatrix && settings.runHiZ) {
        if (perTilePyramid(settings)) computeDepthApexOfTiles(); // no apex in a per-tile pyramid: reduce (and, across bands, all-reduce) it
        computeSunLightMatrices();
    }
    renderSunShadowCascades(); // (RenderFrontend.cpp:354) only with mesh casters set; the uploaded maps otherwise
    bool sceneSdfUpdated = false; // this frame records "sdfInstanceUpdate.comp": what the debug geometry's SDF boxes need
    if (settings.runGI && settings.shading.indirectLightingTech == IndirectLightingTech::SDFTrace) {
        if (settings.sdfTrace.halfResTrace) downscaleDepth(currentRenderTarget);
        updateSceneSdfInstances(); // in front of sdfCameraFrustumCulling; only with a scene SDF set, the uploaded instances otherwise
        sceneSdfUpdated = m_sceneSdfSet;
        SDFTraceDependencies deps = m_frustumScratch; // frustum points/normals from setCameraExtrinsic (fillOutSdfGiDependencies, :1073-1090)
        deps.currentFrame = currentRenderTarget;
        deps.previousFrame = previousRenderTarget;
        deps.depthHalfRes = m_depthHalfRes;
        deps.worldSpaceNormals = m_worldSpaceNormalImage;
        deps.skyLut = m_skyLut;
        deps.shadowMap = m_shadowMaps[settings.shading.sunShadowCascadeCount - 1];
        deps.lightBuffer = m_lightBuffer;
        deps.sunShadowInfoBuffer = m_sunShadowInfoBuffer;
        deps.depthMinMaxPyramid = m_minMaxDepthPyramid;
        if (band) {
            const uint32_t div = settings.sdfTrace.halfResTrace ? 2 : 1;
            GiBand gb;
            gb.traceRows = bandRows(0, div);
            gb.upscaleRows = bandRows(settings.band.colorHalo);
            gb.traceCols = bandCols(0, div);
            gb.upscaleCols = bandCols(settings.band.colorHalo);
            gb.user = this;
            gb.giHalo = settings.band.giHalo; gb.giHistoryHalo = settings.band.giHistoryHalo;
            gb.rowsFirst = settings.band.rowsFirst;
            gb.requested = settings.band.giRequested;
            // registers the images of a GI exchange and records its callback: phase 0 = whole exchange, ExchangeBegin after the producer's
            // edge rows, ExchangeEnd (items already registered) before the consumer
            static const auto giExchange = [](FramePipeline* self, int id, int phase) {
                const SDFGI& gi = self->m_sdfGi;
                const uint32_t d = self->settings.sdfTrace.halfResTrace ? 2 : 1;
                const BandSettings& b = self->settings.band;
                const bool reg = phase != ExchangeEnd;
                const char* what = phase == ExchangeBegin ? " (start)" : (phase == ExchangeEnd ? " (wait)" : "");
                if (id == ExchangeGiRequests) {
                    self->exchangePoint(id, "Exchange: GI sample requests");
                } else if (id == ExchangeGiTrace) {
                    if (reg) { self->addExchangeItem(id, gi.m_indirectDiffuse_Y_SH[0], d, b.giHalo); self->addExchangeItem(id, gi.m_indirectDiffuse_CoCg[0], d, b.giHalo); }
                    self->exchangePoint(id | phase, (std::string("Exchange: traced GI halo rows") + what).c_str());
                } else if (id == ExchangeGiTemporal) {
                    if (reg) { self->addExchangeItem(id, gi.m_indirectDiffuseHistory_Y_SH[1], d, b.giHalo); self->addExchangeItem(id, gi.m_indirectDiffuseHistory_CoCg[1], d, b.giHalo); }
                    self->exchangePoint(id | phase, (std::string("Exchange: temporally filtered GI halo rows") + what).c_str());
                } else {
                    if (reg) { self->addExchangeItem(id, gi.m_indirectDiffuseHistory_Y_SH[0], d, b.giHistoryHalo); self->addExchangeItem(id, gi.m_indirectDiffuseHistory_CoCg[0], d, b.giHistoryHalo); }
                    self->exchangePoint(id | phase, (std::string("Exchange: GI history halo rows") + what).c_str());
                }
            };
            const bool overlap = settings.band.overlapExchange && m_exchangeFn && !settings.band.giRequested; // (a requested texel can be anywhere in its owner's rectangle: no edges-first producers)
            if (settings.band.giRequested && settings.band.overlapExchange && m_exchangeFn) {
                gb.requestedBegin = [](void* user, int id) { giExchange((FramePipeline*)user, id, ExchangeBegin); };
                gb.requestedEnd = [](void* user, int id) { giExchange((FramePipeline*)user, id, ExchangeEnd); };
            }
            if (overlap) {
                gb.exchangeBegin = [](void* user, int id) { giExchange((FramePipeline*)user, id, ExchangeBegin); };
                gb.exchangePoint = [](void* user, int id) { giExchange((FramePipeline*)user, id, ExchangeEnd); };
                gb.exchangeWhole = [](void* user, int id) { giExchange((FramePipeline*)user, id, 0); };
            } else gb.exchangePoint = [](void* user, int id) { giExchange((FramePipeline*)user, id, 0); };
            m_sdfGi.computeIndirectLighting(m_be, m_frameIndex, deps, settings.sdfTrace, &gb);
        } else m_sdfGi.computeIndirectLighting(m_be, m_frameIndex, deps, settings.sdfTrace);
    }
    if (settings.runVolumetrics) {
        if (band) throw std::runtime_error("the volumetric froxel passes are not supported in band rendering");
        computeVolumetricLighting(m_lastDeltaTime);
    }
    if (settings.runShading) computeDeferredShading(currentRenderTarget.colorBuffer, currentRenderTarget);
    // renderDebugGeometry (RenderFrontend.cpp:373-385): behind the shade, in front of the sky and of everything else that reads the colour buffer
    if (settings.runShading && m_debugFlags != 0) recordDebugGeometry(currentRenderTarget, sceneSdfUpdated);
    // renderSky (RenderFrontend.cpp:691-694, Techniques/Sky.cpp:318-353): the deferred pass writes the plain sky LUT colour on depth == 0 pixels; with runSky
    // the sky pass overwrites those pixels with the dithered, in-scattered sky and the sun disc before anything else reads the colour buffer
    if (settings.runShading && settings.runSky) computeSkyAndSunSprite(currentRenderTarget.colorBuffer, currentRenderTarget);
    ImageHandle currentSrc = currentRenderTarget.colorBuffer;
    bool postExchangeStarted = false;
    if (settings.runTAA && settings.taa.enabled) {
        if (settings.taa.useSeparateSupersampling) { // RenderFrontend.cpp:391-395 (whole-frame only: the stage has no halo plan for band rendering)
            if (band) throw std::runtime_error("useSeparateSupersampling is not supported in band rendering");
            m_taa.computeTemporalSuperSampling(m_be, m_frameIndex, currentRenderTarget, previousRenderTarget, m_postProcessBuffers[0]);
            currentSrc = m_postProcessBuffers[0];
        }
        // the bloom chain reads postHalo rows around the band; next frame's temporal filter reprojects into the history image
        const bool bloomOn = settings.runBloom && settings.bloom.enabled;
        if (band && settings.band.overlapExchange && m_exchangeFn) {
            const uint32_t edge = bloomOn ? std::max(settings.band.postHalo, settings.band.taaHistoryHalo) : settings.band.taaHistoryHalo;
            m_taa.computeTemporalFilter(m_be, m_frameIndex, currentSrc, currentRenderTarget, m_postProcessBuffers[1], bandRows(0), edge, [&] {
                if (bloomOn) addExchangeItem(ExchangePost, m_postProcessBuffers[1], 1, settings.band.postHalo);
                addExchangeItem(ExchangePost, m_taa.historyDst(m_frameIndex), 1, settings.band.taaHistoryHalo);
                exchangePoint(ExchangePost | ExchangeBegin, "Exchange: resolved colour halo rows (start)");
            }, settings.band.rowsFirst, bandCols(0));
            postExchangeStarted = true;
        } else m_taa.computeTemporalFilter(m_be, m_frameIndex, currentSrc, currentRenderTarget, m_postProcessBuffers[1], bandRows(0), 0, nullptr, false, bandCols(0));
        currentSrc = m_postProcessBuffers[1];
    }
    if (band) {
        if (postExchangeStarted) exchangePoint(ExchangePost | ExchangeEnd, "Exchange: resolved colour halo rows (wait)");
        else {
            if (settings.runBloom && settings.bloom.enabled) addExchangeItem(ExchangePost, currentSrc, 1, settings.band.postHalo);
            if (settings.runTAA && settings.taa.enabled) addExchangeItem(ExchangePost, m_taa.historyDst(m_frameIndex), 1, settings.band.taaHistoryHalo);
            if (!m_exchangeItems[ExchangePost].empty()) exchangePoint(ExchangePost, "Exchange: resolved colour halo rows");
        }
    }
    // the bloom chain and the tonemap are the frame's asynchronous tail (plr.h async_tail): nothing reads their outputs before the next frame's TAA
    // resolve, and their ten short launches leave the chip mostly idle - they run beside the next frame's exposure / GI / shade passes. In band
    // rendering too: the exchange callbacks are recorded with the images they move (exchangePoint), and only the resolved-colour exchange shares one.
    if (settings.runBloom && settings.bloom.enabled) m_bloom.computeBloom(m_be, currentSrc, settings.bloom, bandRows(settings.band.postHalo), bandRows(0), asyncPostTail(), bandCols(settings.band.postHalo), bandCols(0));
    if (settings.runTonemap) computeTonemapping(currentSrc);
}

// ViewFrustum.cpp:4-52 + the packing of SDFGI.cpp:543-566 (top, bot, near, far, left, right)
static void computeFrustum(const CameraExtrinsic& e, const CameraIntrinsic& in, float points[6][4], float normals[6][4]) {
    const Vec3 nearC = e.position + e.forward * in.near, farC = e.position + e.forward * in.far;
    const float tanFoV = std::tan(in.fov * 3.14159265358979f / 180.f * 0.5f);
    const float hn = tanFoV * in.near, hf = tanFoV * in.far, wn = hn * in.aspectRatio, wf = hf * in.aspectRatio;
    const Vec3 r_u_f = farC + e.up * hf + e.right * wf, l_u_f = farC + e.up * hf - e.right * wf, r_l_f = farC - e.up * hf + e.right * wf, l_l_f = farC - e.up * hf - e.right * wf;
    const Vec3 r_u_n = nearC + e.up * hn + e.right * wn, l_u_n = nearC + e.up * hn - e.right * wn, r_l_n = nearC - e.up * hn + e.right * wn, l_l_n = nearC - e.up * hn - e.right * wn;
    const Vec3 top = normalize(cross(r_u_f - r_u_n, r_u_n - l_u_n)), bot = normalize(cross(r_l_n - l_l_n, r_l_f - r_l_n));
    const Vec3 right = normalize(cross(r_u_n - r_l_n, r_l_f - r_l_n)), left = normalize(cross(l_l_f - l_l_n, l_u_n - l_l_n));
    const Vec3 nearN = normalize(cross(r_u_n - r_l_n, r_l_n - l_l_n)), farN = normalize(cross(r_l_f - l_l_f, r_u_f - r_l_f));
    const Vec3 P[6] = {l_u_f, l_l_f, l_l_n, l_l_f, l_l_f, r_l_f};
    const Vec3 N[6] = {top, bot, nearN, farN, left, right};
    for (int i = 0; i < 6; i++) {
        points[i][0] = P[i].x; points[i][1] = P[i].y; points[i][2] = P[i].z; points[i][3] = 0.f;
        normals[i][0] = N[i].x; normals[i][1] = N[i].y; normals[i][2] = N[i].z; normals[i][3] = 0.f;
    }
}

void FramePipeline::setCameraExtrinsic(const CameraExtrinsic& extrinsic) { // RenderFrontend.cpp:423-454
    m_globalShaderInfo.previousFrameCameraJitter[0] = m_globalShaderInfo.currentFrameCameraJitter[0];
    m_globalShaderInfo.previousFrameCameraJitter[1] = m_globalShaderInfo.currentFrameCameraJitter[1];
    m_cameraExtrinsic = extrinsic;
    const Mat4 viewMatrix = viewMatrixFromCameraExtrinsic(extrinsic);
    Mat4 projectionMatrix = projectionMatrixFromCameraIntrinsic(m_cameraIntrinsic);
    if (settings.taa.enabled) {
        float jitterInPixels[2];
        m_taa.jitterInPixels(m_frameIndex, jitterInPixels);
        m_taa.updateTaaResolveWeights(m_be, jitterInPixels);
        // keep a copy for tests: same arithmetic as updateTaaResolveWeights
        {
            int index = 0; float total = 0.f;
            for (int y = -1; y <= 1; y++)
                for (int x = -1; x <= 1; x++) {
                    const float dx = jitterInPixels[0] - (float)x, dy = jitterInPixels[1] - (float)y;
                    const float d = std::sqrt(dx * dx + dy * dy);
                    m_lastWeights[index] = std::exp(-2.29f * d * d);
                    total += m_lastWeights[index++];
                }
            for (float& w : m_lastWeights) w /= total;
        }
        m_globalShaderInfo.currentFrameCameraJitter[0] = jitterInPixels[0] * (1.f / settings.width);
        m_globalShaderInfo.currentFrameCameraJitter[1] = jitterInPixels[1] * (1.f / settings.height);
        // TAA::applyProjectionMatrixJitter: projection[2][0..1] = offset (TAA.cpp:172-179)
        projectionMatrix.m[2 * 4 + 0] = m_globalShaderInfo.currentFrameCameraJitter[0];
        projectionMatrix.m[2 * 4 + 1] = m_globalShaderInfo.currentFrameCameraJitter[1];
    } else {
        m_globalShaderInfo.currentFrameCameraJitter[0] = m_globalShaderInfo.currentFrameCameraJitter[1] = 0.f;
    }
    m_globalShaderInfo.viewProjectionPrevious = m_globalShaderInfo.viewProjection;
    m_globalShaderInfo.viewProjection = mul(projectionMatrix, viewMatrix);
    computeFrustum(extrinsic, m_cameraIntrinsic, m_frustumScratch.frustumPoints, m_frustumScratch.frustumNormals); // updateCameraFrustum
}

void FramePipeline::updateGlobalShaderInfo(float deltaTime, float time) { // RenderFrontend.cpp:1158-1184
    GlobalShaderInfo& g = m_globalShaderInfo;
    std::memcpy(g.cameraPosPrevious, g.cameraPos, sizeof(g.cameraPos));
    g.cameraPos[0] = m_cameraExtrinsic.position.x; g.cameraPos[1] = m_cameraExtrinsic.position.y; g.cameraPos[2] = m_cameraExtrinsic.position.z; g.cameraPos[3] = 1.f;
    g.deltaTime = deltaTime;
    g.time = time;
    g.nearPlane = m_cameraIntrinsic.near;
    g.farPlane = m_cameraIntrinsic.far;
    const Vec3 r = m_cameraExtrinsic.right, u = m_cameraExtrinsic.up, f = m_cameraExtrinsic.forward;
    g.cameraRight[0] = r.x; g.cameraRight[1] = r.y; g.cameraRight[2] = r.z; g.cameraRight[3] = 0.f;
    g.cameraUp[0] = u.x; g.cameraUp[1] = u.y; g.cameraUp[2] = u.z; g.cameraUp[3] = 0.f;
    std::memcpy(g.cameraForwardPrevious, g.cameraForward, sizeof(g.cameraForward));
    g.cameraForward[0] = f.x; g.cameraForward[1] = f.y; g.cameraForward[2] = f.z; g.cameraForward[3] = 0.f;
    g.cameraTanFovHalf = std::tan(m_cameraIntrinsic.fov * 3.14159265358979f / 180.f * 0.5f);
    g.cameraAspectRatio = m_cameraIntrinsic.aspectRatio;
    g.screenResolution[0] = (int32_t)settings.width; g.screenResolution[1] = (int32_t)settings.height;
    const float lodBiasSampleRadius = 0.5f;
    g.mipBias = settings.taa.enabled && settings.taa.useMipBias ? std::log2(lodBiasSampleRadius) : 0.f;
    m_be.setUniformBufferData(m_globalUniformBuffer, &g, sizeof(g));
    m_submittedGlobals = g;
}

// ------------------------------------------------------------------ live changes (RenderFrontend::setResolution, the UI's stale flags)
static bool sameTaa(const TAASettings& a, const TAASettings& b) {
    return a.enabled == b.enabled && a.useSeparateSupersampling == b.useSeparateSupersampling && a.useClipping == b.useClipping &&
           a.useMotionVectorDilation == b.useMotionVectorDilation && a.historySamplingTech == b.historySamplingTech &&
           a.supersampleUseTonemapping == b.supersampleUseTonemapping && a.filterUseTonemapping == b.filterUseTonemapping && a.useMipBias == b.useMipBias;
}
static bool sameShading(const ShadingConfig& a, const ShadingConfig& b) {
    return a.diffuseBRDF == b.diffuseBRDF && a.directMultiscatter == b.directMultiscatter && a.indirectLightingTech == b.indirectLightingTech &&
           a.useGeometryAA == b.useGeometryAA && a.sunShadowCascadeCount == b.sunShadowCascadeCount;
}
static bool sameDebug(const SDFDebugSettings& a, const SDFDebugSettings& b) {
    return a.visualisationMode == b.visualisationMode && a.showCameraTileUsageWithHiZ == b.showCameraTileUsageWithHiZ && a.useInfluenceRadiusForDebug == b.useInfluenceRadiusForDebug;
}
// the first field updateSettings may not change that differs, or null: everything but the live settings (TAA, bloom, SDF trace / debug, shading config
// without the cascade count) and the resolution
static const char* fixedFieldChanged(const FramePipelineSettings& a, const FramePipelineSettings& b) {
    if (a.shadowMapRes != b.shadowMapRes) return "shadow_map_res";
    if (a.brdfLutRes != b.brdfLutRes) return "brdf_lut_res";
    if (a.maxSdfInstances != b.maxSdfInstances) return "max_sdf_instances";
    if (a.froxelDepth != b.froxelDepth) return "froxel_depth";
    if (a.shading.sunShadowCascadeCount != b.shading.sunShadowCascadeCount) return "sun_shadow_cascade_count";
    if (a.sdfTrace.additionalSunShadowMapPadding != b.sdfTrace.additionalSunShadowMapPadding) return "additional sun shadow map padding";
    if (a.runExposure != b.runExposure || a.runHiZ != b.runHiZ || a.runGI != b.runGI || a.runShading != b.runShading || a.runTAA != b.runTAA || a.runBloom != b.runBloom ||
        a.runTonemap != b.runTonemap || a.runLightMatrix != b.runLightMatrix || a.runVolumetrics != b.runVolumetrics || a.runSkyLuts != b.runSkyLuts ||
        a.runSky != b.runSky)
        return "run_*";
    if (a.volumetricsMaxDistance != b.volumetricsMaxDistance) return "volumetrics_max_distance";
    const BandSettings &x = a.band, &y = b.band;
    if (x.rowBegin != y.rowBegin || x.rowEnd != y.rowEnd || x.colBegin != y.colBegin || x.colEnd != y.colEnd || x.giHalo != y.giHalo || x.giRequested != y.giRequested ||
        x.giHistoryHalo != y.giHistoryHalo || x.colorHalo != y.colorHalo || x.postHalo != y.postHalo || x.taaHistoryHalo != y.taaHistoryHalo ||
        x.overlapExchange != y.overlapExchange || x.rowsFirst != y.rowsFirst || x.raster != y.raster)
        return "band_*";
    return nullptr;
}

void FramePipeline::setResolution(uint32_t width, uint32_t height) { // RenderFrontend.cpp:408-421
    if (m_requestedSettings.band.enabled() || m_requestedSettings.band.tiled())
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "setResolution: a band / tile pipeline cannot change size (its exchange plan follows the frame size)");
    m_targetWidth = width; m_targetHeight = height;
    m_minimized = width == 0 || height == 0;
    if (!m_minimized) m_resolutionChanged = true;
}

void FramePipeline::updateSettings(const FramePipelineSettings& n) {
    if (m_requestedSettings.band.enabled() || m_requestedSettings.band.tiled())
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, "updateSettings: a band / tile pipeline cannot change its settings");
    if (n.width != m_targetWidth || n.height != m_targetHeight)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "updateSettings: width / height differ from the current resolution (resize with setResolution)");
    if (const char* field = fixedFieldChanged(n, m_requestedSettings))
        throw FramePipelineRefusal(PLR_ERR_UNSUPPORTED, std::string("updateSettings: ") + field + " is fixed for the pipeline's lifetime");
    m_pendingSettings = n;
    m_settingsChanged = true;
}

void FramePipeline::applyPendingChanges() { // RenderFrontend::prepareNewFrame, RenderFrontend.cpp:199-264
    if (m_resolutionChanged && !m_minimized) { // (a size recorded before a minimize is applied with the next non-zero size)
        applyResolution(m_targetWidth, m_targetHeight);
        m_resolutionChanged = false;
    }
    if (m_minimized) return; // (:229) what the UI changed stays pending
    if (m_settingsChanged) {
        applySettings(m_pendingSettings);
        m_settingsChanged = false;
    }
}

// RenderFrontend.cpp:199-222 with TAA::resizeImages, Volumetrics::resizeTextures (Volumetrics.cpp:123-133) and SDFGI::resize. Every image and buffer the constructor
// sizes from the screen is re-created as the constructor creates it (zero-filled); what does not follow the screen - the light buffer, the frame counters, the
// SDF volumes and scene, the BRDF LUT, shadow maps, sky LUTs, noise textures - is left as it is.
void FramePipeline::applyResolution(uint32_t W, uint32_t H) {
    // (before the first frame there is no history to cut from: the pipeline then equals one created at the new size, byte for byte)
    if (m_frameIndex.frameIndex > 0) setCameraCut();
    if (W == settings.width && H == settings.height) return; // back from minimized at the same size: the images are kept
    m_be.recreateSwapchain(W, H);
    settings.width = W; settings.height = H;
    const BandSettings& rb = m_requestedSettings.band; // the constructor's clamps (they follow the size)
    settings.band.giHalo = rb.giHalo == 0xfffffffeu ? 0u : std::min(rb.giHalo, std::max(W, H));
    settings.band.giHistoryHalo = std::min(rb.giHistoryHalo, std::max(W, H));
    m_cameraIntrinsic.aspectRatio = (float)W / (float)H;
    m_be.resizeImages({m_frameRenderTargets[0].motionBuffer, m_frameRenderTargets[1].motionBuffer, m_frameRenderTargets[0].colorBuffer, m_frameRenderTargets[0].depthBuffer,
                       m_frameRenderTargets[1].colorBuffer, m_frameRenderTargets[1].depthBuffer, m_postProcessBuffers[0], m_postProcessBuffers[1], m_worldSpaceNormalImage,
                       m_albedoImage, m_specularImage},
                      W, H);
    if (m_shadingNormalCreated) m_be.resizeImages({m_shadingNormalImage}, W, H);
    m_be.resizeImages({m_depthHalfRes}, W / 2, H / 2);
    m_be.recreateImage(m_minMaxDepthPyramid, depthPyramidDescription(settings)); // (its mip layout follows the size: full chain or per tile)
    m_be.updateComputePassShaderDescription(m_depthPyramidPass, depthPyramidShaderDescription());
    m_taa.resizeImages(m_be, W, H);
    // the froxel volumes (Volumetrics.cpp:123-133); also when they are inputs (run_volumetrics off): the constructor sizes the integration volume from the screen
    m_be.resizeImages({m_volumetricIntegrationVolume, m_scatteringTransmittanceVolume, m_volumetricLightingHistory[0], m_volumetricLightingHistory[1], m_volumeMaterialVolume},
                      (uint32_t)std::ceil(W / 8.f), (uint32_t)std::ceil(H / 8.f));
    m_sdfGi.resize(m_be, W, H, settings.sdfTrace);
    m_be.resizeStorageBuffer(m_histogramPerTileBuffer, (size_t)histogramTileCount(W, H) * nHistogramBins * sizeof(uint32_t));
    m_be.updateComputePassShaderDescription(m_histogramPerTilePass, histogramPerTileShaderDescription(W, H));
    m_be.updateComputePassShaderDescription(m_histogramCombinePass, histogramCombineShaderDescription(W, H));
}

// the stale-flag branches of prepareNewFrame (RenderFrontend.cpp:235-264) for what the UI edits (:1882-2011)
void FramePipeline::applySettings(const FramePipelineSettings& n) {
    const FramePipelineSettings old = settings;
    settings.taa = n.taa;
    settings.bloom = n.bloom; // read by every frame's recording
    settings.sdfTrace.halfResTrace = n.sdfTrace.halfResTrace;
    settings.sdfTrace.strictInfluenceRadiusCutoff = n.sdfTrace.strictInfluenceRadiusCutoff;
    settings.sdfTrace.traceInfluenceRadius = n.sdfTrace.traceInfluenceRadius;
    settings.sdfDebug = n.sdfDebug;
    settings.shading = n.shading; // (the cascade count is fixed: updateSettings refused a change)
    if (!sameShading(old.shading, settings.shading)) // m_isMainPassShaderDescriptionStale
        m_be.updateComputePassShaderDescription(m_deferredShadingPass, forwardPassShaderDescription(settings.shading));
    if (old.shading.diffuseBRDF != settings.shading.diffuseBRDF) { // m_isBRDFLutShaderDescriptionStale (:1976): re-baked by the next prepareRenderpasses
        m_be.updateComputePassShaderDescription(m_brdfLutPass, brdfLutShaderDescription(settings.shading));
        m_isBRDFLutShaderDescriptionStale = true;
    }
    if (!sameTaa(old.taa, settings.taa)) m_taa.updateSettings(m_be, settings.taa); // m_taaSettingsChanged: the pass descriptions only
    if (!sameDebug(old.sdfDebug, settings.sdfDebug) || old.sdfTrace.strictInfluenceRadiusCutoff != settings.sdfTrace.strictInfluenceRadiusCutoff)
        m_sdfGi.updateSettings(m_be, settings.sdfTrace, settings.sdfDebug, settings.shading.sunShadowCascadeCount - 1);
    if (old.sdfTrace.halfResTrace != settings.sdfTrace.halfResTrace) { // m_sdfTraceResolutionChanged (:257-262)
        m_sdfGi.resize(m_be, settings.width, settings.height, settings.sdfTrace);
        setCameraCut();
    }
}

void FramePipeline::frame(const CameraExtrinsic& camera, float deltaTime, float time) { // Runtime/main.cpp:79-90
    applyPendingChanges();
    if (m_minimized) return; // (RenderFrontend.cpp:229, 525, 537, 687) nothing recorded, launched or counted
    m_frameIndex.markNewFrame();
    m_taa.rotateWeightBuffer(); // before the passes are recorded: they bind the buffer this frame's weights are written to
    m_lastDeltaTime = deltaTime; // Timer::getDeltaTimeFloat() of this frame (Volumetrics.cpp:124)
    // RenderFrontend::prepareNewFrame, RenderFrontend.cpp:198-278
    m_be.updateShaderCode();
    m_be.newFrame();
    prepareRenderpasses();
    m_be.prepareForDrawcallRecording();
    // App::runUpdate, App.cpp:64-74
    setCameraExtrinsic(camera);
    updateMainPassMatrices(); // (RenderFrontend.cpp:581-585) from the jittered viewProjection / viewProjectionPrevious the global UBO gets
    updateGlobalShaderInfo(deltaTime, time);
    // RenderFrontend::renderFrame, RenderFrontend.cpp:685-705: the GPU-visible frame index lags the CPU one
    m_globalShaderInfo.frameIndex++;
    m_globalShaderInfo.frameIndexMod2 = m_globalShaderInfo.frameIndex % 2;
    m_globalShaderInfo.frameIndexMod3 = m_globalShaderInfo.frameIndex % 3;
    m_globalShaderInfo.frameIndexMod4 = m_globalShaderInfo.frameIndex % 4;
    m_be.renderFrame(true);
    m_globalShaderInfo.cameraCut = 0;
}

} // namespace plrhost
