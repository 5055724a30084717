// Host-side frame graph author for the hot path: the compute part of the reference's RenderFrontend
// (Plain/src/Runtime/Rendering/RenderFrontend.cpp:313-406 prepareRenderpasses and the compute*/init* helpers) and of its
// technique classes (Techniques/TAA.cpp, Bloom.cpp, SDFGI.cpp), written against the RenderBackend shim in
// include/plr_render_backend.hpp. Rasterised passes (depth prepass, shadow cascades, forward shading, sky) are inputs:
// their outputs (G-buffer, shadow maps, LUTs) are uploaded by the caller (the cascades are rasterised by a compute pass instead while mesh casters are set, the G-buffer while scene meshes are set); forward shading is replaced by the deferred
// compute pass. Pass order, bindings, specialisation constants and dispatch counts are the reference's.
#pragma once
#include <array>
#include <string>
#include <functional>
#include <stdexcept>
#include <vector>

#include "../../../include/plr_render_backend.hpp"

namespace plrhost {

struct Vec3 { float x = 0, y = 0, z = 0; };
struct Mat4 { float m[16]; }; // column major: m[col * 4 + row]

// GPU image of GlobalShaderInfo (ResourceDescriptions.h:174-203 / global.inc:4-33); the bool is 4 bytes at offset 320
struct GlobalShaderInfo {
    Mat4 viewProjection{};
    Mat4 viewProjectionPrevious{};
    float sunDirection[4] = {0.f, -1.f, 0.f, 0.f};
    float cameraPos[4] = {0, 0, 0, 0};
    float cameraPosPrevious[4] = {0, 0, 0, 0};
    float cameraRight[4] = {1.f, 0.f, 0.f, 0.f};
    float cameraUp[4] = {0.f, -1.f, 0.f, 0.f};
    float cameraForward[4] = {0.f, 0.f, -1.f, 0.f};
    float cameraForwardPrevious[4] = {0.f, 0.f, -1.f, 0.f};
    int32_t noiseTextureIndices[4] = {0, 0, 0, 0};
    float currentFrameCameraJitter[2] = {0, 0};
    float previousFrameCameraJitter[2] = {0, 0};
    int32_t screenResolution[2] = {0, 0};
    float cameraTanFovHalf = 1.f;
    float cameraAspectRatio = 1.f;
    float nearPlane = 0.1f;
    float farPlane = 100.f;
    float sunIlluminanceLux = 128000.f;
    float exposureOffset = 1.f;
    float exposureAdaptionSpeedEvPerSec = 2.f;
    float deltaTime = 0.016f;
    float time = 0.f;
    float mipBias = 0.f;
    uint32_t cameraCut = 0;
    uint32_t frameIndex = 0;
    uint32_t frameIndexMod2 = 0;
    uint32_t frameIndexMod3 = 0;
    uint32_t frameIndexMod4 = 0;
};
static_assert(sizeof(GlobalShaderInfo) == 340, "GlobalShaderInfo layout");

struct CameraExtrinsic { Vec3 position; Vec3 forward{0, 0, -1}; Vec3 up{0, -1, 0}; Vec3 right{1, 0, 0}; };
struct CameraIntrinsic { float fov = 35.f; float aspectRatio = 1.f; float near = 0.1f; float far = 300.f; }; // Camera.h:11-16

struct FrameRenderTargets { ImageHandle colorBuffer, motionBuffer, depthBuffer; };

// ---- band rendering (no reference counterpart): the frame is partitioned over GPUs by screen rows.
// Every instance allocates the images of the WHOLE frame (HBM is not the constraint: ~80 B/px) and uses full-frame coordinates,
// but records dispatches (ComputePassExecution::dispatchBase) only for the rows it owns plus the halo a later pass reads, and
// calls the exchange callback where a pass reads rows a neighbouring band produced (DESIGN.md "Multi-GPU").
struct RowRange { uint32_t begin = 0, end = 0xffffffffu; }; // pixel rows of a pass's output image; default = all rows
typedef RowRange ColRange;                                   // the same for pixel columns (tile rendering)
struct BandSettings {
    uint32_t rowBegin = 0, rowEnd = 0;  // owned full-resolution rows [rowBegin, rowEnd); rowEnd == 0: band rendering off
    // tile rendering (round 5; BASELINE config 5's 2 x 2 screen tiles): the band is cut in columns too - this instance owns columns [colBegin, colEnd)
    // of its rows (multiples of 64, or the last column). colEnd == 0: whole rows (a band). Every halo below is the same number of COLUMNS on the sides
    // that have a neighbour; the passes are restricted to the tile's columns through ComputePassExecution::dispatchBase[0] (plr.h valid_cols / first_cols)
    uint32_t colBegin = 0, colEnd = 0;
    bool tiled() const { return colEnd > colBegin; }
    uint32_t giHalo = 64;               // trace-resolution rows of the GI images exchanged before each spatial filter pass
    // REQUEST LISTS instead of a halo in front of the two spatial filter passes (round 6; plr_frame.h PLRF_HALO_REQUESTED): a giSampleRequests pass per filter marks
    // the texels outside this rectangle its disc samples land on (they depend on depth, camera and frame index only), the exchange callback ExchangeGiRequests
    // trades the bitmaps, and at ExchangeGiTrace / ExchangeGiTemporal every owner sends exactly the requested texels. The partitioned frame then equals the
    // unpartitioned one bit for bit, as with a whole-image halo, for 6 - 27 MB per rank and frame at 8K instead of 200 (profiles/r06_gi_request_count.txt)
    bool giRequested = false;
    uint32_t giHistoryHalo = 16;        // trace-resolution rows of the filtered GI exchanged for the upscale / next frame's reprojection
    uint32_t colorHalo = 8;             // full-resolution rows shaded beyond the band (3x3 neighbourhood of the temporal filter)
    uint32_t postHalo = 224;            // full-resolution rows of the temporal filter's result exchanged for the bloom chain: the chain's dependency cone
                                        // reaches 222 rows (Bloom::requiredSourceHalo; 6 mips, radius 1.5) - computeBloom refuses a smaller halo
    uint32_t taaHistoryHalo = 32;       // full-resolution rows of the TAA history exchanged (reach of next frame's reprojection + bicubic footprint)
    // Overlap the halo transfers with compute: the pass that produces an exchanged image is recorded as "edge rows first" (the rows the
    // neighbours need), then the exchange is STARTED (callback with ExchangeBegin: enqueue the sends / receives, do not wait), then the
    // interior rows are recorded, and the callback with ExchangeEnd (wait) sits where the first consumer of the halo rows is recorded.
    // Off: one callback per exchange point (start and wait), the producer in one dispatch.
    bool overlapExchange = true;
    // with overlapExchange: the producer of an exchanged image is ONE execution that produces the edge rows first and raises the backend's edge signal
    // (plr.h first_rows) instead of an edge and an interior execution; false = the split recording of round 3
    bool rowsFirst = true;
    bool enabled() const { return rowEnd > rowBegin; }
    // a partitioned pipeline rasterises scene meshes and shadow casters (plr_frame.h band_raster): the depth prepass in this rank's raster window
    // (rasterWindowTiles), every shadow cascade in full on every rank. Off: the scene and caster calls are refused on a partitioned pipeline
    bool raster = false;
    // default giHalo for a frame of `height` rows: 64 trace rows per 2160 rows of frame height (plrf_default_settings)
    static uint32_t giHaloForHeight(uint32_t height) { return 64u * ((height + 2159u) / 2160u); }
};
struct FramePipelineSettings;
// The raster window of a pipeline with settings `s` (as given to the constructor, or its current ones), in 64 x 64 tiles, half-open {x0, y0, x1, y1}: the owned
// rectangle grown, per side with a neighbour, by the largest reach with which a recorder of the pipeline reads the G-buffer images outside the rectangle (derived
// pass by pass at the definition and in DESIGN.md "Rasterising in a partition"), rounded out to tiles and clipped to the frame. No backend call.
void rasterWindowTiles(const FramePipelineSettings& s, uint32_t outTiles[4]);
// the wrap strips of that window (at most 3, four words each as above; returns their number): the tiles at the opposite frame edge that the temporal GI filter's
// repeat-addressed read of last frame's motion reaches from a window that touches a frame edge
uint32_t rasterWrapStrips(const FramePipelineSettings& s, uint32_t outTiles[12]);
// phase bits or-ed into the exchange id a callback receives (0: start the exchange and wait for it)
enum ExchangePhase : int { ExchangeBegin = 0x100, ExchangeEnd = 0x200, ExchangeIdMask = 0xff };
// ExchangeDepthApex (only with runLightMatrix): all-reduce of the band's depth range, min on .r / max on .g of a 1 x 1 RG32F image (depthApexImage())
// ExchangeGiRequests (only with BandSettings::giRequested): the request bitmaps of both spatial filter passes (FramePipeline::giRequestExchange)
enum ExchangeId : int { ExchangeHistogram = 0, ExchangeGiTrace = 1, ExchangeGiTemporal = 2, ExchangeGiHistory = 3, ExchangePost = 4, ExchangeDepthApex = 5, ExchangeGiRequests = 6,
                        ExchangeCount = 7 };
// one image whose rows next to the band must be refreshed from the neighbours: this band sends its first / last haloRows owned
// rows up / down and receives [rowBegin - haloRows, rowBegin) and [rowEnd, rowEnd + haloRows) (clipped to the image)
// tile rendering: the owned rectangle is columns [colBegin, colEnd) of those rows (imageCols texels of texelBytes bytes per row), the halo is haloRows texels wide
// on every side with a neighbour (corners included)
struct ExchangeItem { ImageHandle image; uint32_t mip = 0; uint32_t rowBegin = 0, rowEnd = 0, haloRows = 0, rowBytes = 0, imageRows = 0;
                      uint32_t colBegin = 0, colEnd = 0, imageCols = 0, texelBytes = 0; };
typedef int (*ExchangeCallback)(void* user, int exchangeId, void* hipStream);

// ---- Techniques/TAA.h
enum class HistorySamplingTech : int { Bilinear = 0, Bicubic16Tap = 1, Bicubic9Tap = 2, Bicubic5Tap = 3, Bicubic1Tap = 4 };
struct TAASettings {
    bool enabled = true;
    bool useSeparateSupersampling = false;
    bool useClipping = true;
    bool useMotionVectorDilation = true;
    HistorySamplingTech historySamplingTech = HistorySamplingTech::Bicubic1Tap;
    bool supersampleUseTonemapping = true;
    bool filterUseTonemapping = true;
    bool useMipBias = true;
};
struct BloomSettings { bool enabled = true; float strength = 0.05f; float radius = 1.5f; };
// Techniques/SDFGI.h:9-15
enum class SDFVisualisationMode : int { None = 0, VisualizeSDF = 1, CameraTileUsage = 2, SDFNormals = 3, RaymarchingSteps = 4 };
struct SDFDebugSettings {
    SDFVisualisationMode visualisationMode = SDFVisualisationMode::None;
    bool showCameraTileUsageWithHiZ = true;
    bool useInfluenceRadiusForDebug = false;
};
struct SDFTraceSettings {
    bool halfResTrace = true;
    bool strictInfluenceRadiusCutoff = true;
    float traceInfluenceRadius = 5.f;
    float additionalSunShadowMapPadding = 3.f;
};
enum class DiffuseBRDF : int { Lambert = 0, Disney = 1, CoDWWII = 2, Titanfall2 = 3 };
enum class DirectSpecularMultiscattering : int { McAuley = 0, Simplified = 1, ScaledGGX = 2, None = 3 };
enum class IndirectLightingTech : int { SDFTrace, ConstantAmbient };
struct ShadingConfig {
    DiffuseBRDF diffuseBRDF = DiffuseBRDF::CoDWWII;
    DirectSpecularMultiscattering directMultiscatter = DirectSpecularMultiscattering::McAuley;
    IndirectLightingTech indirectLightingTech = IndirectLightingTech::SDFTrace;
    bool useGeometryAA = true;
    int sunShadowCascadeCount = 3;
};

struct FrameIndexCounter { // Runtime/FrameIndex.cpp
    size_t frameIndex = 0;
    void markNewFrame() { frameIndex++; }
    size_t mod2() const { return frameIndex % 2; }
    size_t mod8() const { return frameIndex % 8; }
};

class TAA {
public:
    void init(RenderBackend& be, int imageWidth, int imageHeight, const TAASettings& settings);
    void computeTemporalFilter(RenderBackend& be, const FrameIndexCounter& fi, ImageHandle colorSrc, const FrameRenderTargets& currentFrame, ImageHandle target,
                               RowRange rows = {}, uint32_t edgeRows = 0, const std::function<void()>& edgesDone = nullptr, bool rowsFirst = false, ColRange cols = {}) const;
    ImageHandle historyDst(const FrameIndexCounter& fi) const { return m_historyBuffers[(fi.mod2() + 1) % 2]; }
    void resizeImages(RenderBackend& be, int imageWidth, int imageHeight);         // TAA::resizeImages (TAA.cpp:69-83)
    void updateSettings(RenderBackend& be, const TAASettings& settings);            // TAA::updateSettings: the pass descriptions only
    // TAASettings::useSeparateSupersampling (TAA.cpp:85-137): luminance of the current frame, then a 2-frame blend with contrast / depth rejection
    void computeTemporalSuperSampling(RenderBackend& be, const FrameIndexCounter& fi, const FrameRenderTargets& currentFrame, const FrameRenderTargets& lastFrame,
                                      ImageHandle target, RowRange rows = {}) const;
    ImageHandle m_sceneLuminance[2];
    void jitterInPixels(const FrameIndexCounter& fi, float out[2]) const;
    void updateTaaResolveWeights(RenderBackend& be, const float cameraJitterInPixels[2]);
    ImageHandle m_historyBuffers[2];
    UniformBufferHandle m_taaResolveWeightBuffer;      // the one this frame's passes bind and this frame's weights go to
    UniformBufferHandle m_taaResolveWeightBuffers[2];   // rotated per frame (rotateWeightBuffer): a resolve that still runs when the next frame is submitted keeps its weights
    uint32_t m_weightBufferIndex = 0;
    void rotateWeightBuffer() { m_weightBufferIndex ^= 1u; m_taaResolveWeightBuffer = m_taaResolveWeightBuffers[m_weightBufferIndex]; }
private:
    RenderPassHandle m_temporalFilterPass, m_temporalSupersamplingPass, m_colorToLuminancePass;
};

class Bloom {
public:
    void init(RenderBackend& be);
    // applyRows: rows bloom is applied to (band rendering; default all). The chain is recorded over the dependency cone of those rows;
    // chainRows: rows of the target image that hold valid colour (the band and the exchanged halo) - must cover the cone's source rows
    // chainCols / applyCols: the same for columns (tile rendering): the chain covers the dependency cone of the tile in both directions
    void computeBloom(RenderBackend& be, ImageHandle targetImage, const BloomSettings& settings, RowRange chainRows = {}, RowRange applyRows = {}, bool asyncTail = false,
                      ColRange chainCols = {}, ColRange applyCols = {}) const;
    struct Cone { RowRange up[6], down[6], source; }; // rows of every level (in the level's own rows) / of the source image the result depends on
    // (the chain is separable in its footprints: the same function of a column range and the image width gives the cone's columns)
    static Cone dependencyCone(RowRange applyRows, uint32_t height, float radius);
    static uint32_t requiredSourceHalo(uint32_t height, float radius); // full-resolution rows of scene colour a band needs beyond its own
private:
    std::vector<RenderPassHandle> m_bloomDownsamplePasses, m_bloomUpsamplePasses;
    RenderPassHandle m_applyBloomPass;
};

// row ranges of one band for the GI passes + where the recorder asks for a halo exchange (band rendering only)
struct GiBand {
    RowRange traceRows;    // trace-resolution rows traced and filtered
    RowRange upscaleRows;  // full-resolution rows of the upscale
    ColRange traceCols, upscaleCols; // tile rendering: the same for columns (default: whole rows)
    void* user = nullptr;
    void (*exchangePoint)(void* user, int exchangeId) = nullptr; // records the exchange (or, with overlap, the wait for it) as a host callback execution
    void (*exchangeBegin)(void* user, int exchangeId) = nullptr; // overlap: records the start of the exchange; null = no overlap
    void (*exchangeWhole)(void* user, int exchangeId) = nullptr; // overlap: an exchange that is not split (start and wait in one callback)
    uint32_t giHalo = 0, giHistoryHalo = 0;                      // trace-resolution halo rows of exchanges 1/2 and 3
    bool rowsFirst = false;                                      // BandSettings::rowsFirst
    bool requested = false;                                      // BandSettings::giRequested: request lists instead of a halo in front of the spatial filters
    // requested + overlap: the response exchange starts behind the producer (requestedBegin), the spatial filter runs the waves that need nothing from it meanwhile
    // (request phase 1), waits (requestedEnd) and runs the rest (phase 2); null: one exchange callback and one filter execution
    void (*requestedBegin)(void* user, int exchangeId) = nullptr;
    void (*requestedEnd)(void* user, int exchangeId) = nullptr;
};
// records exe over `rows` of a w x h image; with edgesDone the first / last `halo` rows are recorded first, then edgesDone(), then the rest
// rowsFirst: ONE execution over all the rows with first_rows = the edges (plr.h), then edgesDone()
// cols: the columns of the rectangle (tile rendering); with rowsFirst its edge columns belong to the edge as well (plr.h first_cols)
void recordRows(RenderBackend& be, ComputePassExecution& exe, uint32_t w, uint32_t h, RowRange rows, uint32_t halo = 0, const std::function<void()>& edgesDone = nullptr, bool rowsFirst = false,
                ColRange cols = {});

struct SDFTraceDependencies {
    FrameRenderTargets currentFrame, previousFrame;
    float frustumPoints[6][4], frustumNormals[6][4];
    ImageHandle depthHalfRes, worldSpaceNormals, skyLut, shadowMap, depthMinMaxPyramid;
    StorageBufferHandle lightBuffer, sunShadowInfoBuffer;
};

class SDFGI {
public:
    void init(RenderBackend& be, int screenW, int screenH, const SDFTraceSettings& traceSettings, const SDFDebugSettings& debugSettings, int sunShadowCascadeIndex,
              uint32_t maxInstances);
    // SDFGI::renderSDFVisualization, Techniques/SDFGI.cpp:334-369
    void renderSDFVisualization(RenderBackend& be, ImageHandle target, const SDFTraceDependencies& deps, const SDFDebugSettings& debugSettings,
                                const SDFTraceSettings& traceSettings) const;
    // packed { uint count; uint pad[3]; SDFInstance[] } and { vec3 min; pad; vec3 max; pad }[] as SDFGI::updateSDFScene builds them
    void updateSDFScene(RenderBackend& be, const void* instanceBufferData, size_t instanceBytes, const void* worldBBData, size_t bbBytes);
    // the instance count of a scene SDF ("sdfInstanceUpdate.comp" writes the buffers): what the culling dispatches are sized by
    void setInstanceCount(uint32_t count) { m_sdfInstanceCount = count; }
    uint32_t instanceCount() const { return m_sdfInstanceCount; }
    void computeIndirectLighting(RenderBackend& be, const FrameIndexCounter& fi, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band = nullptr) const;
    struct IndirectLightingImages { ImageHandle Y_SH, CoCg; };
    IndirectLightingImages getIndirectLightingResults(bool tracedHalfRes) const;
    // SDFGI::resize (SDFGI.cpp:237-258): the trace-resolution images (full or half, traceSettings.halfResTrace) and the full-resolution upscale targets, plus the
    // buffers sized from the screen (culled tiles, request bitmaps)
    void resize(RenderBackend& be, int screenW, int screenH, const SDFTraceSettings& traceSettings);
    // SDFGI::updateSDFDebugSettings / updateSDFTraceSettings: the pass descriptions
    void updateSettings(RenderBackend& be, const SDFTraceSettings& traceSettings, const SDFDebugSettings& debugSettings, int sunShadowCascadeIndex);
    ImageHandle m_indirectDiffuse_Y_SH[2], m_indirectDiffuse_CoCg[2], m_indirectDiffuseHistory_Y_SH[2], m_indirectDiffuseHistory_CoCg[2];
    ImageHandle m_indirectLightingFullRes_Y_SH, m_indirectLightingFullRes_CoCg;
    StorageBufferHandle m_sdfInstanceBuffer, m_sdfCameraFrustumCulledInstances, m_sdfInstanceWorldBBBuffer, m_sdfCameraCulledTiles;
    // request-list exchange (GiBand::requested): per spatial filter pass the bitmap of requested texels, ceil(trace width / 32) words per trace row
    StorageBufferHandle m_giRequestBitmap[2];
    uint32_t m_giRequestRowWords = 0;
private:
    void sampleRequests(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const;
    void sdfInstanceCulling(RenderBackend& be, const SDFTraceDependencies& deps, int targetW, int targetH, float influenceRadius, bool hiZCulling, const GiBand* band) const;
    void diffuseSDFTrace(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const;
    void filterIndirectDiffuse(RenderBackend& be, const SDFTraceDependencies& deps, const SDFTraceSettings& s, const GiBand* band) const;
public:
    UniformBufferHandle m_cameraFrustumBuffer, m_sdfTraceInfluenceRangeBuffer;
private:
    uint32_t m_sdfInstanceCount = 0;
    RenderPassHandle m_diffuseSDFTracePass, m_indirectDiffuseFilterSpatialPass[2], m_indirectDiffuseFilterTemporalPass, m_indirectLightingUpscale,
        m_sdfCameraFrustumCulling, m_sdfCameraTileCulling, m_sdfCameraTileCullingHiZ, m_sdfDebugVisualisationPass, m_giSampleRequestPass[2];
};

// Techniques/Sky.h:6-15 (everything in km); laid out as the std140 block of sky.inc:1-10 (56 bytes)
struct AtmosphereSettings {
    float scatteringRayleighGround[3] = {0.0058f, 0.0135f, 0.0331f};
    float earthRadius = 6371.f;
    float extinctionRayleighGround[3] = {0.0058f, 0.0135f, 0.0331f};
    float atmosphereHeight = 100.f;
    float ozoneExtinction[3] = {0.000650f, 0.001881f, 0.000085f};
    float scatteringMieGround = 0.006f;
    float extinctionMieGround = 1.11f * 0.006f;
    float mieScatteringExponent = 0.76f;
};
static_assert(sizeof(AtmosphereSettings) == 56, "AtmosphereSettings layout");

// Techniques/Volumetrics.h:5-18 and the std140 block of volumetricFroxelLighting.inc:6-16 (state first, then settings: 52 bytes)
struct VolumetricsSettings {
    float scatteringCoefficients[3] = {1.f, 1.f, 1.f};
    float maxDistance = 30.f;
    float absorptionCoefficient = 1.f;
    float baseDensity = 0.003f;
    float densityNoiseRange = 0.008f;
    float densityNoiseScale = 0.5f;
    float phaseFunctionG = 0.2f;
};
struct WindSettings { float vector[3] = {0.f, 0.f, 0.f}; float speed = 0.15f; };
struct VolumetricsState { float windSampleOffset[3] = {0.f, 0.f, 0.f}; float sampleOffset = 0.f; };
struct VolumetricsBufferContents { VolumetricsState state; VolumetricsSettings settings; };
static_assert(sizeof(VolumetricsBufferContents) == 52, "VolumetricLightingSettings layout");

struct FramePipelineSettings {
    uint32_t width = 1920, height = 1080;
    uint32_t shadowMapRes = 2048;  // RenderFrontend.cpp:40
    uint32_t brdfLutRes = 512;     // RenderFrontend.cpp:45
    uint32_t maxSdfInstances = 1200; // SceneConfig.h:3 maxObjectCountMainScene
    uint32_t froxelDepth = 64;
    TAASettings taa;
    BloomSettings bloom;
    SDFTraceSettings sdfTrace;
    SDFDebugSettings sdfDebug; // visualisationMode != None replaces the frame by the debug view (RenderFrontend.cpp:321-340)
    ShadingConfig shading;
    // which groups of prepareRenderpasses are recorded (all on = the full frame)
    bool runExposure = true, runHiZ = true, runGI = true, runShading = true, runTAA = true, runBloom = true, runTonemap = true;
    BandSettings band; // width/height stay the WHOLE frame's
    // input producers recorded as compute passes instead of being uploaded by the caller
    bool runLightMatrix = false; // lightMatrix.comp after the depth pyramid (RenderFrontend.cpp:353, 840-872); in band mode the apex it reads is the all-reduced depth range of the bands (ExchangeDepthApex)
    bool runVolumetrics = false; // froxelVolumeMaterial / froxelLightScattering / volumeLightingReprojection / volumetricLightingIntegration (Volumetrics.cpp:119-243)
    // "skyAndSunSprite.comp" behind the deferred shade: sky dither, froxel in-scattering on the sky and the sun disc (Sky::renderSky, Techniques/Sky.cpp:318-353)
    // on the depth == 0 pixels; needs runShading, not recorded under the SDF debug view (RenderFrontend.cpp:691-694)
    bool runSky = false;
    bool runSkyLuts = false;     // skyTransmissionLut / skyMultiscatterLut / skyLut.comp (Techniques/Sky.cpp:260-316) instead of uploaded LUTs
    float volumetricsMaxDistance = 30.f; // VolumetricsSettings::maxDistance, the last cascade's minimum far plane
};

// a change FramePipeline::setResolution / updateSettings refuses; code = PLR_ERR_UNSUPPORTED or PLR_ERR_INVALID_ARGUMENT (plr.h)
struct FramePipelineRefusal : std::runtime_error {
    int code;
    FramePipelineRefusal(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

// mesh shadow casters (plr_frame.h plrf_set_shadow_casters): the fields of MeshData the shadow pass reads, and one draw of a mesh under a model matrix
struct ShadowCasterMesh { const float* positions = nullptr; uint32_t vertexCount = 0; const uint32_t* indices = nullptr; uint32_t indexCount = 0; };
struct ShadowCasterDraw { uint32_t mesh = 0; float modelMatrix[16] = {}; }; // glm column-major
struct ShadowRasterStats { uint64_t trianglesSubmitted = 0, trianglesDrawn = 0, guardBandRejects = 0; };
// scene meshes (plr_frame.h plrf_set_scene_meshes): a mesh with optional vertex normals (null: face normals), and one draw of a mesh under a model matrix with
// the draw's constant material, two RGBA8 texels as the albedo and specular images store them
struct SceneMesh { const float* positions = nullptr; const float* normals = nullptr; uint32_t vertexCount = 0; const uint32_t* indices = nullptr; uint32_t indexCount = 0; };
struct SceneDraw { uint32_t mesh = 0; float modelMatrix[16] = {}; uint32_t albedo = 0, specular = 0; }; // glm column-major
struct PrepassRasterStats { uint64_t trianglesSubmitted = 0, trianglesClipped = 0, subtrianglesDrawn = 0, rejects = 0; };
// what both mesh sets are validated and packed into, without a backend: the meshes back to back and the draws of either rasteriser. Throws FramePipelineRefusal.
struct PackedMeshes {
    std::vector<float> positions, models;          // 3 floats per vertex, 16 floats per draw
    std::vector<uint32_t> indices;
    std::vector<uint32_t> draws;                   // the pass's record per draw: {firstIndex, indexCount, vertexOffset, transformIndex} and what the pass adds
    uint32_t triangleCount = 0;
    std::vector<uint32_t> meshVertexCounts;        // per mesh, in the order the positions are packed: what the texture and cutout packers lay the UVs out by
    std::vector<float> drawBounds;                 // 6 floats per draw {lo.xyz, hi.xyz}: packDrawBounds ("drawCulling.comp"'s bounds)
};
// setShadowCasters: the buffers of "sunShadowRaster.comp" (device/sun_shadow_raster.h), draws of 4 words (plr::sunraster::Draw)
typedef PackedMeshes PackedCasters;
// setSceneMeshes: the buffers of "depthPrepassRaster.comp" (device/depth_prepass_raster.h), draws of 6 words (plr::prepass::Draw: albedo and specular behind the four)
struct PackedScene : PackedMeshes {
    std::vector<float> normals;                    // 3 floats per vertex, zeros for a mesh without
    std::vector<uint8_t> meshHasNormals;           // per mesh: given with vertex normals (packSceneNormalMaps derives bitangents from them)
    std::vector<uint32_t> drawMeshes;              // per draw: its mesh (packSceneSdf maps draws to SDF instances by it)
    std::vector<uint32_t> meshFirstIndex, meshIndexCounts; // per mesh: where its triangle list lies in `indices` (setSceneSdf bakes from it)
};
// the bounds buffer of "drawCulling.comp" (device/draw_culling.h): per draw the local box of its mesh over ALL the mesh's vertices (indexed or not), exact fp32
// minima and maxima; an axis on which a vertex is a NaN gets NaN bounds (the pass keeps such a draw), a mesh without vertices an all-zero box. Throws
// FramePipelineRefusal for a draw that names no mesh
std::vector<float> packDrawBounds(const float* const* meshPositions, const uint32_t* meshVertexCounts, uint32_t meshCount, const uint32_t* drawMeshes, uint32_t drawCount);
PackedScene packSceneMeshes(const SceneMesh* meshes, uint32_t meshCount, const SceneDraw* draws, uint32_t drawCount);
PackedCasters packShadowCasters(const ShadowCasterMesh* meshes, uint32_t meshCount, const ShadowCasterDraw* draws, uint32_t drawCount);
void refuseNonFiniteMatrices(const float* matrices16, uint32_t drawCount, const char* call);
// refuses (PLR_ERR_INVALID_ARGUMENT, naming `draw`) a caster's model matrix whose last row is not exactly (0, 0, 0, 1)
void refuseUnlessAffine(const float* matrix16, uint32_t draw, const char* call);
// material textures of the scene meshes (plr_frame.h plrf_set_scene_textures): RGBA8 texels, R in the low byte; mipCount levels back to back, or 0: level 0
// only and the host builds the full chain. A material names a texture per output or kNoSceneTexture
constexpr uint32_t kNoSceneTexture = 0xffffffffu;
struct SceneTexture { const uint32_t* texels = nullptr; uint32_t width = 0, height = 0, mipCount = 0; };
struct SceneMaterial { uint32_t albedoTexture = kNoSceneTexture, specularTexture = kNoSceneTexture; };
// what setSceneTextures validates and packs, without a backend: the four extra buffers of a textured "depthPrepassRaster.comp" (device/depth_prepass_raster.h)
struct PackedTextures {
    std::vector<float> uvs;          // 2 floats per vertex of the packed scene, zeros for a mesh given without
    std::vector<uint32_t> materials; // 2 words per draw
    std::vector<uint32_t> textures;  // 4 words per texture: {texelOffset, width, height, mipCount}
    std::vector<uint32_t> texels;
};
// sceneMeshVertexCounts / sceneDrawCount: of the scene the pipeline holds (sceneMeshCount 0: none). Throws FramePipelineRefusal.
PackedTextures packSceneTextures(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                 uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount);
// material textures with a format (plr_frame.h plrf_set_scene_textures_formatted): `data` holds `bytes` bytes - RGBA8 texels as for SceneTexture, or the BC1 / BC3 /
// BC5 blocks of mipCount >= 1 levels back to back, level l being ceil(W_l / 4) x ceil(H_l / 4) blocks, row-major. format: PLR_FORMAT_RGBA8 | BC1 | BC3 | BC5
struct SceneTextureData { const void* data = nullptr; uint64_t bytes = 0; uint32_t width = 0, height = 0, mipCount = 0, format = 0; };
// what setSceneTexturesFormatted validates and packs, without a backend: PackedTextures - `textures` with word offsets, `texels` with the blocks of a compressed
// texture at a multiple of 4 words - and binding 14 of a format-aware "depthPrepassRaster.comp", one format code per texture
struct PackedFormattedTextures : PackedTextures {
    std::vector<uint32_t> formats;
    bool compressed = false; // an entry that is not RGBA8: only then the frame records the sixth push-constant word
};
// Throws FramePipelineRefusal.
PackedFormattedTextures packSceneTexturesFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                                   uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount);
// the block decode contract on the host (plr_image_io.h plr_decode_bc_to_rgba8): one width x height level of `format` (PLR_FORMAT_BC1 | BC3 | BC5), `bytes` bytes of
// blocks, into width * height RGBA8 words, R in the low byte. Throws FramePipelineRefusal: another format, a size of 0 or above 16384, null pointers, a byte count
// other than the level's
void decodeBlockCompressedLevel(uint32_t format, uint32_t width, uint32_t height, const void* blocks, uint64_t bytes, uint32_t* outWords);
// the encode contract on the host (plr_image_io.h plr_encode_rgba8_to_bc; device/texture_build.h holds the arithmetic the kernel shares): one width x height level
// of RGBA8 words into the `bytes` bytes of its `format` blocks. Throws FramePipelineRefusal for what decodeBlockCompressedLevel refuses
void encodeBlockCompressedLevel(uint32_t format, uint32_t width, uint32_t height, const uint32_t* words, void* outBlocks, uint64_t bytes);
// a texture the GPU builds the store entry of (plr_frame.h plrf_build_scene_textures): SceneTextureData and the format the store is to hold
struct SceneTextureSource { const void* data = nullptr; uint64_t bytes = 0; uint32_t width = 0, height = 0, mipCount = 0, format = 0, storeFormat = 0; };
// what buildSceneTextures validates and lays out, without a backend (DESIGN.md "Texture store built on the GPU"): the store of packSceneTexturesFormatted for the
// same textures with all their levels - `texels` holds the levels that are stored as given and zeros where a pass writes -, the RGBA8 staging chains with the given
// levels in place (every level at a multiple of 4 words), and the job tables of the two passes (device/texture_build.h)
struct PackedTextureBuild : PackedFormattedTextures {
    std::vector<uint32_t> staging;
    std::vector<uint32_t> chainJobs;      // ChainJob records, the jobs of one launch back to back, launches in level order
    struct ChainLaunch { uint32_t firstJob, jobCount, groupCount; };
    std::vector<ChainLaunch> chainLaunches;
    std::vector<uint32_t> encodeJobs;     // EncodeJob records
    uint32_t encodeGroups = 0;
    uint64_t chainTexels = 0, blocksEncoded = 0;
};
// Throws FramePipelineRefusal.
PackedTextureBuild packSceneTextureBuild(const SceneTextureSource* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                         uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount);
// what setSceneAlphaCutoffs validates and packs, without a backend: binding 10 of an alpha-tested "depthPrepassRaster.comp", one cutoff code per draw
struct PackedAlphaCutoffs {
    std::vector<uint32_t> cutoffs;
    bool tested = false; // a cutoff other than 0: only then the frame records the fourth push-constant word
};
// sceneDrawCount / sceneTextureCount: of the scene and the textures the pipeline holds. Throws FramePipelineRefusal.
PackedAlphaCutoffs packSceneAlphaCutoffs(const uint32_t* cutoffs, uint32_t drawCount, uint32_t sceneDrawCount, uint32_t sceneTextureCount);
// what setSceneNormalMaps validates, derives and packs, without a backend: bindings 11 - 13 of a normal-mapped "depthPrepassRaster.comp" and its fifth push-constant word
struct PackedNormalMaps {
    std::vector<float> tangents, bitangents; // 3 floats per vertex of the packed scene, zeros for a mesh given without tangents
    std::vector<uint32_t> normalMaterials;   // one texture index, or kNoSceneTexture, per draw
    uint32_t decode = 0;
};
// of the scene and the textures the pipeline holds: per mesh its vertex count and whether it came with normals, the packed normals (3 floats per vertex)
struct SceneNormalMapContext {
    const uint32_t* meshVertexCounts = nullptr; const uint8_t* meshHasNormals = nullptr; const float* normals = nullptr;
    uint32_t meshCount = 0, drawCount = 0, textureCount = 0;
};
// bitangent = normalize(cross(tangent, normal)) in fp64 from the promoted floats, each component (float)(c_r / len); (0, 0, 0) where len is not a finite number > 0
void deriveBitangent(const float tangent[3], const float normal[3], float out[3]);
// Throws FramePipelineRefusal.
PackedNormalMaps packSceneNormalMaps(const float* const* meshTangents, const float* const* meshBitangents, uint32_t meshCount, const uint32_t* normalTextures, uint32_t drawCount,
                                     uint32_t decode, const SceneNormalMapContext& scene);
// alpha-tested cutouts of the shadow casters (plr_frame.h plrf_set_shadow_caster_cutouts): per caster draw the texture whose alpha is tested (kNoSceneTexture:
// alpha 255 everywhere) and the cutoff code 0 .. 255, 0 = opaque
struct ShadowCutout { uint32_t albedoTexture = kNoSceneTexture, alphaCutoff = 0; };
// what setShadowCasterCutouts validates and packs, without a backend: bindings 6 - 9 of a "sunShadowRaster.comp" record with textureCount > 0
struct PackedShadowCutouts {
    std::vector<float> uvs;          // 2 floats per vertex of the packed casters, zeros for a mesh given without
    std::vector<uint32_t> materials; // 2 words per draw: {albedoTexture, cutoff}
    std::vector<uint32_t> textures;  // 4 words per texture: {texelOffset, width, height, mipCount}
    std::vector<uint32_t> texels;
    bool tested = false; // a cutoff other than 0: only then the frames record the third push-constant word
};
// casterMeshVertexCounts / casterDrawCount: of the casters the pipeline holds (casterDrawCount 0: none). Throws FramePipelineRefusal.
PackedShadowCutouts packShadowCasterCutouts(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts,
                                            uint32_t drawCount, const uint32_t* casterMeshVertexCounts, uint32_t casterMeshCount, uint32_t casterDrawCount);
// what setShadowCasterCutoutsFormatted validates and packs, without a backend: PackedShadowCutouts - `textures` with word offsets, `texels` with the blocks of a
// compressed texture at a multiple of 4 words, the store packSceneTexturesFormatted gives the same textures - and binding 14 of a format-aware "sunShadowRaster.comp"
struct PackedFormattedShadowCutouts : PackedShadowCutouts {
    std::vector<uint32_t> formats;
    bool compressed = false; // an entry that is not RGBA8: only then the frames record the fourth push-constant word
};
// Throws FramePipelineRefusal: what packShadowCasterCutouts refuses, an unknown format, mipCount 0 on a compressed entry, a bytes mismatch, more than 2^28 words
PackedFormattedShadowCutouts packShadowCasterCutoutsFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount,
                                                              const ShadowCutout* cutouts, uint32_t drawCount, const uint32_t* casterMeshVertexCounts, uint32_t casterMeshCount,
                                                              uint32_t casterDrawCount);
// the scene's SDF (plr_frame.h plrf_set_scene_sdf): per mesh an index from addSdfVolume*, kSceneSdfBake, or kNoSceneTexture (no SDF: its draws make no instance)
constexpr uint32_t kSceneSdfBake = 0xfffffffeu;
// of the scene the pipeline holds: the packed positions and per mesh its vertex count, per draw its mesh and its current model matrix
struct SceneSdfContext {
    const float* positions = nullptr; const uint32_t* meshVertexCounts = nullptr; const uint32_t* drawMeshes = nullptr; const float* models = nullptr;
    uint32_t meshCount = 0, drawCount = 0, maxInstances = 0;
};
// what setSceneSdf validates and derives, without a backend: the local boxes and the instance map of "sdfInstanceUpdate.comp" (device/scene_sdf.h)
struct PackedSceneSdf {
    std::vector<uint32_t> meshSdf;       // per mesh, as given
    std::vector<float> meshBoxes;        // 6 floats per mesh: the fp32 min and max of its positions (zeros for a mesh without an SDF)
    std::vector<uint32_t> instanceDraws; // instance i is draw instanceDraws[i]: the draws whose mesh has an SDF, in draw order
    std::vector<uint32_t> bakedMeshes;   // the meshes that asked for kSceneSdfBake, ascending
};
// Throws FramePipelineRefusal: no scene, a mesh count other than the scene's, null input, an SDF mesh without vertices or with a non-finite position, more
// instances than maxInstances, an instance whose determinant (below) is zero or not finite
PackedSceneSdf packSceneSdf(const uint32_t* sdfTextures, uint32_t meshCount, const SceneSdfContext& scene);
// the fp64 determinant of model * translate(bbOffset) the instance contract divides by (device/scene_sdf.h instanceDeterminant); localBox6 = min, max
double sceneSdfDeterminant(const float* model16, const float* localBox6);
// refuses (PLR_ERR_INVALID_ARGUMENT, naming the draw) a model matrix of a draw that is an SDF instance whose determinant is zero or not finite
void refuseSingularSceneSdfMatrices(const float* matrices16, uint32_t drawCount, const PackedSceneSdf& sdf, const uint32_t* drawMeshes, const char* call);
// the instance table (8 words per instance: plr::scenesdf::InstanceEntry) once every SDF mesh has its global texture array index
std::vector<uint32_t> sceneSdfInstanceTable(const PackedSceneSdf& sdf, const uint32_t* drawMeshes, const uint32_t* meshTextureIndices);
// 3 floats per draw, a NaN red = derive. Throws FramePipelineRefusal: no scene SDF, a draw count other than the scene's, null values, a non-finite component
// of an entry whose red is a number
std::vector<float> packSceneSdfMeanAlbedo(const float* rgbOrNan, uint32_t drawCount, uint32_t sceneDrawCount, bool sceneSdfSet);
// appends levels 1 .. of the full chain of a width x height level 0 (already the last `width * height` texels of `texels`): level l + 1 texel (x, y) per channel
// is (a + b + c + d + 2) >> 2 of the level-l texels at (min(2x, W - 1) | min(2x + 1, W - 1), min(2y, H - 1) | min(2y + 1, H - 1))
void appendMipChain(std::vector<uint32_t>& texels, uint32_t width, uint32_t height);

class FramePipeline {
public:
    explicit FramePipeline(const FramePipelineSettings& s);
    // RenderFrontend::renderSunShadowCascades (RenderFrontend.cpp:354, 760-774) as "sunShadowRaster.comp" (kernels/sun_shadow_raster.hip): while casters are set every
    // frame records one execution per cascade behind computeSunLightMatrices, writing shadow0 .. shadow<cascade count - 1> from whatever sunShadowInfo holds; without
    // casters the uploaded maps are used. Meshes and matrices are copied; drawCount 0 removes the casters. Refusals (FramePipelineRefusal): a mesh index or a vertex
    // index out of range, an index count that is no multiple of 3 and a matrix whose last row is not (0, 0, 0, 1) are PLR_ERR_INVALID_ARGUMENT, a band / tile
    // pipeline is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setShadowCasters(const ShadowCasterMesh* meshes, uint32_t meshCount, const ShadowCasterDraw* draws, uint32_t drawCount);
    // the draws' model matrices for the next frame (setStorageBufferData: applied in call order at the next frame); drawCount must be the casters' draw count
    void setShadowCasterTransforms(const float* matrices16, uint32_t drawCount);
    // alpha-tested cutouts for the casters now set (DESIGN.md "Alpha-tested cutout casters in the sun shadow raster"): textures as for setSceneTextures (the
    // casters keep their own copy: they are another mesh set than the scene's), meshUvs[k]: 2 floats per vertex of caster mesh k, null: all (0, 0), and per draw
    // the texture whose alpha is tested and a cutoff code 0 .. 255, 0 = opaque, 128 = the reference's alpha < 0.5 -> discard. From the next frame on, while a
    // cutoff is not 0, the cascades are recorded with the third push-constant word and bindings 6 - 9, and a fragment whose alpha code is below its draw's cutoff
    // is no fragment. The pass culls front faces, so a single-sided card that faces the light is culled before it is tested, as in the reference: a cutout that
    // is to cast needs both windings. Everything is copied. textureCount 0 removes the cutouts; every setShadowCasters drops them too; they survive
    // setShadowCasterTransforms, setResolution and updateSettings. Refusals: no casters, a mesh or draw count other than the casters', a texture size of 0 or above
    // 16384, too many mips, null texels, a texture index out of range, a cutoff above 255, more than 2^28 texels, a non-finite UV are PLR_ERR_INVALID_ARGUMENT; a
    // band / tile pipeline is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setShadowCasterCutouts(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts, uint32_t drawCount);
    // setShadowCasterCutouts for textures that carry a format (DESIGN.md "Block-compressed cutout textures in the sun shadow raster"): entries as for
    // setSceneTexturesFormatted. While an entry is BC1, BC3 or BC5 and a cutoff is not 0 the cascades are recorded with the fourth push-constant word and binding
    // 14, and the kernel decodes a BC3 tap's alpha block (BC1 and BC5 have alpha 255 everywhere); a call whose entries are all RGBA8 records exactly the pass
    // setShadowCasterCutouts records. The two calls replace one another's store; lifetime and removal are setShadowCasterCutouts'. Refusals: what that call
    // refuses, an unknown format, mipCount 0 on a compressed entry, a bytes mismatch, more than 2^28 words in total. A refused call changes nothing.
    void setShadowCasterCutoutsFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts,
                                         uint32_t drawCount);
    // counters of the last frame's execution for `cascade`; waits for the GPU. Zero before the first frame with casters.
    ShadowRasterStats shadowRasterStats(uint32_t cascade);
    // the shape of the record the last frame with casters made per cascade: the bytes of its push constants (8: opaque, 12: tested, 16: format-aware) and the storage
    // buffers it bound (6, 10, 11). Zeros before the first frame with casters. Does not wait
    void shadowRasterRecord(uint32_t* pushBytes, uint32_t* storageBuffers) const { *pushBytes = m_casterPushBytes; *storageBuffers = m_casterBufferCount; }
    // RenderFrontend::renderDepthPrepass (RenderFrontend.cpp:351, 792-802) as "depthPrepassRaster.comp" (kernels/depth_prepass_raster.hip): while a scene is set every
    // frame records one execution in front of the depth pyramid (also under the SDF debug view) that writes the current render target's depth and motion and the
    // normal, albedo and specular images from the pipeline's own camera matrices and jitter; without a scene the uploaded G-buffer is used. Everything is
    // copied; drawCount 0 removes the scene. Refusals (FramePipelineRefusal): a mesh index or a vertex index out of range, an index count that is no multiple of
    // 3 and a non-finite matrix element are PLR_ERR_INVALID_ARGUMENT, a band / tile pipeline is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setSceneMeshes(const SceneMesh* meshes, uint32_t meshCount, const SceneDraw* draws, uint32_t drawCount);
    // the draws' model matrices from the next frame on; a draw's previous model matrix is the one the last recorded frame used (on the first frame after
    // setSceneMeshes and after a camera cut: the current one). drawCount must be the scene's draw count
    void setSceneMeshTransforms(const float* matrices16, uint32_t drawCount);
    // material textures for the scene now set (DESIGN.md "Material textures in the depth prepass"): from the next frame on the pass is recorded with the third
    // push-constant word and bindings 6 - 9, and a draw whose material names a texture stores the sampled texel instead of its constant word. meshUvs[k]: 2 floats
    // per vertex of mesh k, null: all (0, 0). Everything is copied. textureCount 0 removes them (whatever the other arguments are); setSceneMeshes drops them
    // too. Refusals: no scene, a mesh or draw count other than the scene's, a texture size of 0 or above 16384, too many mips, null texels, a material index out
    // of range, more than 2^28 texels, a non-finite UV are PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setSceneTextures(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount);
    // setSceneTextures for textures that carry a format (DESIGN.md "Block-compressed textures in the depth prepass"): RGBA8 entries behave as there (mipCount 0
    // included); a BC1, BC3 or BC5 entry gives the blocks of its mipCount >= 1 levels and is sampled through the block decode contract. While an entry is
    // compressed the pass is recorded with the sixth push-constant word and binding 14; a call whose entries are all RGBA8 records what setSceneTextures records.
    // Lifetime, removal and what cutoffs and normal maps set afterwards index are setSceneTextures'. Further refusals (PLR_ERR_INVALID_ARGUMENT): an unknown
    // format, mipCount 0 on a compressed entry, a byte count other than the exact size of the entry's levels, more than 2^28 words in total.
    void setSceneTexturesFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount);
    // setSceneTexturesFormatted with the mip chains and the BC1 / BC3 / BC5 blocks made on the GPU (DESIGN.md "Texture store built on the GPU"): the call uploads
    // the given levels, the next frame records "textureMipChain.comp" (one execution per level, at most 14) and "textureBlockEncode.comp" (one execution) once, in
    // front of everything else, and the staging buffer is released after that frame. The store has the layout setSceneTexturesFormatted gives the same textures
    // with all their levels. Further refusals (PLR_ERR_INVALID_ARGUMENT): a format pair the build has no path for, more than 2^28 staging words.
    void buildSceneTextures(const SceneTextureSource* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials, uint32_t drawCount);
    // the texel store as the kernels see it: its word count, and the words when outWords is not null (capacityWords must suffice). Refused while there is no
    // store, and before a frame has run since the call that set or built it (the upload and the build passes belong to that frame); waits for the GPU
    uint64_t readSceneTextureStore(uint32_t* outWords, uint64_t capacityWords);
    struct TextureBuildStats { uint32_t chainLaunches = 0, encodeLaunches = 0; uint64_t chainTexels = 0, blocksEncoded = 0, stagingBytes = 0; };
    TextureBuildStats textureBuildStats() const { return m_textureBuildStats; } // of the last build a frame has recorded; zeros before there is one
    // alpha-tested cutouts for the scene and textures now set (DESIGN.md "Alpha-tested cutouts in the depth prepass"): one cutoff code 0 .. 255 per draw, 0 =
    // opaque, 128 = the reference's alpha < 0.5 -> discard. From the next frame on, while a cutoff is not 0, the pass is recorded with the fourth push-constant word
    // and binding 10, and a fragment whose sampled albedo alpha code is below its draw's cutoff is no fragment. Copied. drawCount 0 removes them; setSceneMeshes
    // and setSceneTextures drop them too. Refusals: no scene, no textures, a count other than the scene's, null cutoffs, a value above 255 are
    // PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setSceneAlphaCutoffs(const uint32_t* cutoffs, uint32_t drawCount);
    // normal maps for the scene and textures now set (DESIGN.md "Normal maps in the depth prepass"): per draw an index into the scene's textures or kNoSceneTexture,
    // per mesh 3 floats per vertex of tangents (null: all (0, 0, 0)) and of bitangents (null: derived on the host as normalize(cross(tangent, normal)),
    // deriveBitangent), and the decode (1: the reference's, 2: unit). From the next frame on the pass is recorded with the fifth push-constant word, bindings
    // 11 - 13 and storage image 5 - the shadingNormal image, created by the first successful call and re-created by a resize -, and the deferred shade reads
    // shadingNormal where it read normal; the SDF trace and the GI filters keep normal. Everything is copied. drawCount 0 removes them and the shade reads normal
    // again; setSceneMeshes and setSceneTextures drop them too; they survive setSceneMeshTransforms, setSceneAlphaCutoffs, setResolution and updateSettings.
    // Refusals: no scene, no textures, a mesh or draw count other than the scene's, null normalTextures, an index that names no texture, a non-finite tangent or
    // bitangent, a decode other than 1 or 2, null bitangents with tangents for a mesh given without normals are PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline
    // is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setSceneNormalMaps(const float* const* meshTangents, const float* const* meshBitangents, uint32_t meshCount, const uint32_t* normalTextures, uint32_t drawCount,
                            uint32_t decode);
    // anisotropic filtering of every texture sample of the depth prepass (DESIGN.md "Anisotropic filtering in the depth prepass"): 0 or 1 is off - isotropic
    // trilinear filtering, the pass record as it was -, 2 .. 16 is the contract's A (8: the reference's sampler). One scalar of pipeline state: it needs neither a
    // scene nor textures, takes effect with the next recorded frame whose scene has textures (the seventh push-constant word), and survives every other scene call,
    // setResolution and updateSettings. Refusals: a value above 16 is PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline is PLR_ERR_UNSUPPORTED. A refused call
    // changes nothing.
    void setSceneAnisotropy(uint32_t maxAnisotropy);
    // counters of the last frame's execution for the scene now set; waits for the GPU. Zero while no scene is set and before the first frame of a newly set scene.
    PrepassRasterStats prepassRasterStats();
    // frustum culling of whole draws on the GPU ("drawCulling.comp", kernels/draw_culling.hip; DESIGN.md "Frustum culling of draws"): kCullScene culls the depth
    // prepass's draws against the frame's own jittered viewProjection (one execution in front of the prepass, wherever the prepass is recorded), kCullShadowCasters
    // the casters per cascade against that frame's light matrices (one execution for all cascades behind computeSunLightMatrices, in front of the first cascade).
    // The rasterisers then bind the culled copy of their draw array - wrap strips of a band / tile pipeline the same copy -, and their images are byte for byte
    // what they are without culling; their counters count the kept draws only. The flags take effect with the next frame and hold until changed, across
    // setSceneMeshes, setShadowCasters, setResolution and updateSettings; a flag whose mesh set is absent does nothing until one is set. A pipeline that never
    // sets a flag records, creates and allocates nothing for it. Refusals: unknown bits are PLR_ERR_INVALID_ARGUMENT, a band / tile pipeline without band.raster
    // is PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    static constexpr uint32_t kCullScene = 1u, kCullShadowCasters = 2u;
    void setDrawCulling(uint32_t flags);
    // counters of the last frame's cull execution; view 0: the main pass, 1 + c: cascade c. Waits for the GPU. All zero for a view that is off, absent or not yet
    // rendered; a view at or past 1 + the cascade count is refused (PLR_ERR_INVALID_ARGUMENT)
    struct DrawCullingStats { uint32_t draws = 0, visibleDraws = 0; uint64_t triangles = 0, visibleTriangles = 0; uint32_t culledByPlane[5] = {0, 0, 0, 0, 0}; };
    DrawCullingStats drawCullingStats(uint32_t view);
    // RenderFrontend::renderDebugGeometry (RenderFrontend.cpp:375-378, 947-956) as "debugGeometry.comp" (kernels/debug_geometry.hip; DESIGN.md "Debug geometry as a
    // compute pass"): while flags are set, every frame records one execution right behind the deferred shade - in front of the sky pass and everything else that
    // reads the colour buffer - that draws one-pixel lines into the frame's colour and depth images, depth-tested (GreaterEqual) and with depth write on:
    // kDebugDrawBoxes the twelve edges of the axis-aligned world box of every scene draw, red (the reference's "Render bounding boxes"; with kCullScene set only
    // the draws the cull kept), kDebugSdfBoxes those of the padded world box of every instance the scene SDF wrote this frame, green, kDebugLines the caller's
    // segments. A flagged source that is absent contributes nothing. Not recorded with the SDF debug view on, nor on a minimized frame. Flags and lines are
    // copied, take effect with the next frame and hold across setSceneMeshes, setSceneMeshTransforms, the texture calls, setResolution and updateSettings. A
    // pipeline that never sets a flag records, creates and allocates nothing for it. Refusals: unknown bits, null lines with a count, more than 2^20 lines, a
    // non-finite coordinate or colour component or a negative colour are PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline (the pass writes depth and has no
    // halo plan) and a pipeline without runShading are PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    static constexpr uint32_t kDebugDrawBoxes = 1u, kDebugSdfBoxes = 2u, kDebugLines = 4u;
    struct DebugLine { float a[3], b[3], rgb[3]; }; // world space; linear colour, stored as is
    void setDebugGeometry(uint32_t flags);
    void setDebugLines(const DebugLine* lines, uint32_t count); // count 0 removes them
    // counters of the last frame that recorded the pass; waits for the GPU. All zero before there is one
    struct DebugGeometryStats { uint32_t submitted = 0, clipped = 0, rejected = 0, drawn = 0, fragments = 0, pixelsWritten = 0; };
    DebugGeometryStats debugGeometryStats();
    // SDFGI::updateSDFScene (Techniques/SDFGI.cpp:260-313) as "sdfInstanceUpdate.comp" (kernels/scene_sdf.hip; DESIGN.md "SDF instances from the scene"): while a
    // scene SDF is set every frame that records the GI trace or the SDF debug view records one execution in front of the camera frustum culling that writes
    // sdfInstances and sdfWorldBBs from mainPassMatrices, and - in a frame after the texture store or the materials changed - "sceneMeanAlbedo.comp" in front of it.
    // sdfTextures[m]: an index from addSdfVolume*, kSceneSdfBake (baked now with the asset pipeline's bake at plr_sdf_texture_description's resolution and
    // registered in the global texture array), or kNoSceneTexture. meshCount 0 removes it; setSceneMeshes removes it too; volumes baked for it are released then,
    // and a repeated call re-uses their images. While it is set setSdfScene is refused (PLR_ERR_UNSUPPORTED) and setSceneMeshTransforms refuses a singular
    // matrix; after a removal the instance count is 0. Refusals: packSceneSdf's are PLR_ERR_INVALID_ARGUMENT; a band / tile pipeline without band.raster is
    // PLR_ERR_UNSUPPORTED. A refused call changes nothing.
    void setSceneSdf(const uint32_t* sdfTextures, uint32_t meshCount);
    // per draw the mean albedo of its instance instead of the derived one (3 floats, a NaN red = derive); drawCount 0 removes the overrides, and so does setSceneSdf
    void setSceneSdfMeanAlbedo(const float* rgbOrNan, uint32_t drawCount);
    struct SceneSdfStats { uint32_t instances = 0, volumesBaked = 0; uint64_t volumeBytes = 0; };
    SceneSdfStats sceneSdfStats() const;
    // the frame's noise inputs as compute passes (kernels/noise.hip; DESIGN.md "Noise textures as compute passes"): generateBlueNoiseTexture for noise0 .. noise3
    // (RenderFrontend.cpp:1251-1269) as four executions of "blueNoiseVoidAndCluster.comp" - texture t takes streams 2 t and 2 t + 1 of the seed -, and
    // generate3DPerlinNoise for perlinNoise3D (Volumetrics.cpp:71-90, 8 cells) as one of "perlinNoise3D.comp". The next frame() records them once, in front of
    // everything else; after that the images stay as written until the caller uploads to them or calls again. A later call before that frame replaces the seed
    // of the kinds it names. The result is a pure function of the seed, so the ranks of a band / tile partition agree without an exchange. A pipeline that never
    // calls this records, creates and allocates nothing for it. Refusals (PLR_ERR_INVALID_ARGUMENT): flags 0 or unknown bits; kNoisePerlin on a pipeline
    // without a perlinNoise3D image. A refused call changes nothing.
    static constexpr uint32_t kNoiseBlue = 1u, kNoisePerlin = 2u;
    void generateNoise(uint32_t seed, uint32_t flags);
    // {swaps, converged, ones, 0} per texture and channel of the last blue-noise generation a frame has run; waits for the GPU. Zero before there is one.
    struct NoiseStats { uint32_t status[4][2][4] = {}; };
    NoiseStats noiseStats();
    void rasterWindow(uint32_t outTiles[4]) const { rasterWindowTiles(settings, outTiles); }
    // RenderFrontend::setResolution (RenderFrontend.cpp:408-421): recorded, applied at the start of the next frame() (prepareNewFrame, :199-222). Every image and
    // buffer whose size follows the screen is re-created zero-filled, as the constructor creates it, and the next frame is a camera cut; a resize to the size the
    // images already have (back from minimized) keeps them and only cuts. Width or height 0: minimized, frame() renders nothing and advances nothing.
    // Partitioned pipelines (band / tile) refuse (FramePipelineRefusal, PLR_ERR_UNSUPPORTED): the exchange plan depends on the frame size.
    void setResolution(uint32_t width, uint32_t height);
    // the settings the reference's UI edits at run time (RenderFrontend.cpp:1882-2011; plr_frame.h plrf_update_settings lists them), recorded and applied at the
    // start of the next frame() with the stale-flag branches of prepareNewFrame (:235-264). Any other field that differs from the pipeline's is refused
    // (PLR_ERR_UNSUPPORTED), width / height that differ from the current resolution too (PLR_ERR_INVALID_ARGUMENT: resizing is setResolution's).
    void updateSettings(const FramePipelineSettings& s);
    // applies what setResolution / updateSettings recorded now instead of at the next frame(): a caller that uploads the frame's inputs (G-buffer, froxel
    // volume) does so into images of the new size
    void applyPendingChanges();
    bool minimized() const { return m_minimized; }
    // one iteration of the reference main loop (Runtime/main.cpp:79-90): markNewFrame, prepareNewFrame, update, renderFrame
    void frame(const CameraExtrinsic& camera, float deltaTime, float time);
    // only re-record + submit with the current state (used by benchmarks that replay one frame)
    ImageHandle image(const std::string& name) const;
    bool storageBuffer(const std::string& name, StorageBufferHandle* out) const;
    bool uniformBuffer(const std::string& name, UniformBufferHandle* out) const;
    uint32_t addSdfVolume(uint32_t res, const void* halfData, size_t bytes);
    // loads a baked SDF volume from a DDS file (what registerMeshes / loadImagesFromPaths do with MeshBinary::texturePaths.sdfTexturePath,
    // RenderFrontend.cpp:456-521) and returns its global texture array index; outDesc (optional) receives the file's description
    uint32_t addSdfVolumeFromDds(const std::string& path, ImageDescription* outDesc = nullptr);
    void setSdfScene(const void* instanceBufferData, size_t instanceBytes, const void* worldBBData, size_t bbBytes);
    void setSunDirection(const float dir[3]);
    void setCameraIntrinsic(float fovDegrees, float nearPlane, float farPlane);
    void setCameraCut() { m_globalShaderInfo.cameraCut = 1; }
    const GlobalShaderInfo& lastSubmittedGlobals() const { return m_submittedGlobals; }
    const float* lastResolveWeights() const { return m_lastWeights; }
    size_t cpuFrameIndex() const { return m_frameIndex.frameIndex; }
    // band rendering: called (from inside renderFrame, in pass order) where rows of neighbouring bands are needed
    void setExchangeCallback(ExchangeCallback fn, void* user) { m_exchangeFn = fn; m_exchangeUser = user; }
    const std::vector<ExchangeItem>& exchangeItems(int exchangeId) const { return m_exchangeItems[exchangeId]; }
    StorageBufferHandle histogramBuffer() const { return m_histogramBuffer; }
    const SDFGI& sdfGi() const { return m_sdfGi; }
    ImageHandle depthHalfRes() const { return m_depthHalfRes; }
    ImageHandle depthApexImage() const { return m_bandDepthApex; }
    RenderBackend& backend() { return m_be; }
    FramePipelineSettings settings;

private:
    void prepareRenderpasses();
    void applyResolution(uint32_t width, uint32_t height);
    void applySettings(const FramePipelineSettings& s);
    ShaderDescription depthPyramidShaderDescription();
    void computeColorBufferHistogram(ImageHandle lastFrameColor);
    void computeExposure();
    void computeDepthPyramid(ImageHandle depthBuffer);
    void downscaleDepth(const FrameRenderTargets& currentTarget);
    void computeDeferredShading(ImageHandle colorTarget, const FrameRenderTargets& current);
    void computeSkyAndSunSprite(ImageHandle colorTarget, const FrameRenderTargets& current);
    void computeTonemapping(ImageHandle src);
    bool asyncPostTail() const { return true; } // bloom chain + tonemap as the frame's asynchronous tail (plr.h async_tail)
    void computeBRDFLut();
    void computeDepthApexOfTiles();
    void computeSunLightMatrices();
    void renderSunShadowCascades();
    void renderDepthPrepass(const FrameRenderTargets& current);
    void updateMainPassMatrices();
    // a storage buffer of either mesh set (or of the cull, debug and SDF passes on top of them) that grows with what is set: a buffer and the capacity that
    // describes it are one object. bytes 0: never created
    struct GrowableBuffer { StorageBufferHandle handle; size_t bytes = 0; };
    void fillBuffer(GrowableBuffer& buffer, const void* data, size_t bytes);
    template <class T> void fillBuffer(GrowableBuffer& buffer, const std::vector<T>& data) { fillBuffer(buffer, data.data(), data.size() * sizeof(T)); }
    void updateTransmissionLut();
    void computeVolumetricLighting(float deltaTime);
    void updateSkyLut();
    void setCameraExtrinsic(const CameraExtrinsic& extrinsic);
    void updateGlobalShaderInfo(float deltaTime, float time);
    RowRange bandRows(uint32_t halo, uint32_t divisor = 1) const;
    ColRange bandCols(uint32_t halo, uint32_t divisor = 1) const; // the tile's columns + halo at 1 / divisor resolution; whole rows when the band is not tiled
    void exchangePoint(int exchangeId, const char* label);
    void addExchangeItem(int exchangeId, ImageHandle image, uint32_t divisor, uint32_t haloRows);
    static int exchangeTrampoline(void* user, void* stream);

    RenderBackend m_be;
    FramePipelineSettings m_requestedSettings; // as given to the constructor (before its clamps): what updateSettings holds the fixed fields to
    uint32_t m_targetWidth = 0, m_targetHeight = 0; // the last resolution asked for (setResolution)
    bool m_resolutionChanged = false, m_minimized = false, m_settingsChanged = false;
    FramePipelineSettings m_pendingSettings;
    FrameIndexCounter m_frameIndex;
    GlobalShaderInfo m_globalShaderInfo, m_submittedGlobals;
    float m_lastWeights[9] = {};
    CameraExtrinsic m_cameraExtrinsic;
    CameraIntrinsic m_cameraIntrinsic;
    SDFTraceDependencies m_frustumScratch{}; // zero until the first setCameraExtrinsic: the reference frontend is a zero-initialised global (RenderFrontend.h)
    int m_sceneRenderTargetIndex = 0;
    bool m_isBRDFLutShaderDescriptionStale = true;
    uint32_t m_depthPyramidThreadgroupCount = 0;

    UniformBufferHandle m_globalUniformBuffer, m_volumetricsInfoBuffer;
    FrameRenderTargets m_frameRenderTargets[2];
    ImageHandle m_postProcessBuffers[2], m_worldSpaceNormalImage, m_albedoImage, m_specularImage, m_minMaxDepthPyramid, m_bandDepthApex, m_depthHalfRes, m_brdfLut, m_skyLut,
        m_transmissionLut, m_volumetricIntegrationVolume;
    ImageHandle m_shadowMaps[4], m_noiseTextures[4];
    std::vector<ImageHandle> m_sdfVolumes;
    StorageBufferHandle m_histogramPerTileBuffer, m_histogramBuffer, m_lightBuffer, m_sunShadowInfoBuffer, m_depthPyramidSyncBuffer;
    RenderPassHandle m_histogramPerTilePass, m_histogramResetPass, m_histogramCombinePass, m_preExposeLightsPass, m_depthPyramidPass, m_depthDownscalePass,
        m_deferredShadingPass, m_tonemappingPass, m_brdfLutPass, m_lightMatrixPass, m_depthApexPass, m_skyTransmissionLutPass, m_skyMultiscatterLutPass, m_skyLutPass,
        m_skyAndSunSpritePass;
    ImageHandle m_skyMultiscatterLut, m_scatteringTransmittanceVolume, m_volumetricLightingHistory[2], m_volumeMaterialVolume, m_perlinNoise3D;
    RenderPassHandle m_froxelVolumeMaterialPass, m_froxelScatteringTransmittancePass, m_volumetricLightingIntegration, m_volumetricLightingReprojection;
    VolumetricsState m_volumetricsState;
    float m_lastDeltaTime = 0.f;
    UniformBufferHandle m_atmosphereSettingsBuffer;
    // mesh shadow casters: created by the first setShadowCasters (a pipeline without casters allocates and records nothing for them)
    uint32_t m_casterDrawCount = 0, m_casterTriangleCount = 0;
    bool m_casterPassesCreated = false;
    RenderPassHandle m_sunShadowRasterPass[4];
    GrowableBuffer m_casterTransforms, m_casterPositions, m_casterIndices, m_casterDraws, m_casterScratch[4];
    // cutouts: created by the first setShadowCasterCutouts; 0 textures, or no cutoff other than 0 = the 8-byte pass record
    uint32_t m_casterTextureCount = 0;
    bool m_casterAlphaTested = false;
    bool m_casterCompressed = false; // setShadowCasterCutoutsFormatted with an entry that is not RGBA8: the 16-byte pass record and binding 14
    uint32_t m_casterPushBytes = 0, m_casterBufferCount = 0; // of the cascades' record as the last frame made it (shadowRasterRecord)
    std::vector<uint32_t> m_casterMeshVertexCounts;
    GrowableBuffer m_casterUvs, m_casterMaterials, m_casterTextures, m_casterTexels, m_casterTextureFormats;
    void dropCasterCutouts() { m_casterTextureCount = 0; m_casterAlphaTested = m_casterCompressed = false; } // every setShadowCasters: they belonged to the casters that are gone
    // scene meshes: created by the first setSceneMeshes (a pipeline without a scene allocates and records nothing for them)
    uint32_t m_sceneDrawCount = 0, m_sceneTriangleCount = 0;
    bool m_scenePassCreated = false, m_scenePreviousValid = false, m_sceneRecorded = false; // recorded: a frame has run the pass for the scene now set
    RenderPassHandle m_depthPrepassRasterPass;
    GrowableBuffer m_sceneMatrices, m_scenePositions, m_sceneNormals, m_sceneIndices, m_sceneDraws, m_sceneScratch;
    // material textures: created by the first setSceneTextures; 0 textures = the untextured pass record
    uint32_t m_sceneTextureCount = 0;
    std::vector<uint32_t> m_sceneMeshVertexCounts;
    GrowableBuffer m_sceneUvs, m_sceneMaterials, m_sceneTextures, m_sceneTexels;
    bool m_sceneTexturesCompressed = false; // setSceneTexturesFormatted with a BC1 / BC3 / BC5 entry: the sixth push-constant word and binding 14
    GrowableBuffer m_sceneTextureFormats;
    // alpha cutoffs: created by the first setSceneAlphaCutoffs; not tested = the pass record without the fourth push-constant word
    bool m_sceneAlphaTested = false;
    GrowableBuffer m_sceneAlphaCutoffs;
    // normal maps: buffers and the shadingNormal image created by the first setSceneNormalMaps; decode 0 = the pass record without the fifth push-constant word
    uint32_t m_sceneNormalDecode = 0;
    uint32_t m_sceneMaxAnisotropy = 0; // setSceneAnisotropy: >= 2 with textures set = the pass record with the seventh push-constant word; no scene call resets it
    std::vector<uint8_t> m_sceneMeshHasNormals;
    std::vector<float> m_sceneNormalsHost; // the packed normals: what absent bitangents are derived from
    GrowableBuffer m_sceneTangents, m_sceneBitangents, m_sceneNormalMaterials;
    ImageHandle m_shadingNormalImage;
    bool m_shadingNormalCreated = false;
    bool normalMapped() const { return m_sceneNormalDecode != 0 && m_sceneTextureCount != 0 && m_sceneDrawCount != 0; }
    // what a call drops of what was set on top of it, each rule once: the removal and the replacement branch of a setter call the same one. m_sceneMaxAnisotropy,
    // the cull flags and the debug flags survive every one of them
    void dropSceneNormalMaps() { m_sceneNormalDecode = 0; }    // they named textures
    void dropSceneAlphaCutoffs() { m_sceneAlphaTested = false; } // they belonged to the materials
    void dropSceneTextures() { m_sceneTextureCount = 0; m_sceneTexturesCompressed = false; m_textureBuildPending = false; dropSceneAlphaCutoffs(); dropSceneNormalMaps(); } // they belonged to the scene
    // the tail of both texture calls: fills the store, takes the counts over and drops what the previous store carried. formats: of a store with a compressed entry
    void takeSceneTextures(const PackedTextures& packed, uint32_t textureCount, const std::vector<uint32_t>* formats);
    std::vector<float> m_sceneModel, m_scenePreviousModel; // 16 floats per draw: what the next frame uses, what the last recorded frame used
    // the scene's SDF: passes and buffers created by the first setSceneSdf. The host keeps the scene's positions, indices and draw -> mesh map for it (the
    // local boxes and the bake need them when setSceneSdf comes)
    std::vector<float> m_scenePositionsHost;
    std::vector<uint32_t> m_sceneIndicesHost, m_sceneDrawMeshes, m_sceneMeshFirstIndex, m_sceneMeshIndexCounts;
    bool m_sceneSdfSet = false, m_sceneSdfPassesCreated = false, m_sceneSdfMeansStale = false;
    PackedSceneSdf m_sceneSdf;
    RenderPassHandle m_sdfInstanceUpdatePass, m_sceneMeanAlbedoPass;
    GrowableBuffer m_sceneSdfTable, m_sceneSdfOverrides, m_sceneSdfMeans, m_sceneSdfMeanScratch;
    uint32_t m_sceneSdfMeanGroups = 1; // dispatch_count[0] of "sceneMeanAlbedo.comp": from the largest level 0 of the store
    struct BakedVolume { ImageHandle image; bool inUse = false; uint64_t bytes = 0; };
    std::vector<BakedVolume> m_sceneSdfVolumes; // images of baked volumes: released (re-created at 1 x 1 x 1) with the scene's SDF, re-used by the next bake
    // draw culling: the pass and the GPU buffers are created by the first setDrawCulling with a flag (and by a mesh call while a flag is set); the host keeps the
    // per-draw local boxes of both mesh sets from the moment the meshes are set - they live and die with the meshes
    uint32_t m_cullFlags = 0;
    bool m_cullPassesCreated = false, m_sceneCullRecorded = false, m_casterCullRecorded = false; // recorded: a frame has run the cull for the mesh set and flags now set
    RenderPassHandle m_drawCullingPass[2]; // main view, shadow views
    std::vector<float> m_sceneBoundsHost, m_casterBoundsHost;
    bool m_sceneBoundsUploaded = false, m_casterBoundsUploaded = false;
    GrowableBuffer m_sceneBounds, m_sceneCulledDraws, m_sceneCullStats, m_casterBounds, m_casterCulledDraws[4], m_casterCullStats;
    bool cullScene() const { return (m_cullFlags & kCullScene) != 0 && m_sceneDrawCount != 0; }
    bool cullCasters() const { return (m_cullFlags & kCullShadowCasters) != 0 && m_casterDrawCount != 0; }
    void prepareDrawCulling();
    void recordDrawCulling(bool shadowViews);
    bool m_sceneBoundsOnGpu = false; // m_sceneBounds holds m_sceneBoundsHost: draw culling and the debug boxes both read it
    void uploadSceneBounds();
    // debug geometry: the pass and its buffers are created by the first setDebugGeometry with a flag; the host keeps the caller's lines
    uint32_t m_debugFlags = 0;
    bool m_debugPassCreated = false, m_debugRecorded = false, m_debugLinesUploaded = false; // recorded: a frame has run the pass since the flags were last 0
    RenderPassHandle m_debugGeometryPass;
    std::vector<float> m_debugLinesHost; // 9 floats per line
    GrowableBuffer m_debugLines, m_debugStats;
    void refuseDebugGeometryUnsupported(const char* call) const;
    void prepareDebugGeometry();
    void recordDebugGeometry(const FrameRenderTargets& current, bool sdfBoxesWritten);
    // noise generation: passes and buffers created by the first generateNoise
    bool m_noisePassesCreated = false;
    uint32_t m_noisePending = 0, m_noiseBlueSeed = 0; // kinds the next frame records; the Perlin seed lives in the queued fill of the gradients
    RenderPassHandle m_blueNoisePass, m_perlinNoisePass;
    StorageBufferHandle m_noiseGaussianTable, m_noisePerlinGradients, m_noiseStatus[4];
    void recordNoiseGeneration();
    // the texture build: passes created by the first buildSceneTextures; the job tables and the staging chains belong to the build that is pending
    bool m_textureBuildPassesCreated = false, m_textureBuildPending = false, m_textureStagingHeld = false, m_textureStagingQueued = false;
    bool m_sceneStoreInFrame = false; // a frame has run since the store was set or built: readSceneTextureStore reads what the kernels see
    uint64_t m_sceneTexelWords = 0;
    RenderPassHandle m_textureMipChainPass, m_textureBlockEncodePass;
    GrowableBuffer m_textureChainJobs, m_textureEncodeJobs, m_textureStaging;
    std::vector<PackedTextureBuild::ChainLaunch> m_textureChainLaunches;
    uint32_t m_textureEncodeJobCount = 0, m_textureEncodeGroups = 0;
    TextureBuildStats m_textureBuildStats, m_textureBuildPendingStats;
    void recordTextureBuild();
    void releaseTextureStaging();
    void removeSceneSdf();
    void updateSceneSdfInstances();
    void noteSceneTexturesChanged(uint32_t maxLevel0Texels);
public:
    AtmosphereSettings atmosphereSettings;
    VolumetricsSettings volumetricsSettings;
    WindSettings windSettings;
private:
    TAA m_taa;
    Bloom m_bloom;
    SDFGI m_sdfGi;

    ExchangeCallback m_exchangeFn = nullptr;
    void* m_exchangeUser = nullptr;
    struct ExchangeCtx { FramePipeline* self; int id; } m_exchangeCtx[3 * ExchangeCount]; // [phase * ExchangeCount + id], phase 0 / begin / end
    std::vector<ExchangeItem> m_exchangeItems[ExchangeCount];
};

} // namespace plrhost
