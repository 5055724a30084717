// "blueNoiseVoidAndCluster.comp" and "perlinNoise3D.comp": what the launchers and the host tables (kernels/noise.hip) and the frame pipeline
// (frontend/frame_pipeline.cpp) share - the pass records' bindings, push constants and limits, and the integer part of THE NOISE CONTRACT (DESIGN.md "Noise
// textures as compute passes") as functions that compile for the host and the device alike.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLR_NOISE_HD __host__ __device__ inline
#else
#define PLR_NOISE_HD inline
#endif

namespace plr {
namespace noise {

// ---- "blueNoiseVoidAndCluster.comp": dispatch {channels, 1, 1}, one block of kBlueThreads lanes per channel
constexpr int kBlueImageBinding = 0;  // storage image, R8 (1 channel) or RG8 (2), W x H with 4 <= W, H <= 64
constexpr int kBlueTableBinding = 1;  // G: W H floats (plr_noise_gaussian_table), read-only
constexpr int kBlueStatusBinding = 2; // out: {swaps, converged, ones, 0} per channel
struct BluePushConstants { uint32_t seed, firstStream; };
constexpr uint32_t kBlueMinSize = 4, kBlueMaxSize = 64;
constexpr uint32_t kBlueThreads = 1024, kBluePixelsPerThread = 4; // lane i owns pixels i, i + 1024, ...: 64 x 64 = 4 per lane
constexpr uint32_t kBlueStatusWords = 4;
constexpr uint32_t kBlueStreams = 8;  // stream 2 texture + channel of the frame's four RG8 textures

// ---- "perlinNoise3D.comp": dispatch {ceil(R^3 / 256), 1, 1}, a lane per voxel
constexpr int kPerlinImageBinding = 0;    // storage image, R8, R x R x R with R <= 256
constexpr int kPerlinGradientBinding = 1; // gridCellCount^3 x 4 floats (plr_noise_perlin_gradients), read-only
struct PerlinPushConstants { uint32_t gridCellCount; };
constexpr uint32_t kPerlinThreads = 256, kPerlinMaxResolution = 256, kPerlinMaxCells = 32;
constexpr uint32_t kPerlinStream = 8;
constexpr uint32_t kPerlinFrameCells = 8; // Volumetrics.cpp:71-90: the 32^3 volume of the froxel material pass has 8 cells

// ---- THE NOISE CONTRACT, integers
PLR_NOISE_HD uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
PLR_NOISE_HD uint32_t streamKey(uint32_t seed, uint32_t stream) { return lowbias32(seed ^ (0x9E3779B9u * (stream + 1u))); }
PLR_NOISE_HD uint32_t whiteNoise(uint32_t key, uint32_t i) { return lowbias32(key + i) & 255u; }
// fp32: one multiply, truncated
PLR_NOISE_HD uint32_t minorityCount(uint32_t pixelCount) { return (uint32_t)((float)pixelCount * 0.1f); }
// fp32: float(rank) + 0.5f, / float(N), * 255.f, truncated
PLR_NOISE_HD uint32_t rankCode(uint32_t rank, uint32_t pixelCount) { return (uint32_t)(((float)rank + 0.5f) / (float)pixelCount * 255.f); }
// the fp32 angle of a hash: 24 bits, exact up to the last multiply
PLR_NOISE_HD float perlinAngle(uint32_t hash) { return ((float)(hash >> 8) * 5.9604644775390625e-08f) * (2.f * 3.1415f); }

} // namespace noise
} // namespace plr
