// Validation and packing of the scene's SDF (FramePipeline::setSceneSdf, setSceneSdfMeanAlbedo, and the determinant test setSceneMeshTransforms runs while a
// scene SDF is set) for "sdfInstanceUpdate.comp": host code without a backend call, beside scene_packing.cpp, so that a stand-alone program can run it under a
// sanitizer (tools/scene_sdf_check.cpp). The determinant is the instance contract's own fp64 expression (device/scene_sdf.h), evaluated by the text the kernel
// evaluates; this file is compiled without floating-point contraction like every other.
#include <cmath>
#include <cstring>
#include <string>

#include "../device/scene_sdf.h"
#include "frame_pipeline.h"

namespace plrhost {

static plr::scenesdf::Box boxOf(const float* six) {
    plr::scenesdf::Box b;
    for (int c = 0; c < 3; c++) { b.mn[c] = six[c]; b.mx[c] = six[3 + c]; }
    return b;
}

double sceneSdfDeterminant(const float* model16, const float* localBox6) { return plr::scenesdf::instanceDeterminant(model16, boxOf(localBox6)); }

void refuseSingularSceneSdfMatrices(const float* matrices16, uint32_t drawCount, const PackedSceneSdf& sdf, const uint32_t* drawMeshes, const char* call) {
    for (uint32_t i = 0; i < (uint32_t)sdf.instanceDraws.size(); i++) {
        const uint32_t d = sdf.instanceDraws[i];
        if (d >= drawCount) continue;
        const double det = sceneSdfDeterminant(matrices16 + (size_t)d * 16u, sdf.meshBoxes.data() + (size_t)drawMeshes[d] * 6u);
        if (det == 0.0 || !std::isfinite(det))
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": singular model matrix: the determinant of draw " + std::to_string(d) + " (SDF instance " + std::to_string(i) +
                                       ") is " + (det == 0.0 ? std::string("zero") : std::string("not finite")) + ", its worldToLocal does not exist");
    }
}

// everything is validated before anything is built; the caller changes its state only with the result in hand
PackedSceneSdf packSceneSdf(const uint32_t* sdfTextures, uint32_t meshCount, const SceneSdfContext& scene) {
    const char* call = "setSceneSdf";
    if (scene.drawCount == 0 || scene.meshCount == 0) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": no scene set (setSceneMeshes comes first)");
    if (meshCount != scene.meshCount)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": mesh count " + std::to_string(meshCount) + " differs from the scene's mesh count " + std::to_string(scene.meshCount));
    if (!sdfTextures) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": meshes are null");
    PackedSceneSdf out;
    out.meshSdf.assign(sdfTextures, sdfTextures + meshCount);
    out.meshBoxes.assign((size_t)meshCount * 6u, 0.f);
    size_t vertex = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        const uint32_t n = scene.meshVertexCounts[m];
        if (sdfTextures[m] != kNoSceneTexture) {
            if (n == 0) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": mesh " + std::to_string(m) + " has an SDF and no vertex: it has no local box");
            float* box = out.meshBoxes.data() + (size_t)m * 6u;
            for (uint32_t v = 0; v < n; v++)
                for (int c = 0; c < 3; c++) {
                    const float p = scene.positions[(vertex + v) * 3u + c];
                    if (!std::isfinite(p))
                        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": non-finite position: vertex " + std::to_string(v) + " of mesh " + std::to_string(m) + ", which has an SDF");
                    box[c] = v == 0 ? p : plr::scenesdf::minOf(box[c], p);
                    box[3 + c] = v == 0 ? p : plr::scenesdf::maxOf(box[3 + c], p);
                }
            if (sdfTextures[m] == kSceneSdfBake) out.bakedMeshes.push_back(m);
        }
        vertex += n;
    }
    for (uint32_t d = 0; d < scene.drawCount; d++)
        if (sdfTextures[scene.drawMeshes[d]] != kNoSceneTexture) out.instanceDraws.push_back(d);
    if (out.instanceDraws.size() > scene.maxInstances)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": too many SDF instances: " + std::to_string(out.instanceDraws.size()) + " draws have a mesh with an SDF, max_sdf_instances is " +
                                   std::to_string(scene.maxInstances));
    refuseSingularSceneSdfMatrices(scene.models, scene.drawCount, out, scene.drawMeshes, call);
    return out;
}

std::vector<uint32_t> sceneSdfInstanceTable(const PackedSceneSdf& sdf, const uint32_t* drawMeshes, const uint32_t* meshTextureIndices) {
    std::vector<uint32_t> table(sdf.instanceDraws.size() * 8u);
    for (size_t i = 0; i < sdf.instanceDraws.size(); i++) {
        const uint32_t d = sdf.instanceDraws[i], m = drawMeshes[d];
        plr::scenesdf::InstanceEntry e{};
        e.draw = d; e.sdfTextureIndex = meshTextureIndices[m];
        std::memcpy(e.localMin, sdf.meshBoxes.data() + (size_t)m * 6u, 12);
        std::memcpy(e.localMax, sdf.meshBoxes.data() + (size_t)m * 6u + 3u, 12);
        std::memcpy(table.data() + i * 8u, &e, sizeof(e));
    }
    return table;
}

std::vector<float> packSceneSdfMeanAlbedo(const float* rgbOrNan, uint32_t drawCount, uint32_t sceneDrawCount, bool sceneSdfSet) {
    const char* call = "setSceneSdfMeanAlbedo";
    if (!sceneSdfSet) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": no scene SDF set (setSceneSdf comes first)");
    if (drawCount != sceneDrawCount)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": draw count " + std::to_string(drawCount) + " differs from the scene's draw count " + std::to_string(sceneDrawCount));
    if (!rgbOrNan) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": values are null");
    for (uint32_t d = 0; d < drawCount; d++) {
        const float* v = rgbOrNan + (size_t)d * 3u;
        if (std::isnan(v[0])) continue; // derive: green and blue are not looked at
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(v[c]))
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": non-finite mean albedo: component " + std::to_string(c) + " of draw " + std::to_string(d) + " (a NaN red alone means derive)");
    }
    return std::vector<float>(rgbOrNan, rgbOrNan + (size_t)drawCount * 3u);
}

} // namespace plrhost
