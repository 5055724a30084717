// Validation and packing of scene meshes for "depthPrepassRaster.comp" (FramePipeline::setSceneMeshes): host code without a backend call, so that a stand-alone
// program can run it under a sanitizer (tools/scene_packing_check.cpp).
#include <cmath>
#include <cstring>
#include <string>

#include "../device/depth_prepass_raster.h"
#include "frame_pipeline.h"

namespace plrhost {

void refuseNonFiniteMatrices(const float* matrices16, uint32_t drawCount, const char* call) {
    for (uint32_t d = 0; d < drawCount; d++)
        for (int e = 0; e < 16; e++)
            if (!std::isfinite(matrices16[(size_t)d * 16u + e]))
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": non-finite matrix element: element " + std::to_string(e) + " of the model matrix of draw " +
                                           std::to_string(d));
}

// everything is validated before anything is built; the caller changes its state only with the result in hand
PackedScene packSceneMeshes(const SceneMesh* meshes, uint32_t meshCount, const SceneDraw* draws, uint32_t drawCount) {
    const char* call = "setSceneMeshes";
    if (!meshes || !draws || meshCount == 0 || drawCount == 0) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": draws without meshes");
    std::vector<uint32_t> firstIndex(meshCount), vertexOffset(meshCount);
    uint64_t vertices = 0, indices = 0, triangles = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        const SceneMesh& mesh = meshes[m];
        if ((mesh.vertexCount && !mesh.positions) || (mesh.indexCount && !mesh.indices)) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": mesh " + std::to_string(m) + " has null data");
        if (mesh.indexCount % 3u != 0u)
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": mesh " + std::to_string(m) + " has " + std::to_string(mesh.indexCount) + " indices, not a triangle list");
        for (uint32_t i = 0; i < mesh.indexCount; i++)
            if (mesh.indices[i] >= mesh.vertexCount)
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": vertex index out of range: index " + std::to_string(i) + " of mesh " + std::to_string(m) + " is " +
                                           std::to_string(mesh.indices[i]) + ", the mesh has " + std::to_string(mesh.vertexCount) + " vertices");
        firstIndex[m] = (uint32_t)indices; vertexOffset[m] = (uint32_t)vertices;
        vertices += mesh.vertexCount; indices += mesh.indexCount;
    }
    for (uint32_t d = 0; d < drawCount; d++) {
        if (draws[d].mesh >= meshCount)
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": mesh index out of range: draw " + std::to_string(d) + " names mesh " + std::to_string(draws[d].mesh) +
                                       " of " + std::to_string(meshCount));
        triangles += meshes[draws[d].mesh].indexCount / 3u;
    }
    for (uint32_t d = 0; d < drawCount; d++)
        for (int e = 0; e < 16; e++)
            if (!std::isfinite(draws[d].modelMatrix[e]))
                throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": non-finite matrix element: element " + std::to_string(e) + " of the model matrix of draw " + std::to_string(d));
    if (vertices == 0 || indices == 0 || triangles == 0) throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": the draws hold no triangle");
    if (vertices > 0xffffffffull || indices > 0xffffffffull || triangles > (uint64_t)plr::prepass::kMaxTriangles)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": too many vertices, indices or triangles");
    PackedScene out;
    out.positions.resize((size_t)vertices * 3u);
    out.normals.assign((size_t)vertices * 3u, 0.f); // all-zero: the pass takes the face normal
    out.indices.resize((size_t)indices);
    out.models.resize((size_t)drawCount * 16u);
    out.draws.resize((size_t)drawCount * 6u);
    for (uint32_t m = 0; m < meshCount; m++) {
        if (meshes[m].vertexCount) std::memcpy(out.positions.data() + (size_t)vertexOffset[m] * 3u, meshes[m].positions, (size_t)meshes[m].vertexCount * 12u);
        if (meshes[m].vertexCount && meshes[m].normals) std::memcpy(out.normals.data() + (size_t)vertexOffset[m] * 3u, meshes[m].normals, (size_t)meshes[m].vertexCount * 12u);
        if (meshes[m].indexCount) std::memcpy(out.indices.data() + firstIndex[m], meshes[m].indices, (size_t)meshes[m].indexCount * 4u);
    }
    for (uint32_t d = 0; d < drawCount; d++) {
        const plr::prepass::Draw draw{firstIndex[draws[d].mesh], meshes[draws[d].mesh].indexCount, vertexOffset[draws[d].mesh], d, draws[d].albedo, draws[d].specular};
        std::memcpy(out.draws.data() + (size_t)d * 6u, &draw, sizeof(draw));
        std::memcpy(out.models.data() + (size_t)d * 16u, draws[d].modelMatrix, 64);
    }
    out.triangleCount = (uint32_t)triangles;
    return out;
}

} // namespace plrhost
