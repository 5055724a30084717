// Validation and packing of scene meshes, their material textures, their alpha cutoffs and their normal maps for "depthPrepassRaster.comp"
// (FramePipeline::setSceneMeshes, setSceneTextures, setSceneTexturesFormatted, setSceneAlphaCutoffs, setSceneNormalMaps) and of the shadow casters and their
// cutouts for "sunShadowRaster.comp" (setShadowCasters, setShadowCasterCutouts, setShadowCasterCutoutsFormatted), the host's decoder and encoder of BC1 / BC3 / BC5 blocks, and the layout and job
// tables of the texture store the GPU builds (buildSceneTextures: "textureMipChain.comp", "textureBlockEncode.comp"): host code without a backend
// call, so that a stand-alone program can run it under a sanitizer (tools/scene_packing_check.cpp for both mesh sets, tools/scene_texture_check.cpp,
// tools/scene_alpha_check.cpp, tools/scene_normal_check.cpp, tools/shadow_cutout_check.cpp, tools/shadow_cutout_bc_check.cpp, tools/scene_bc_check.cpp,
// tools/draw_bounds_check.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../device/depth_prepass_raster.h"
#include "../device/sun_shadow_raster.h"
#include "../device/texture_build.h"
#include "frame_pipeline.h"

namespace plrhost {

static void refuseNonFiniteMatrix(const float* m, uint32_t draw, const char* call) {
    for (int e = 0; e < 16; e++)
        if (!std::isfinite(m[e]))
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": non-finite matrix element: element " + std::to_string(e) + " of the model matrix of draw " +
                                       std::to_string(draw));
}

void refuseNonFiniteMatrices(const float* matrices16, uint32_t drawCount, const char* call) {
    for (uint32_t d = 0; d < drawCount; d++) refuseNonFiniteMatrix(matrices16 + (size_t)d * 16u, d, call);
}

std::vector<float> packDrawBounds(const float* const* meshPositions, const uint32_t* meshVertexCounts, uint32_t meshCount, const uint32_t* drawMeshes, uint32_t drawCount) {
    std::vector<float> boxes((size_t)meshCount * 6u, 0.f); // (a mesh without vertices: all zero; its draws hold no triangle)
    for (uint32_t m = 0; m < meshCount; m++) {
        const float* p = meshPositions[m];
        const uint32_t n = meshVertexCounts[m];
        if (n == 0 || !p) continue;
        float* box = boxes.data() + (size_t)m * 6u;
        for (int a = 0; a < 3; a++) {
            float lo = p[a], hi = p[a];
            bool nan = lo != lo;
            for (uint32_t v = 1; v < n; v++) {
                const float x = p[(size_t)v * 3u + a];
                if (x != x) nan = true;
                if (x < lo) lo = x;
                if (x > hi) hi = x;
            }
            box[a] = nan ? std::nanf("") : lo;
            box[3 + a] = nan ? std::nanf("") : hi;
        }
    }
    std::vector<float> out((size_t)drawCount * 6u);
    for (uint32_t d = 0; d < drawCount; d++) {
        if (drawMeshes[d] >= meshCount)
            throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, "packDrawBounds: mesh index out of range: draw " + std::to_string(d) + " names mesh " + std::to_string(drawMeshes[d]) + " of " + std::to_string(meshCount));
        std::memcpy(out.data() + (size_t)d * 6u, boxes.data() + (size_t)drawMeshes[d] * 6u, 24);
    }
    return out;
}

void refuseUnlessAffine(const float* m, uint32_t draw, const char* call) {
    if (m[3] != 0.f || m[7] != 0.f || m[11] != 0.f || m[15] != 1.f)
        throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, std::string(call) + ": the model matrix of draw " + std::to_string(draw) +
                                   " is not affine (its last row must be exactly (0, 0, 0, 1): the shadow pass does not divide by w)");
}

// ---- what the scene's meshes and the shadow casters share: the checks per mesh and of every draw's mesh index, the layout of the meshes back to back, the copies
// and the bounds. `out.draws` stays empty: the draw record is the caller's, from the layout returned with the rest
struct MeshLayout { std::vector<uint32_t> firstIndex, vertexOffset, drawMeshes; };
// the matrix rules differ in their place as well: checkDraw(d) runs right behind the mesh index check of draw d, checkDraws() once behind the last draw, both in
// front of the checks of the totals. Everything is validated before anything is built; the caller changes its state only with the result in hand
template <class Mesh, class Draw, class CheckDraw, class CheckDraws>
static MeshLayout packMeshes(const std::string& call, const Mesh* meshes, uint32_t meshCount, const Draw* draws, uint32_t drawCount, uint64_t maxTriangles, CheckDraw&& checkDraw,
                             CheckDraws&& checkDraws, PackedMeshes& out) {
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (!meshes || !draws || meshCount == 0 || drawCount == 0) refuse("draws without meshes");
    MeshLayout at{std::vector<uint32_t>(meshCount), std::vector<uint32_t>(meshCount), std::vector<uint32_t>(drawCount)};
    uint64_t vertices = 0, indices = 0, triangles = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        const Mesh& mesh = meshes[m];
        if ((mesh.vertexCount && !mesh.positions) || (mesh.indexCount && !mesh.indices)) refuse("mesh " + std::to_string(m) + " has null data");
        if (mesh.indexCount % 3u != 0u) refuse("mesh " + std::to_string(m) + " has " + std::to_string(mesh.indexCount) + " indices, not a triangle list");
        for (uint32_t i = 0; i < mesh.indexCount; i++)
            if (mesh.indices[i] >= mesh.vertexCount)
                refuse("vertex index out of range: index " + std::to_string(i) + " of mesh " + std::to_string(m) + " is " + std::to_string(mesh.indices[i]) + ", the mesh has " +
                       std::to_string(mesh.vertexCount) + " vertices");
        at.firstIndex[m] = (uint32_t)indices; at.vertexOffset[m] = (uint32_t)vertices;
        vertices += mesh.vertexCount; indices += mesh.indexCount;
    }
    for (uint32_t d = 0; d < drawCount; d++) {
        if (draws[d].mesh >= meshCount) refuse("mesh index out of range: draw " + std::to_string(d) + " names mesh " + std::to_string(draws[d].mesh) + " of " + std::to_string(meshCount));
        checkDraw(d);
        triangles += meshes[draws[d].mesh].indexCount / 3u;
    }
    checkDraws();
    if (vertices == 0 || indices == 0 || triangles == 0) refuse("the draws hold no triangle");
    if (vertices > 0xffffffffull || indices > 0xffffffffull || triangles > maxTriangles) refuse("too many vertices, indices or triangles");
    out.positions.resize((size_t)vertices * 3u);
    out.indices.resize((size_t)indices);
    out.models.resize((size_t)drawCount * 16u);
    out.meshVertexCounts.resize(meshCount);
    std::vector<const float*> meshPositions(meshCount);
    for (uint32_t m = 0; m < meshCount; m++) {
        if (meshes[m].vertexCount) std::memcpy(out.positions.data() + (size_t)at.vertexOffset[m] * 3u, meshes[m].positions, (size_t)meshes[m].vertexCount * 12u);
        if (meshes[m].indexCount) std::memcpy(out.indices.data() + at.firstIndex[m], meshes[m].indices, (size_t)meshes[m].indexCount * 4u);
        out.meshVertexCounts[m] = meshes[m].vertexCount;
        meshPositions[m] = meshes[m].positions;
    }
    for (uint32_t d = 0; d < drawCount; d++) {
        std::memcpy(out.models.data() + (size_t)d * 16u, draws[d].modelMatrix, 64);
        at.drawMeshes[d] = draws[d].mesh;
    }
    out.triangleCount = (uint32_t)triangles;
    out.drawBounds = packDrawBounds(meshPositions.data(), out.meshVertexCounts.data(), meshCount, at.drawMeshes.data(), drawCount);
    return at;
}

PackedScene packSceneMeshes(const SceneMesh* meshes, uint32_t meshCount, const SceneDraw* draws, uint32_t drawCount) {
    const char* call = "setSceneMeshes";
    PackedScene out;
    // every element of every matrix is finite: checked once every draw names a mesh
    const MeshLayout at = packMeshes(call, meshes, meshCount, draws, drawCount, plr::prepass::kMaxTriangles, [](uint32_t) {},
                                     [&] { for (uint32_t d = 0; d < drawCount; d++) refuseNonFiniteMatrix(draws[d].modelMatrix, d, call); }, out);
    out.normals.assign(out.positions.size(), 0.f); // all-zero: the pass takes the face normal
    out.meshHasNormals.resize(meshCount);
    out.meshIndexCounts.resize(meshCount);
    for (uint32_t m = 0; m < meshCount; m++) {
        if (meshes[m].vertexCount && meshes[m].normals) std::memcpy(out.normals.data() + (size_t)at.vertexOffset[m] * 3u, meshes[m].normals, (size_t)meshes[m].vertexCount * 12u);
        out.meshHasNormals[m] = meshes[m].normals ? 1 : 0;
        out.meshIndexCounts[m] = meshes[m].indexCount;
    }
    out.draws.resize((size_t)drawCount * 6u);
    for (uint32_t d = 0; d < drawCount; d++) {
        const uint32_t m = draws[d].mesh;
        const plr::prepass::Draw draw{at.firstIndex[m], meshes[m].indexCount, at.vertexOffset[m], d, draws[d].albedo, draws[d].specular};
        std::memcpy(out.draws.data() + (size_t)d * 6u, &draw, sizeof(draw));
    }
    out.drawMeshes = at.drawMeshes;
    out.meshFirstIndex = at.firstIndex;
    return out;
}

PackedCasters packShadowCasters(const ShadowCasterMesh* meshes, uint32_t meshCount, const ShadowCasterDraw* draws, uint32_t drawCount) {
    const char* call = "setShadowCasters";
    PackedCasters out;
    // the last row of a matrix is (0, 0, 0, 1): checked draw by draw, behind the draw's mesh index
    const MeshLayout at = packMeshes(call, meshes, meshCount, draws, drawCount, 0x7fffffffull, [&](uint32_t d) { refuseUnlessAffine(draws[d].modelMatrix, d, call); }, [] {}, out);
    out.draws.resize((size_t)drawCount * 4u);
    for (uint32_t d = 0; d < drawCount; d++) {
        const uint32_t m = draws[d].mesh;
        const plr::sunraster::Draw draw{at.firstIndex[m], meshes[m].indexCount, at.vertexOffset[m], d};
        std::memcpy(out.draws.data() + (size_t)d * 4u, &draw, sizeof(draw));
    }
    return out;
}

void appendMipChain(std::vector<uint32_t>& texels, uint32_t width, uint32_t height) {
    size_t src = texels.size() - (size_t)width * height;
    for (uint32_t w = width, h = height; w > 1u || h > 1u;) {
        const uint32_t nw = w > 1u ? w >> 1 : 1u, nh = h > 1u ? h >> 1 : 1u;
        const size_t dst = texels.size();
        texels.resize(dst + (size_t)nw * nh);
        for (uint32_t y = 0; y < nh; y++) {
            const uint32_t y0 = std::min(2u * y, h - 1u), y1 = std::min(2u * y + 1u, h - 1u);
            for (uint32_t x = 0; x < nw; x++) {
                const uint32_t x0 = std::min(2u * x, w - 1u), x1 = std::min(2u * x + 1u, w - 1u);
                const uint32_t a = texels[src + (size_t)y0 * w + x0], b = texels[src + (size_t)y0 * w + x1], c = texels[src + (size_t)y1 * w + x0], d = texels[src + (size_t)y1 * w + x1];
                uint32_t word = 0;
                for (int k = 0; k < 32; k += 8) word |= ((((a >> k) & 255u) + ((b >> k) & 255u) + ((c >> k) & 255u) + ((d >> k) & 255u) + 2u) >> 2) << k;
                texels[dst + (size_t)y * nw + x] = word;
            }
        }
        src = dst; w = nw; h = nh;
    }
}

// ---- the texture store and the UVs, shared by the scene's textures and the shadow casters' cutouts: `refuse` throws with the call's name in front
// size, mip count and data pointer of texture t, the rules every texture call shares; returns the levels of its full chain
template <class Refuse> static uint32_t validateTextureShape(uint32_t t, uint32_t width, uint32_t height, uint32_t mipCount, const void* data, Refuse&& refuse) {
    namespace pp = plr::prepass;
    if (width < 1u || height < 1u || width > pp::kMaxTextureSize || height > pp::kMaxTextureSize)
        refuse("texture size out of range: texture " + std::to_string(t) + " is " + std::to_string(width) + " x " + std::to_string(height) + ", each side must be 1 .. 16384");
    const uint32_t full = pp::fullMipCount(width, height);
    if (mipCount > full)
        refuse("too many mips: texture " + std::to_string(t) + " (" + std::to_string(width) + " x " + std::to_string(height) + ") has " + std::to_string(mipCount) + " levels, at most " + std::to_string(full));
    if (!data) refuse("null texels: texture " + std::to_string(t));
    return full;
}

template <class Refuse> static uint64_t validateTextures(const SceneTexture* textures, uint32_t textureCount, Refuse&& refuse) {
    uint64_t total = 0;
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTexture& tex = textures[t];
        const uint32_t full = validateTextureShape(t, tex.width, tex.height, tex.mipCount, tex.texels, refuse);
        const uint32_t levels = tex.mipCount ? tex.mipCount : full;
        for (uint32_t l = 0; l < levels; l++) total += (uint64_t)std::max(1u, tex.width >> l) * std::max(1u, tex.height >> l);
    }
    return total;
}

// the UVs of the meshes back to back, zeros for a mesh given without; refuses a non-finite one
template <class Refuse> static std::vector<float> packUvs(const float* const* meshUvs, uint32_t meshCount, const uint32_t* meshVertexCounts, Refuse&& refuse) {
    uint64_t vertices = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        if (meshUvs && meshUvs[m])
            for (size_t i = 0; i < (size_t)meshVertexCounts[m] * 2u; i++)
                if (!std::isfinite(meshUvs[m][i]))
                    refuse("non-finite UV: vertex " + std::to_string(i / 2u) + " of mesh " + std::to_string(m));
        vertices += meshVertexCounts[m];
    }
    std::vector<float> uvs((size_t)vertices * 2u, 0.f);
    size_t at = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        if (meshUvs && meshUvs[m] && meshVertexCounts[m]) std::memcpy(uvs.data() + at, meshUvs[m], (size_t)meshVertexCounts[m] * 8u);
        at += (size_t)meshVertexCounts[m] * 2u;
    }
    return uvs;
}

// the table {texelOffset, width, height, mipCount} and the texels of validated textures, a chain built where mipCount is 0
static void packTextureStore(const SceneTexture* textures, uint32_t textureCount, uint64_t total, std::vector<uint32_t>& table, std::vector<uint32_t>& texels) {
    namespace pp = plr::prepass;
    table.resize((size_t)textureCount * 4u);
    texels.reserve((size_t)total);
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTexture& tex = textures[t];
        const pp::Texture entry{(uint32_t)texels.size(), tex.width, tex.height, tex.mipCount ? tex.mipCount : pp::fullMipCount(tex.width, tex.height)};
        std::memcpy(table.data() + (size_t)t * 4u, &entry, sizeof(entry));
        size_t given = 0;
        for (uint32_t l = 0; l < std::max(1u, tex.mipCount); l++) given += (size_t)std::max(1u, tex.width >> l) * std::max(1u, tex.height >> l);
        texels.insert(texels.end(), tex.texels, tex.texels + given);
        if (tex.mipCount == 0) appendMipChain(texels, tex.width, tex.height);
    }
}

// everything is validated before anything is built
PackedTextures packSceneTextures(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                 uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount) {
    namespace pp = plr::prepass;
    const std::string call = "setSceneTextures";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (sceneDrawCount == 0) refuse("no scene set (plrf_set_scene_meshes comes first)");
    if (meshCount != sceneMeshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(sceneMeshCount) + " of the scene");
    if (drawCount != sceneDrawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(sceneDrawCount) + " of the scene");
    if (!textures || !materials) refuse("textures or materials are null");
    const uint64_t total = validateTextures(textures, textureCount, refuse);
    for (uint32_t d = 0; d < drawCount; d++)
        for (uint32_t index : {materials[d].albedoTexture, materials[d].specularTexture})
            if (index != kNoSceneTexture && index >= textureCount)
                refuse("material texture index out of range: draw " + std::to_string(d) + " names texture " + std::to_string(index) + " of " + std::to_string(textureCount));
    if (total > pp::kMaxTexels) refuse("too many texels: " + std::to_string(total) + " in all levels of all textures, at most 2^28");
    PackedTextures out;
    out.uvs = packUvs(meshUvs, meshCount, sceneMeshVertexCounts, refuse);
    out.materials.resize((size_t)drawCount * 2u);
    for (uint32_t d = 0; d < drawCount; d++) { out.materials[2u * d] = materials[d].albedoTexture; out.materials[2u * d + 1u] = materials[d].specularTexture; }
    packTextureStore(textures, textureCount, total, out.textures, out.texels);
    return out;
}

// ---- block-compressed textures (DESIGN.md "Block-compressed textures in the depth prepass")
// the contract's format code of a PLR_FORMAT_* value, or -1
static int textureFormatCode(uint32_t format) {
    namespace pp = plr::prepass;
    switch (format) {
    case PLR_FORMAT_RGBA8: return (int)pp::kTextureFormatRgba8;
    case PLR_FORMAT_BC1: return (int)pp::kTextureFormatBc1;
    case PLR_FORMAT_BC3: return (int)pp::kTextureFormatBc3;
    case PLR_FORMAT_BC5: return (int)pp::kTextureFormatBc5;
    default: return -1;
    }
}

// ---- the format-aware store, shared by the scene's textures (setSceneTexturesFormatted) and the shadow casters' cutouts (setShadowCasterCutoutsFormatted): the
// checks per texture and the layout first, the store once the call's other checks have passed. `refuse` throws with the call's name in front
struct FormattedLayout { std::vector<uint32_t> codes, offsets; uint64_t total = 0; }; // per texture the contract's format code and the word offset; the words in all
template <class Refuse> static FormattedLayout validateFormattedTextures(const SceneTextureData* textures, uint32_t textureCount, Refuse&& refuse) {
    namespace pp = plr::prepass;
    FormattedLayout at{std::vector<uint32_t>(textureCount), std::vector<uint32_t>(textureCount), 0};
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTextureData& tex = textures[t];
        const int code = textureFormatCode(tex.format);
        if (code < 0)
            refuse("unknown format: texture " + std::to_string(t) + " has format " + std::to_string(tex.format) + ", it must be PLR_FORMAT_RGBA8, PLR_FORMAT_BC1, PLR_FORMAT_BC3 or PLR_FORMAT_BC5");
        const uint32_t full = validateTextureShape(t, tex.width, tex.height, tex.mipCount, tex.data, refuse);
        const bool blocks = (uint32_t)code != pp::kTextureFormatRgba8;
        if (blocks && tex.mipCount == 0)
            refuse("mip_count 0 on a compressed texture: texture " + std::to_string(t) + " (the host has no encoder to build a chain with: give its levels)");
        const uint64_t given = pp::textureWords((uint32_t)code, tex.width, tex.height, std::max(1u, tex.mipCount)) * 4u;
        if (tex.bytes != given)
            refuse("bytes mismatch: texture " + std::to_string(t) + " (" + std::to_string(tex.width) + " x " + std::to_string(tex.height) + ", " + std::to_string(std::max(1u, tex.mipCount)) +
                   " level(s)) has " + std::to_string(tex.bytes) + " bytes, its levels hold " + std::to_string(given));
        if (blocks) at.total = (at.total + 3u) & ~(uint64_t)3u;
        at.offsets[t] = (uint32_t)std::min<uint64_t>(at.total, 0xffffffffu); // (a total that does not fit is refused by the caller)
        at.total += pp::textureWords((uint32_t)code, tex.width, tex.height, tex.mipCount ? tex.mipCount : full);
        at.codes[t] = (uint32_t)code;
    }
    return at;
}
// An RGBA8 entry is packed as packTextureStore packs it; a compressed one starts at a multiple of 4 words (16 bytes), zeros in front of it where needed. Returns
// whether an entry is compressed: without one the table and the words are packTextureStore's own
static bool packFormattedStore(const SceneTextureData* textures, uint32_t textureCount, const FormattedLayout& at, std::vector<uint32_t>& table, std::vector<uint32_t>& words) {
    namespace pp = plr::prepass;
    bool compressed = false;
    table.resize((size_t)textureCount * 4u);
    words.reserve((size_t)at.total);
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTextureData& tex = textures[t];
        words.resize(at.offsets[t], 0u); // (the padding in front of a compressed texture)
        const pp::Texture entry{at.offsets[t], tex.width, tex.height, tex.mipCount ? tex.mipCount : pp::fullMipCount(tex.width, tex.height)};
        std::memcpy(table.data() + (size_t)t * 4u, &entry, sizeof(entry));
        const size_t given = (size_t)(tex.bytes / 4u);
        words.resize(words.size() + given);
        std::memcpy(words.data() + at.offsets[t], tex.data, given * 4u); // (the caller's data may sit at any alignment)
        if (tex.mipCount == 0) appendMipChain(words, tex.width, tex.height);
        compressed = compressed || at.codes[t] != pp::kTextureFormatRgba8;
    }
    return compressed;
}

// everything is validated before anything is built. Without a compressed entry the result is packSceneTextures' own, and `compressed` stays false
PackedFormattedTextures packSceneTexturesFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                                   uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount) {
    namespace pp = plr::prepass;
    const std::string call = "setSceneTexturesFormatted";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (sceneDrawCount == 0) refuse("no scene set (plrf_set_scene_meshes comes first)");
    if (meshCount != sceneMeshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(sceneMeshCount) + " of the scene");
    if (drawCount != sceneDrawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(sceneDrawCount) + " of the scene");
    if (!textures || !materials) refuse("textures or materials are null");
    const FormattedLayout at = validateFormattedTextures(textures, textureCount, refuse);
    for (uint32_t d = 0; d < drawCount; d++)
        for (uint32_t index : {materials[d].albedoTexture, materials[d].specularTexture})
            if (index != kNoSceneTexture && index >= textureCount)
                refuse("material texture index out of range: draw " + std::to_string(d) + " names texture " + std::to_string(index) + " of " + std::to_string(textureCount));
    if (at.total > pp::kMaxTexels) refuse("too many texels: " + std::to_string(at.total) + " words in all levels of all textures, at most 2^28");
    PackedFormattedTextures out;
    out.uvs = packUvs(meshUvs, meshCount, sceneMeshVertexCounts, refuse);
    out.materials.resize((size_t)drawCount * 2u);
    for (uint32_t d = 0; d < drawCount; d++) { out.materials[2u * d] = materials[d].albedoTexture; out.materials[2u * d + 1u] = materials[d].specularTexture; }
    out.compressed = packFormattedStore(textures, textureCount, at, out.textures, out.texels);
    out.formats = at.codes;
    return out;
}

// the contract's colour block: texel i as r | g << 8 | b << 16
static uint32_t colourBlockTexel(const uint8_t* b, uint32_t i, bool alwaysFour) {
    const uint32_t c0 = (uint32_t)b[0] | ((uint32_t)b[1] << 8), c1 = (uint32_t)b[2] | ((uint32_t)b[3] << 8);
    const uint32_t indices = (uint32_t)b[4] | ((uint32_t)b[5] << 8) | ((uint32_t)b[6] << 16) | ((uint32_t)b[7] << 24);
    const uint32_t k = (indices >> (2u * i)) & 3u;
    const bool four = alwaysFour || c0 > c1;
    auto expand = [](uint32_t c, int channel) { // RGB565, red in the high bits
        const uint32_t r5 = (c >> 11) & 31u, g6 = (c >> 5) & 63u, b5 = c & 31u;
        return channel == 0 ? (r5 << 3) | (r5 >> 2) : channel == 1 ? (g6 << 2) | (g6 >> 4) : (b5 << 3) | (b5 >> 2);
    };
    uint32_t word = 0;
    for (int channel = 0; channel < 3; channel++) {
        const uint32_t e0 = expand(c0, channel), e1 = expand(c1, channel);
        uint32_t c;
        if (k == 0u) c = e0;
        else if (k == 1u) c = e1;
        else if (four) c = k == 2u ? (2u * e0 + e1 + 1u) / 3u : (e0 + 2u * e1 + 1u) / 3u;
        else c = k == 2u ? (e0 + e1 + 1u) >> 1 : 0u;
        word |= c << (8 * channel);
    }
    return word;
}
// the contract's alpha block: the code of texel i
static uint32_t alphaBlockTexel(const uint8_t* b, uint32_t i) {
    const uint32_t a0 = b[0], a1 = b[1];
    uint64_t bits = 0;
    for (int k = 0; k < 6; k++) bits |= (uint64_t)b[2 + k] << (8 * k);
    const uint32_t k = (uint32_t)((bits >> (3u * i)) & 7u);
    if (k == 0u) return a0;
    if (k == 1u) return a1;
    if (a0 > a1) return ((8u - k) * a0 + (k - 1u) * a1 + 3u) / 7u;
    if (k == 6u) return 0u;
    if (k == 7u) return 255u;
    return ((6u - k) * a0 + (k - 1u) * a1 + 2u) / 5u;
}

void decodeBlockCompressedLevel(uint32_t format, uint32_t width, uint32_t height, const void* blocks, uint64_t bytes, uint32_t* outWords) {
    namespace pp = plr::prepass;
    const std::string call = "plr_decode_bc_to_rgba8";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    const int code = textureFormatCode(format);
    if (code <= 0) refuse("format " + std::to_string(format) + " is not PLR_FORMAT_BC1, PLR_FORMAT_BC3 or PLR_FORMAT_BC5");
    if (width < 1u || height < 1u || width > pp::kMaxTextureSize || height > pp::kMaxTextureSize)
        refuse("the level is " + std::to_string(width) + " x " + std::to_string(height) + ", each side must be 1 .. 16384");
    if (!blocks || !outWords) refuse("blocks or out_words are null");
    const uint64_t need = pp::textureWords((uint32_t)code, width, height, 1) * 4u;
    if (bytes != need)
        refuse("bytes mismatch: " + std::to_string(bytes) + " bytes for a " + std::to_string(width) + " x " + std::to_string(height) + " level that holds " + std::to_string(need));
    const size_t blockBytes = (size_t)pp::blockWords((uint32_t)code) * 4u, blocksPerRow = ((size_t)width + 3u) / 4u;
    const uint8_t* data = (const uint8_t*)blocks;
    for (uint32_t y = 0; y < height; y++)
        for (uint32_t x = 0; x < width; x++) {
            const uint8_t* b = data + ((size_t)(y >> 2) * blocksPerRow + (x >> 2)) * blockBytes;
            const uint32_t i = 4u * (y & 3u) + (x & 3u);
            uint32_t word;
            if ((uint32_t)code == pp::kTextureFormatBc1) word = colourBlockTexel(b, i, false) | (255u << 24);
            else if ((uint32_t)code == pp::kTextureFormatBc3) word = colourBlockTexel(b + 8, i, true) | (alphaBlockTexel(b, i) << 24);
            else word = alphaBlockTexel(b, i) | (alphaBlockTexel(b + 8, i) << 8) | (255u << 24);
            outWords[(size_t)y * width + x] = word;
        }
}

// ---- the texture store built on the GPU (DESIGN.md "Texture store built on the GPU")
void encodeBlockCompressedLevel(uint32_t format, uint32_t width, uint32_t height, const uint32_t* words, void* outBlocks, uint64_t bytes) {
    namespace pp = plr::prepass;
    const std::string call = "plr_encode_rgba8_to_bc";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    const int code = textureFormatCode(format);
    if (code <= 0) refuse("format " + std::to_string(format) + " is not PLR_FORMAT_BC1, PLR_FORMAT_BC3 or PLR_FORMAT_BC5");
    if (width < 1u || height < 1u || width > pp::kMaxTextureSize || height > pp::kMaxTextureSize)
        refuse("the level is " + std::to_string(width) + " x " + std::to_string(height) + ", each side must be 1 .. 16384");
    if (!words || !outBlocks) refuse("words or out_blocks are null");
    const uint64_t need = pp::textureWords((uint32_t)code, width, height, 1) * 4u;
    if (bytes != need)
        refuse("bytes mismatch: " + std::to_string(bytes) + " bytes for a " + std::to_string(width) + " x " + std::to_string(height) + " level whose blocks hold " + std::to_string(need));
    const size_t blockBytes = (size_t)pp::blockWords((uint32_t)code) * 4u, blocksX = ((size_t)width + 3u) / 4u, blocksY = ((size_t)height + 3u) / 4u;
    uint8_t* out = (uint8_t*)outBlocks;
    for (size_t by = 0; by < blocksY; by++)
        for (size_t bx = 0; bx < blocksX; bx++) {
            uint32_t t[16], block[4];
            for (uint32_t j = 0; j < 4u; j++)
                for (uint32_t i = 0; i < 4u; i++)
                    t[4u * j + i] = words[std::min<size_t>(4u * by + j, height - 1u) * width + std::min<size_t>(4u * bx + i, width - 1u)];
            plr::texbuild::encodeBlock((uint32_t)code, t, block);
            std::memcpy(out + (by * blocksX + bx) * blockBytes, block, blockBytes); // (the caller's buffer may sit at any alignment)
        }
}

// everything is validated before anything is laid out. The store's layout is packSceneTexturesFormatted's for the same textures with all their levels
PackedTextureBuild packSceneTextureBuild(const SceneTextureSource* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const SceneMaterial* materials,
                                         uint32_t drawCount, const uint32_t* sceneMeshVertexCounts, uint32_t sceneMeshCount, uint32_t sceneDrawCount) {
    namespace pp = plr::prepass;
    namespace tb = plr::texbuild;
    const std::string call = "buildSceneTextures";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (sceneDrawCount == 0) refuse("no scene set (plrf_set_scene_meshes comes first)");
    if (meshCount != sceneMeshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(sceneMeshCount) + " of the scene");
    if (drawCount != sceneDrawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(sceneDrawCount) + " of the scene");
    if (!textures || !materials) refuse("textures or materials are null");
    struct Plan { uint32_t source, stored, levels, given, offset; uint64_t staging; }; // format codes; levels of the store entry; levels the caller gave; word offsets
    std::vector<Plan> plans(textureCount);
    uint64_t total = 0, staging = 0;
    auto levelWords = [](uint32_t code, uint32_t w, uint32_t h) { return pp::textureWords(code, w, h, 1); };
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTextureSource& tex = textures[t];
        const int source = textureFormatCode(tex.format), stored = textureFormatCode(tex.storeFormat);
        if (source < 0 || stored < 0 || (source != (int)pp::kTextureFormatRgba8 && source != stored))
            refuse("unsupported format pair: texture " + std::to_string(t) + " has format " + std::to_string(tex.format) + " and store_format " + std::to_string(tex.storeFormat) +
                   " (an RGBA8 source is stored as RGBA8, BC1, BC3 or BC5; a BC1, BC3 or BC5 source as what it is)");
        const uint32_t full = validateTextureShape(t, tex.width, tex.height, tex.mipCount, tex.data, refuse);
        Plan& plan = plans[t];
        plan.source = (uint32_t)source; plan.stored = (uint32_t)stored; plan.levels = tex.mipCount ? tex.mipCount : full; plan.given = std::max(1u, tex.mipCount);
        const uint64_t given = pp::textureWords(plan.source, tex.width, tex.height, plan.given) * 4u;
        if (tex.bytes != given)
            refuse("bytes mismatch: texture " + std::to_string(t) + " (" + std::to_string(tex.width) + " x " + std::to_string(tex.height) + ", " + std::to_string(plan.given) +
                   " level(s)) has " + std::to_string(tex.bytes) + " bytes, its levels hold " + std::to_string(given));
        if (plan.stored != pp::kTextureFormatRgba8) total = (total + 3u) & ~(uint64_t)3u;
        plan.offset = (uint32_t)std::min<uint64_t>(total, 0xffffffffu); // (a total that does not fit is refused below)
        total += pp::textureWords(plan.stored, tex.width, tex.height, plan.levels);
        // staging: every level of an RGBA8 source that is encoded; levels 1 .. of a compressed source whose chain is built. Each level at a multiple of 4 words
        plan.staging = staging;
        const bool encoded = plan.source == pp::kTextureFormatRgba8 && plan.stored != pp::kTextureFormatRgba8, chained = plan.source != pp::kTextureFormatRgba8 && tex.mipCount == 0;
        if (encoded || chained)
            for (uint32_t l = encoded ? 0u : 1u; l < plan.levels; l++) staging += (levelWords(pp::kTextureFormatRgba8, std::max(1u, tex.width >> l), std::max(1u, tex.height >> l)) + 3u) & ~(uint64_t)3u;
    }
    for (uint32_t d = 0; d < drawCount; d++)
        for (uint32_t index : {materials[d].albedoTexture, materials[d].specularTexture})
            if (index != kNoSceneTexture && index >= textureCount)
                refuse("material texture index out of range: draw " + std::to_string(d) + " names texture " + std::to_string(index) + " of " + std::to_string(textureCount));
    if (total > pp::kMaxTexels) refuse("too many texels: " + std::to_string(total) + " words in all levels of all textures, at most 2^28");
    if (staging > tb::kMaxStagingWords) refuse("too many staging texels: the RGBA8 chains the build needs hold " + std::to_string(staging) + " words, at most 2^28");
    PackedTextureBuild out;
    out.uvs = packUvs(meshUvs, meshCount, sceneMeshVertexCounts, refuse);
    out.materials.resize((size_t)drawCount * 2u);
    for (uint32_t d = 0; d < drawCount; d++) { out.materials[2u * d] = materials[d].albedoTexture; out.materials[2u * d + 1u] = materials[d].specularTexture; }
    out.textures.resize((size_t)textureCount * 4u);
    out.texels.assign((size_t)total, 0u);
    out.staging.assign((size_t)staging, 0u);
    out.formats.resize(textureCount);
    std::vector<std::vector<tb::ChainJob>> chain(tb::kMaxChainLaunches + 1u); // by the level built
    std::vector<tb::EncodeJob> encode;
    for (uint32_t t = 0; t < textureCount; t++) {
        const SceneTextureSource& tex = textures[t];
        const Plan& plan = plans[t];
        const pp::Texture entry{plan.offset, tex.width, tex.height, plan.levels};
        std::memcpy(out.textures.data() + (size_t)t * 4u, &entry, sizeof(entry));
        out.formats[t] = plan.stored;
        out.compressed = out.compressed || plan.stored != pp::kTextureFormatRgba8;
        const bool rgbaSource = plan.source == pp::kTextureFormatRgba8, encoded = rgbaSource && plan.stored != pp::kTextureFormatRgba8;
        // where level l lives while the build runs: {word offset, in the staging buffer}
        std::vector<uint32_t> storeAt(plan.levels), stagingAt(plan.levels, 0u);
        uint64_t s = plan.offset, g = plan.staging;
        for (uint32_t l = 0; l < plan.levels; l++) {
            const uint32_t w = std::max(1u, tex.width >> l), h = std::max(1u, tex.height >> l);
            storeAt[l] = (uint32_t)s; s += levelWords(plan.stored, w, h);
            if (encoded || (!rgbaSource && tex.mipCount == 0 && l >= 1u)) { stagingAt[l] = (uint32_t)g; g += ((uint64_t)w * h + 3u) & ~(uint64_t)3u; }
        }
        // the given levels: into the store where they are stored as given, into the staging chains where they are encoded
        const uint8_t* data = (const uint8_t*)tex.data;
        for (uint32_t l = 0; l < plan.given; l++) {
            const uint32_t w = std::max(1u, tex.width >> l), h = std::max(1u, tex.height >> l);
            const size_t words = (size_t)levelWords(plan.source, w, h);
            std::memcpy((encoded ? out.staging.data() + stagingAt[l] : out.texels.data() + storeAt[l]), data, words * 4u); // (the caller's data may sit at any alignment)
            data += words * 4u;
        }
        const bool staged = encoded || !rgbaSource; // where the chain's levels are built
        for (uint32_t l = plan.given; l < plan.levels; l++) { // (only with mipCount 0: level l from level l - 1)
            const uint32_t w = std::max(1u, tex.width >> (l - 1u)), h = std::max(1u, tex.height >> (l - 1u));
            const bool fromBlocks = !rgbaSource && l == 1u; // level 0 of a compressed source: its blocks, in the store
            tb::ChainJob job{};
            job.src = fromBlocks || !staged ? storeAt[l - 1u] : stagingAt[l - 1u];
            job.dst = staged ? stagingAt[l] : storeAt[l];
            job.srcWidth = w; job.srcHeight = h;
            job.flags = (fromBlocks ? plan.source : pp::kTextureFormatRgba8) | (staged && !fromBlocks ? tb::kChainSrcStaging : 0u) | (staged ? tb::kChainDstStaging : 0u);
            chain[l].push_back(job);
            out.chainTexels += (uint64_t)std::max(1u, w >> 1) * std::max(1u, h >> 1);
        }
        if (staged)
            for (uint32_t l = encoded ? 0u : 1u; l < plan.levels; l++) {
                if (!encoded && tex.mipCount != 0) break; // a compressed source with its levels: nothing to encode
                tb::EncodeJob job{};
                job.src = stagingAt[l]; job.dst = storeAt[l];
                job.width = std::max(1u, tex.width >> l); job.height = std::max(1u, tex.height >> l); job.format = plan.stored;
                encode.push_back(job);
                out.blocksEncoded += (uint64_t)((job.width + 3u) / 4u) * ((job.height + 3u) / 4u);
            }
    }
    // the workgroups of the jobs, launch by launch
    for (uint32_t l = 1; l <= tb::kMaxChainLaunches; l++) {
        if (chain[l].empty()) continue;
        uint32_t groups = 0;
        for (tb::ChainJob& job : chain[l]) {
            job.firstGroup = groups;
            groups += (std::max(1u, job.srcWidth >> 1) * std::max(1u, job.srcHeight >> 1) + tb::kGroupLanes - 1u) / tb::kGroupLanes;
        }
        out.chainLaunches.push_back({(uint32_t)(out.chainJobs.size() * 4u / sizeof(tb::ChainJob)), (uint32_t)chain[l].size(), groups});
        const size_t at = out.chainJobs.size();
        out.chainJobs.resize(at + chain[l].size() * (sizeof(tb::ChainJob) / 4u));
        std::memcpy(out.chainJobs.data() + at, chain[l].data(), chain[l].size() * sizeof(tb::ChainJob));
    }
    for (tb::EncodeJob& job : encode) {
        job.firstGroup = out.encodeGroups;
        out.encodeGroups += (((job.width + 3u) / 4u) * ((job.height + 3u) / 4u) + tb::kGroupLanes - 1u) / tb::kGroupLanes;
    }
    out.encodeJobs.resize(encode.size() * (sizeof(tb::EncodeJob) / 4u));
    if (!encode.empty()) std::memcpy(out.encodeJobs.data(), encode.data(), encode.size() * sizeof(tb::EncodeJob));
    return out;
}

// the cutouts of the caster draws, whichever store they index: returns whether a cutoff is not 0
template <class Refuse> static bool validateCutouts(const ShadowCutout* cutouts, uint32_t drawCount, uint32_t textureCount, Refuse&& refuse) {
    bool tested = false;
    for (uint32_t d = 0; d < drawCount; d++) {
        if (cutouts[d].albedoTexture != kNoSceneTexture && cutouts[d].albedoTexture >= textureCount)
            refuse("texture index out of range: draw " + std::to_string(d) + " names texture " + std::to_string(cutouts[d].albedoTexture) + " of " + std::to_string(textureCount));
        if (cutouts[d].alphaCutoff > 255u)
            refuse("cutoff out of range: draw " + std::to_string(d) + " has " + std::to_string(cutouts[d].alphaCutoff) + ", a cutoff code is 0 (opaque) .. 255");
        tested = tested || cutouts[d].alphaCutoff != plr::prepass::kAlphaCutoffOpaque;
    }
    return tested;
}

// everything is validated before anything is built
PackedShadowCutouts packShadowCasterCutouts(const SceneTexture* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount, const ShadowCutout* cutouts,
                                            uint32_t drawCount, const uint32_t* casterMeshVertexCounts, uint32_t casterMeshCount, uint32_t casterDrawCount) {
    namespace pp = plr::prepass;
    const std::string call = "setShadowCasterCutouts";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (casterDrawCount == 0) refuse("no casters set (plrf_set_shadow_casters comes first)");
    if (meshCount != casterMeshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(casterMeshCount) + " of the casters");
    if (drawCount != casterDrawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(casterDrawCount) + " of the casters");
    if (!textures || !cutouts) refuse("textures or cutouts are null");
    const uint64_t total = validateTextures(textures, textureCount, refuse);
    PackedShadowCutouts out;
    out.tested = validateCutouts(cutouts, drawCount, textureCount, refuse);
    if (total > pp::kMaxTexels) refuse("too many texels: " + std::to_string(total) + " in all levels of all textures, at most 2^28");
    out.uvs = packUvs(meshUvs, meshCount, casterMeshVertexCounts, refuse);
    out.materials.resize((size_t)drawCount * 2u);
    for (uint32_t d = 0; d < drawCount; d++) { out.materials[2u * d] = cutouts[d].albedoTexture; out.materials[2u * d + 1u] = cutouts[d].alphaCutoff; }
    packTextureStore(textures, textureCount, total, out.textures, out.texels);
    return out;
}

// everything is validated before anything is built: packShadowCasterCutouts' checks in its order, with the format-aware store's checks per texture
// (validateFormattedTextures) where that one has validateTextures', and the store packed by packFormattedStore
PackedFormattedShadowCutouts packShadowCasterCutoutsFormatted(const SceneTextureData* textures, uint32_t textureCount, const float* const* meshUvs, uint32_t meshCount,
                                                              const ShadowCutout* cutouts, uint32_t drawCount, const uint32_t* casterMeshVertexCounts, uint32_t casterMeshCount,
                                                              uint32_t casterDrawCount) {
    namespace pp = plr::prepass;
    const std::string call = "setShadowCasterCutoutsFormatted";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (casterDrawCount == 0) refuse("no casters set (plrf_set_shadow_casters comes first)");
    if (meshCount != casterMeshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(casterMeshCount) + " of the casters");
    if (drawCount != casterDrawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(casterDrawCount) + " of the casters");
    if (!textures || !cutouts) refuse("textures or cutouts are null");
    const FormattedLayout at = validateFormattedTextures(textures, textureCount, refuse);
    PackedFormattedShadowCutouts out;
    out.tested = validateCutouts(cutouts, drawCount, textureCount, refuse);
    if (at.total > pp::kMaxTexels) refuse("too many texels: " + std::to_string(at.total) + " words in all levels of all textures, at most 2^28");
    out.uvs = packUvs(meshUvs, meshCount, casterMeshVertexCounts, refuse);
    out.materials.resize((size_t)drawCount * 2u);
    for (uint32_t d = 0; d < drawCount; d++) { out.materials[2u * d] = cutouts[d].albedoTexture; out.materials[2u * d + 1u] = cutouts[d].alphaCutoff; }
    out.compressed = packFormattedStore(textures, textureCount, at, out.textures, out.texels);
    out.formats = at.codes;
    return out;
}

// everything is validated before anything is built
PackedAlphaCutoffs packSceneAlphaCutoffs(const uint32_t* cutoffs, uint32_t drawCount, uint32_t sceneDrawCount, uint32_t sceneTextureCount) {
    const std::string call = "setSceneAlphaCutoffs";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (sceneDrawCount == 0) refuse("no scene set (plrf_set_scene_meshes comes first)");
    if (sceneTextureCount == 0) refuse("no textures set (plrf_set_scene_textures comes first: the alpha of a fragment is its albedo sample)");
    if (drawCount != sceneDrawCount) refuse("cutoff count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(sceneDrawCount) + " of the scene");
    if (!cutoffs) refuse("cutoffs are null");
    PackedAlphaCutoffs out;
    for (uint32_t d = 0; d < drawCount; d++) {
        if (cutoffs[d] > 255u) refuse("cutoff out of range: draw " + std::to_string(d) + " has " + std::to_string(cutoffs[d]) + ", a cutoff code is 0 (opaque) .. 255");
        out.tested = out.tested || cutoffs[d] != plr::prepass::kAlphaCutoffOpaque;
    }
    out.cutoffs.assign(cutoffs, cutoffs + drawCount);
    return out;
}

// normalize(cross(tangent, normal)) in fp64 from the promoted floats (ModelImport.cpp:184), (0, 0, 0) where the length is not a finite number > 0. The build is
// -ffp-contract=off: every operation below is one IEEE operation, in this order
void deriveBitangent(const float t[3], const float n[3], float out[3]) {
    const double tx = t[0], ty = t[1], tz = t[2], nx = n[0], ny = n[1], nz = n[2];
    const double cx = ty * nz - tz * ny, cy = tz * nx - tx * nz, cz = tx * ny - ty * nx;
    const double len = std::sqrt((cx * cx + cy * cy) + cz * cz);
    const bool good = len > 0.0 && std::isfinite(len);
    out[0] = good ? (float)(cx / len) : 0.f; out[1] = good ? (float)(cy / len) : 0.f; out[2] = good ? (float)(cz / len) : 0.f;
}

// everything is validated before anything is built
PackedNormalMaps packSceneNormalMaps(const float* const* meshTangents, const float* const* meshBitangents, uint32_t meshCount, const uint32_t* normalTextures, uint32_t drawCount,
                                     uint32_t decode, const SceneNormalMapContext& scene) {
    namespace pp = plr::prepass;
    const std::string call = "setSceneNormalMaps";
    auto refuse = [&](const std::string& why) { throw FramePipelineRefusal(PLR_ERR_INVALID_ARGUMENT, call + ": " + why); };
    if (scene.drawCount == 0) refuse("no scene set (plrf_set_scene_meshes comes first)");
    if (scene.textureCount == 0) refuse("no textures set (plrf_set_scene_textures comes first: a normal map is one of the scene's textures)");
    if (meshCount != scene.meshCount) refuse("mesh count " + std::to_string(meshCount) + " differs from the mesh count " + std::to_string(scene.meshCount) + " of the scene");
    if (drawCount != scene.drawCount) refuse("draw count " + std::to_string(drawCount) + " differs from the draw count " + std::to_string(scene.drawCount) + " of the scene");
    if (!normalTextures) refuse("normal_textures are null");
    if (decode != pp::kNormalDecodeReference && decode != pp::kNormalDecodeUnit)
        refuse("decode is " + std::to_string(decode) + ", it must be 1 (PLRF_NORMAL_DECODE_REFERENCE) or 2 (PLRF_NORMAL_DECODE_UNIT)");
    for (uint32_t d = 0; d < drawCount; d++)
        if (normalTextures[d] != kNoSceneTexture && normalTextures[d] >= scene.textureCount)
            refuse("normal texture index out of range: draw " + std::to_string(d) + " names texture " + std::to_string(normalTextures[d]) + " of " + std::to_string(scene.textureCount));
    uint64_t vertices = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        const float* tangents = meshTangents ? meshTangents[m] : nullptr;
        const float* bitangents = meshBitangents ? meshBitangents[m] : nullptr;
        if (tangents && !bitangents && !scene.meshHasNormals[m])
            refuse("mesh " + std::to_string(m) + " was given without normals: its bitangents cannot be derived from cross(tangent, normal), give them");
        for (const float* v : {tangents, bitangents})
            if (v)
                for (size_t i = 0; i < (size_t)scene.meshVertexCounts[m] * 3u; i++)
                    if (!std::isfinite(v[i]))
                        refuse(std::string("non-finite ") + (v == tangents ? "tangent" : "bitangent") + ": vertex " + std::to_string(i / 3u) + " of mesh " + std::to_string(m));
        vertices += scene.meshVertexCounts[m];
    }
    PackedNormalMaps out;
    out.tangents.assign((size_t)vertices * 3u, 0.f);
    out.bitangents.assign((size_t)vertices * 3u, 0.f);
    size_t at = 0;
    for (uint32_t m = 0; m < meshCount; m++) {
        const float* tangents = meshTangents ? meshTangents[m] : nullptr;
        const float* bitangents = meshBitangents ? meshBitangents[m] : nullptr;
        const size_t floats = (size_t)scene.meshVertexCounts[m] * 3u;
        if (tangents && floats) std::memcpy(out.tangents.data() + at, tangents, floats * sizeof(float));
        if (bitangents && floats) std::memcpy(out.bitangents.data() + at, bitangents, floats * sizeof(float));
        else if (tangents) // derived; without tangents they stay (0, 0, 0)
            for (size_t v = 0; v < floats; v += 3u) deriveBitangent(tangents + v, scene.normals + at + v, out.bitangents.data() + at + v);
        at += floats;
    }
    out.normalMaterials.assign(normalTextures, normalTextures + drawCount);
    out.decode = decode;
    return out;
}

} // namespace plrhost
