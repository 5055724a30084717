// Stand-alone check of the scene normal map validation, bitangent derivation and packing (csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU
// and no backend:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_normal_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_normal_check
//   ./scene_normal_check
// It packs tangents, bitangents and normal texture indices for a two-mesh scene, compares every packed float with its source or with the written rule, and sends
// each kind of invalid input through the validation: every refusal must name its cause and none may read outside the caller's arrays (heap blocks of exactly the
// stated size, so the sanitizer sees an overrun).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

// 3 floats per vertex in a heap block of exactly that size
static std::unique_ptr<float[]> vectors(uint32_t vertices, float salt) {
    std::unique_ptr<float[]> b(new float[(size_t)vertices * 3u]);
    for (uint32_t i = 0; i < vertices * 3u; i++) b[i] = std::sin(salt + 0.7f * (float)i) + 0.1f;
    return b;
}

struct Scene {
    std::vector<uint32_t> vertexCounts{5u, 3u};
    std::vector<uint8_t> hasNormals{1, 0};
    std::unique_ptr<float[]> normals = vectors(8, 3.f); // packed: mesh 0's five, then mesh 1's three (zeros in the pipeline: it came without)
    uint32_t drawCount = 3, textureCount = 2;
    SceneNormalMapContext context() const {
        SceneNormalMapContext c;
        c.meshVertexCounts = vertexCounts.data(); c.meshHasNormals = hasNormals.data(); c.normals = normals.get();
        c.meshCount = (uint32_t)vertexCounts.size(); c.drawCount = drawCount; c.textureCount = textureCount;
        return c;
    }
};

static std::string refusal(const float* const* tangents, const float* const* bitangents, uint32_t meshCount, const uint32_t* textures, uint32_t drawCount, uint32_t decode,
                           const SceneNormalMapContext& scene, int* code) {
    try {
        packSceneNormalMaps(tangents, bitangents, meshCount, textures, drawCount, decode, scene);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

int main() {
    namespace pp = plr::prepass;
    static_assert(pp::kNormalDecodeReference == 1u && pp::kNormalDecodeUnit == 2u, "decode codes");
    static_assert(sizeof(pp::NormalPushConstants) == 20 && pp::kTangentBinding == 11 && pp::kBitangentBinding == 12 && pp::kNormalMaterialBinding == 13 && pp::kShadingNormalBinding == 5,
                  "pass record");
    static_assert(sizeof(pp::Material) == 8, "materials keeps its 8-byte stride");
    Scene scene;
    for (int k = 15; k < 24; k++) scene.normals[k] = 0.f;
    const SceneNormalMapContext ctx = scene.context();
    std::unique_ptr<float[]> t0 = vectors(5, 1.f), t1 = vectors(3, 2.f), b0 = vectors(5, 4.f), b1 = vectors(3, 5.f);
    std::unique_ptr<uint32_t[]> tex(new uint32_t[3]{1u, kNoSceneTexture, 0u});
    {   // everything given
        const float* tangents[2] = {t0.get(), t1.get()};
        const float* bitangents[2] = {b0.get(), b1.get()};
        const PackedNormalMaps p = packSceneNormalMaps(tangents, bitangents, 2, tex.get(), 3, pp::kNormalDecodeUnit, ctx);
        CHECK(p.tangents.size() == 24 && p.bitangents.size() == 24 && p.decode == 2u);
        CHECK(std::memcmp(p.tangents.data(), t0.get(), 60) == 0 && std::memcmp(p.tangents.data() + 15, t1.get(), 36) == 0);
        CHECK(std::memcmp(p.bitangents.data(), b0.get(), 60) == 0 && std::memcmp(p.bitangents.data() + 15, b1.get(), 36) == 0);
        CHECK(p.normalMaterials == std::vector<uint32_t>({1u, kNoSceneTexture, 0u}));
    }
    {   // mesh 0's bitangents derived, mesh 1 without tangents: zeros, and no derivation for it
        const float* tangents[2] = {t0.get(), nullptr};
        const PackedNormalMaps p = packSceneNormalMaps(tangents, nullptr, 2, tex.get(), 3, pp::kNormalDecodeReference, ctx);
        CHECK(p.decode == 1u);
        for (int v = 0; v < 5; v++) {
            const double tx = t0[3 * v], ty = t0[3 * v + 1], tz = t0[3 * v + 2], nx = scene.normals[3 * v], ny = scene.normals[3 * v + 1], nz = scene.normals[3 * v + 2];
            const double cx = ty * nz - tz * ny, cy = tz * nx - tx * nz, cz = tx * ny - ty * nx;
            const double len = std::sqrt((cx * cx + cy * cy) + cz * cz);
            CHECK(len > 0.0 && p.bitangents[3 * v] == (float)(cx / len) && p.bitangents[3 * v + 1] == (float)(cy / len) && p.bitangents[3 * v + 2] == (float)(cz / len));
        }
        for (int k = 15; k < 24; k++) CHECK(p.tangents[k] == 0.f && p.bitangents[k] == 0.f);
    }
    {   // the rule's edges: parallel vectors and zeros give (0, 0, 0); the largest floats still normalise
        float out[3];
        const float x[3] = {1.f, 0.f, 0.f}, z[3] = {0.f, 0.f, 1.f}, zero[3] = {0.f, 0.f, 0.f}, x2[3] = {2.f, 0.f, 0.f};
        deriveBitangent(x, z, out);
        CHECK(out[0] == 0.f && out[1] == -1.f && out[2] == 0.f);
        deriveBitangent(x, x2, out);
        CHECK(out[0] == 0.f && out[1] == 0.f && out[2] == 0.f);
        deriveBitangent(zero, z, out);
        CHECK(out[0] == 0.f && out[1] == 0.f && out[2] == 0.f);
        const float huge[3] = {3e38f, 0.f, 0.f}, hugeY[3] = {0.f, 3e38f, 0.f};
        deriveBitangent(huge, hugeY, out); // 9e76 and its square fit fp64: the rule is fp64 so that floats cannot overflow it
        CHECK(out[0] == 0.f && out[1] == 0.f && out[2] == 1.f);
    }
    {   // no tangents at all: everything zero
        const PackedNormalMaps p = packSceneNormalMaps(nullptr, nullptr, 2, tex.get(), 3, pp::kNormalDecodeUnit, ctx);
        CHECK(p.tangents == std::vector<float>(24, 0.f) && p.bitangents == std::vector<float>(24, 0.f));
    }
    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };
    const float* tangents[2] = {t0.get(), t1.get()};
    const float* bitangents[2] = {b0.get(), b1.get()};
    SceneNormalMapContext none = ctx;
    none.drawCount = 0;
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, none, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene set"));
    SceneNormalMapContext untextured = ctx;
    untextured.textureCount = 0;
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, untextured, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no textures set"));
    why = refusal(tangents, bitangents, 1, tex.get(), 3, 1, ctx, &code); // (the counts are refused before anything is read)
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 1") && has("mesh count 2"));
    why = refusal(tangents, bitangents, 2, tex.get(), 2, 1, ctx, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 2") && has("draw count 3"));
    why = refusal(tangents, bitangents, 2, nullptr, 3, 1, ctx, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("normal_textures are null"));
    for (uint32_t bad : {0u, 3u, 0xffffffffu}) {
        why = refusal(tangents, bitangents, 2, tex.get(), 3, bad, ctx, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("decode is") && has(std::to_string(bad).c_str()));
    }
    tex[2] = 2u;
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, ctx, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("normal texture index out of range") && has("draw 2") && has("texture 2 of 2"));
    tex[2] = 0u;
    t1[4] = std::numeric_limits<float>::quiet_NaN();
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, ctx, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite tangent") && has("vertex 1 of mesh 1"));
    t1[4] = 0.5f;
    b0[14] = std::numeric_limits<float>::infinity();
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, ctx, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite bitangent") && has("vertex 4 of mesh 0"));
    b0[14] = 0.5f;
    const float* onlyFirst[2] = {b0.get(), nullptr};
    why = refusal(tangents, onlyFirst, 2, tex.get(), 3, 1, ctx, &code); // mesh 1 came without normals and has tangents but no bitangents
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh 1 was given without normals"));
    why = refusal(tangents, bitangents, 2, tex.get(), 3, 1, ctx, &code);
    CHECK(code == 0);
    std::printf(g_failures ? "scene_normal_check: %d check(s) failed\n" : "scene_normal_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
