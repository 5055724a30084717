// Stand-alone check of the scene SDF validation and packing (csrc/frontend/scene_sdf_packing.cpp) and of the instance contract's host arithmetic
// (csrc/device/scene_sdf.h) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_sdf_check.cpp
//       plainrenderer_amd/csrc/frontend/scene_sdf_packing.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_sdf_check
//   ./scene_sdf_check
// It packs a scene of three meshes and five draws, compares the local boxes, the instance map and the instance table with what is worked out here, evaluates the
// contract on matrices whose inverse is known exactly, and sends each kind of invalid input through the validation: every refusal must name its cause and none
// may read outside the caller's arrays (the arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/scene_sdf.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

struct Scene {
    std::unique_ptr<float[]> positions; // exactly 3 * vertices floats
    std::unique_ptr<uint32_t[]> vertexCounts, drawMeshes;
    std::unique_ptr<float[]> models;
    uint32_t meshCount = 3, drawCount = 5;
    SceneSdfContext context(uint32_t maxInstances = 8) const {
        SceneSdfContext c;
        c.positions = positions.get(); c.meshVertexCounts = vertexCounts.get(); c.drawMeshes = drawMeshes.get(); c.models = models.get();
        c.meshCount = meshCount; c.drawCount = drawCount; c.maxInstances = maxInstances;
        return c;
    }
};

static Scene makeScene() {
    Scene s;
    // mesh 0: four vertices; mesh 1: none; mesh 2: three vertices
    const float p[21] = {-1.f, 2.f, 0.5f, 3.f, -2.f, 0.25f, 0.f, 0.f, -4.f, 1.f, 1.f, 1.f, 5.f, 5.f, 5.f, 6.f, 4.f, 5.f, 5.5f, 4.5f, 7.f};
    s.positions.reset(new float[21]);
    std::memcpy(s.positions.get(), p, sizeof(p));
    s.vertexCounts.reset(new uint32_t[3]{4, 0, 3});
    s.drawMeshes.reset(new uint32_t[5]{2, 0, 1, 0, 2});
    s.models.reset(new float[80]);
    for (int d = 0; d < 5; d++)
        for (int e = 0; e < 16; e++) s.models[d * 16 + e] = e % 5 == 0 ? 1.f + (float)d : e >= 12 && e < 15 ? (float)(d - e) : 0.f;
    return s;
}

static std::string refusal(const std::vector<uint32_t>& sdf, const SceneSdfContext& c, int* code) {
    try {
        packSceneSdf(sdf.empty() ? nullptr : sdf.data(), (uint32_t)sdf.size(), c);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

int main() {
    namespace ss = plr::scenesdf;
    const Scene scene = makeScene();
    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };

    // ---- packing: mesh 0 from volume 7, mesh 1 without an SDF, mesh 2 baked
    const std::vector<uint32_t> sdf = {7u, kNoSceneTexture, kSceneSdfBake};
    const PackedSceneSdf p = packSceneSdf(sdf.data(), 3, scene.context());
    CHECK(p.meshSdf == sdf && p.bakedMeshes == std::vector<uint32_t>({2u}));
    CHECK(p.instanceDraws == std::vector<uint32_t>({0u, 1u, 3u, 4u})); // draw 2 has mesh 1
    const float box0[6] = {-1.f, -2.f, -4.f, 3.f, 2.f, 1.f}, box2[6] = {5.f, 4.f, 5.f, 6.f, 5.f, 7.f};
    CHECK(p.meshBoxes.size() == 18 && std::memcmp(p.meshBoxes.data(), box0, 24) == 0 && std::memcmp(p.meshBoxes.data() + 12, box2, 24) == 0);
    for (int k = 6; k < 12; k++) CHECK(p.meshBoxes[k] == 0.f);
    const uint32_t textureIndices[3] = {7u, kNoSceneTexture, 41u};
    const std::vector<uint32_t> table = sceneSdfInstanceTable(p, scene.drawMeshes.get(), textureIndices);
    CHECK(table.size() == 32);
    ss::InstanceEntry e[4];
    std::memcpy(e, table.data(), sizeof(e));
    CHECK(e[0].draw == 0 && e[0].sdfTextureIndex == 41 && std::memcmp(e[0].localMin, box2, 12) == 0 && std::memcmp(e[0].localMax, box2 + 3, 12) == 0);
    CHECK(e[1].draw == 1 && e[1].sdfTextureIndex == 7 && std::memcmp(e[1].localMin, box0, 12) == 0 && e[2].draw == 3 && e[3].draw == 4 && e[3].sdfTextureIndex == 41);
    // no mesh with an SDF: no instance, and nothing else is refused
    CHECK(packSceneSdf(std::vector<uint32_t>(3, kNoSceneTexture).data(), 3, scene.context()).instanceDraws.empty());

    // ---- the contract's arithmetic where the result is known exactly
    {
        ss::Box cube{{-1.f, -1.f, -1.f}, {1.f, 1.f, 1.f}}, slab{{-4.5f, -0.5f, -1.5f}, {4.5f, 0.5f, 1.5f}};
        const ss::Box pc = ss::paddedBox(cube), ps = ss::paddedBox(slab);
        CHECK(pc.mn[0] == -1.5f && pc.mx[2] == 1.5f && ps.mn[0] == -4.5f - 0.075f * 9.f && ps.mn[1] == -1.f && ps.mx[2] == 2.f);
        float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const ss::Box w = ss::paddedBox(ss::worldBoxOf(identity, slab));
        CHECK(std::memcmp(&w, &ps, sizeof(w)) == 0);
        // scale (2, 0.5, 4), translation (3, -4, 8): the inverse is scale (0.5, 2, 0.25), translation (-1.5, 8, -2)
        const float m[16] = {2, 0, 0, 0, 0, 0.5f, 0, 0, 0, 0, 4, 0, 3, -4, 8, 1};
        float inv[16];
        ss::inverseOf(m, inv);
        const float want[16] = {0.5f, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0.25f, 0, -1.5f, 8, -2, 1};
        for (int k = 0; k < 16; k++) CHECK(inv[k] == want[k]);
        CHECK(ss::determinantOf(ss::subDeterminantsOf(m)) == 4.0);
        float l2w[16];
        ss::localToWorldOf(m, ss::Box{{0.f, 2.f, -1.f}, {2.f, 4.f, 1.f}}, l2w); // bbOffset (1, 3, 0)
        CHECK(l2w[12] == 5.f && l2w[13] == -2.5f && l2w[14] == 8.f && l2w[15] == 1.f && l2w[0] == 2.f);
        // x scaled by 2^-100 and moved by 2^100: the determinant is finite, the inverse's translation is beyond fp32
        const float tiny = std::ldexp(1.f, -100), far = std::ldexp(1.f, 100);
        const float o[16] = {tiny, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, far, 0, 0, 1};
        CHECK(sceneSdfDeterminant(o, box0) == std::ldexp(1.0, -100));
        ss::localToWorldOf(o, ss::paddedBox(cube), l2w);
        ss::inverseOf(l2w, inv);
        bool anyInf = false, anyNan = false;
        for (int k = 0; k < 16; k++) { anyInf |= std::isinf(inv[k]); anyNan |= std::isnan(inv[k]); }
        CHECK(anyInf && !anyNan);
        float albedo[3];
        ss::meanOfWord(0xff804020u, albedo);
        CHECK(albedo[0] == (32.f / 255.f) / 1.f && albedo[1] == (64.f / 255.f) / 1.f && albedo[2] == (128.f / 255.f) / 1.f);
        ss::meanOfWord(0x00ffffffu, albedo);
        CHECK(albedo[0] == 0.f && albedo[2] == 0.f);
        CHECK(ss::meanScratchBytes(1) == 48 && ss::meanScratchBytes(4) == 144);
    }

    // ---- refusals
    Scene none = makeScene();
    none.drawCount = 0;
    why = refusal(sdf, none.context(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene set"));
    why = refusal({7u, kNoSceneTexture}, scene.context(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 2") && has("mesh count 3"));
    why = refusal({}, scene.context(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 0"));
    try { packSceneSdf(nullptr, 3, scene.context()); code = 0; } catch (const FramePipelineRefusal& e2) { code = e2.code; why = e2.what(); }
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
    why = refusal({7u, 9u, kSceneSdfBake}, scene.context(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh 1") && has("no vertex"));
    why = refusal(sdf, scene.context(3), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many SDF instances") && has("4 draws") && has("is 3"));
    why = refusal(sdf, scene.context(4), &code);
    CHECK(code == 0);
    for (float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        Scene bad = makeScene();
        bad.positions[3 * 5 + 1] = v; // vertex 1 of mesh 2
        why = refusal(sdf, bad.context(), &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite position") && has("vertex 1 of mesh 2"));
        why = refusal({7u, kNoSceneTexture, kNoSceneTexture}, bad.context(), &code); // the mesh has no SDF: its positions are not looked at
        CHECK(code == 0);
    }
    {
        Scene flat = makeScene();
        flat.models[3 * 16 + 5] = 0.f; // draw 3: a zero scale in y
        why = refusal(sdf, flat.context(), &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("singular model matrix") && has("draw 3") && has("zero"));
        flat = makeScene();
        flat.models[2 * 16 + 5] = 0.f; // draw 2 is no instance: its matrix is not tested
        why = refusal(sdf, flat.context(), &code);
        CHECK(code == 0);
        flat = makeScene();
        for (int k : {0, 5, 10}) flat.models[16 + k] = 3e38f; // draw 1: the fp64 determinant is finite, the fourth column's fp32 products are not
        flat.models[16 + 12] = -3e38f;
        why = refusal(sdf, flat.context(), &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("singular model matrix") && has("draw 1") && has("not finite"));
        // the same test on new transforms
        std::unique_ptr<float[]> moved(new float[80]);
        std::memcpy(moved.get(), scene.models.get(), 320);
        try { refuseSingularSceneSdfMatrices(moved.get(), 5, p, scene.drawMeshes.get(), "setSceneMeshTransforms"); code = 0; } catch (const FramePipelineRefusal& e2) { code = e2.code; }
        CHECK(code == 0);
        for (int k = 0; k < 4; k++) moved[4 * 16 + 4 + k] = moved[4 * 16 + k]; // draw 4: two equal columns
        try { refuseSingularSceneSdfMatrices(moved.get(), 5, p, scene.drawMeshes.get(), "setSceneMeshTransforms"); code = 0; } catch (const FramePipelineRefusal& e2) { code = e2.code; why = e2.what(); }
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("setSceneMeshTransforms") && has("draw 4") && has("instance 3"));
    }
    // ---- the overrides
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::unique_ptr<float[]> v(new float[15]{0.5f, 0.25f, 1.f, nan, nan, std::numeric_limits<float>::infinity(), 0.f, 0.f, 0.f, nan, 1.f, 2.f, 1.f, 1.f, 1.f});
        const std::vector<float> packed = packSceneSdfMeanAlbedo(v.get(), 5, 5, true);
        CHECK(packed.size() == 15 && std::memcmp(packed.data(), v.get(), 60) == 0);
        auto refused = [&](const float* values, uint32_t count, uint32_t sceneCount, bool set) {
            try { packSceneSdfMeanAlbedo(values, count, sceneCount, set); code = 0; why.clear(); } catch (const FramePipelineRefusal& e2) { code = e2.code; why = e2.what(); }
        };
        refused(v.get(), 5, 5, false);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene SDF"));
        refused(v.get(), 4, 5, true);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 4") && has("draw count 5"));
        refused(nullptr, 5, 5, true);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
        v[7] = std::numeric_limits<float>::infinity();
        refused(v.get(), 5, 5, true);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite mean albedo") && has("component 1 of draw 2"));
    }
    std::printf(g_failures ? "scene_sdf_check: %d check(s) failed\n" : "scene_sdf_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
