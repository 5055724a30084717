// Stand-alone check of the validation and packing of both rasterised mesh sets, the scene's meshes and the shadow casters (csrc/frontend/scene_packing.cpp), for a
// sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_packing_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_packing_check
//   ./scene_packing_check
// It packs scenes with and without normals, with an empty mesh and with shared meshes, and the same meshes as casters, compares every packed element with its
// source, and sends each kind of invalid input through the validation: every refusal must name its cause - the casters' are compared in full, and an input with
// several defects must report the one that comes first - and none may read outside the caller's arrays (the arrays are heap blocks of exactly the stated size,
// so the sanitizer sees an overrun).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/device/sun_shadow_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

struct OwnedMesh {
    std::unique_ptr<float[]> positions, normals;
    std::unique_ptr<uint32_t[]> indices;
    SceneMesh view;
};

// a strip of `quads` quads: 2 (quads + 1) vertices, 6 quads indices, in heap blocks of exactly that size
static OwnedMesh strip(uint32_t quads, bool withNormals, float offset) {
    OwnedMesh m;
    const uint32_t v = 2 * (quads + 1), n = 6 * quads;
    m.positions.reset(new float[3 * v]);
    if (withNormals) m.normals.reset(new float[3 * v]);
    m.indices.reset(new uint32_t[n ? n : 1]);
    for (uint32_t i = 0; i < v; i++) {
        m.positions[3 * i + 0] = offset + (float)(i / 2); m.positions[3 * i + 1] = (float)(i % 2); m.positions[3 * i + 2] = 0.25f * (float)i;
        if (withNormals) { m.normals[3 * i + 0] = 0.f; m.normals[3 * i + 1] = 0.6f; m.normals[3 * i + 2] = -0.8f; }
    }
    for (uint32_t q = 0; q < quads; q++) {
        const uint32_t a = 2 * q, idx[6] = {a, a + 1, a + 3, a, a + 3, a + 2};
        std::memcpy(m.indices.get() + 6 * q, idx, sizeof(idx));
    }
    m.view = SceneMesh{m.positions.get(), withNormals ? m.normals.get() : nullptr, v, m.indices.get(), n};
    return m;
}

static SceneDraw draw(uint32_t mesh, float tx, uint32_t albedo, uint32_t specular) {
    SceneDraw d;
    d.mesh = mesh; d.albedo = albedo; d.specular = specular;
    d.modelMatrix[0] = d.modelMatrix[5] = d.modelMatrix[10] = d.modelMatrix[15] = 1.f;
    d.modelMatrix[12] = tx;
    return d;
}

static ShadowCasterMesh caster(const SceneMesh& m) { return ShadowCasterMesh{m.positions, m.vertexCount, m.indices, m.indexCount}; }

static ShadowCasterDraw casterDraw(uint32_t mesh, float tx) {
    ShadowCasterDraw d;
    d.mesh = mesh;
    d.modelMatrix[0] = d.modelMatrix[5] = d.modelMatrix[10] = d.modelMatrix[15] = 1.f;
    d.modelMatrix[12] = tx;
    return d;
}

template <class Pack> static std::string refusalOf(Pack&& pack, int* code) {
    try {
        pack();
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}
static std::string refusal(const std::vector<SceneMesh>& meshes, const std::vector<SceneDraw>& draws, int* code) {
    return refusalOf([&] { packSceneMeshes(meshes.data(), (uint32_t)meshes.size(), draws.data(), (uint32_t)draws.size()); }, code);
}
static std::string refusal(const std::vector<ShadowCasterMesh>& meshes, const std::vector<ShadowCasterDraw>& draws, int* code) {
    return refusalOf([&] { packShadowCasters(meshes.data(), (uint32_t)meshes.size(), draws.data(), (uint32_t)draws.size()); }, code);
}

// the shadow casters: the scene's three meshes and the same draws, every refusal by its full text
static void checkCasters(const OwnedMesh& a, const OwnedMesh& b, const OwnedMesh& c) {
    const std::vector<ShadowCasterMesh> meshes = {caster(a.view), caster(b.view), caster(c.view)};
    const std::vector<ShadowCasterDraw> draws = {casterDraw(2, 1.f), casterDraw(0, 2.f), casterDraw(1, 3.f), casterDraw(2, 4.f)};
    const PackedCasters p = packShadowCasters(meshes.data(), 3, draws.data(), 4);
    CHECK(p.triangleCount == 530 && p.meshVertexCounts == (std::vector<uint32_t>{12, 2, 262}));
    CHECK(p.positions.size() == 3u * (12 + 2 + 262) && p.indices.size() == 30u + 0u + 780u && p.draws.size() == 16 && p.models.size() == 64);
    CHECK(std::memcmp(p.positions.data(), a.positions.get(), 36 * 4) == 0 && std::memcmp(p.positions.data() + 36, b.positions.get(), 6 * 4) == 0 &&
          std::memcmp(p.positions.data() + 36 + 6, c.positions.get(), 786 * 4) == 0);
    CHECK(std::memcmp(p.indices.data(), a.indices.get(), 30 * 4) == 0 && std::memcmp(p.indices.data() + 30, c.indices.get(), 780 * 4) == 0);
    static_assert(sizeof(plr::sunraster::Draw) == 16, "a caster draw is 4 words");
    const uint32_t want[16] = {30, 780, 14, 0, 0, 30, 0, 1, 30, 0, 12, 2, 30, 780, 14, 3};
    CHECK(std::memcmp(p.draws.data(), want, sizeof(want)) == 0);
    for (int k = 0; k < 4; k++) CHECK(std::memcmp(p.models.data() + 16 * k, draws[k].modelMatrix, 64) == 0);
    const float* positions[3] = {a.positions.get(), b.positions.get(), c.positions.get()};
    const uint32_t counts[3] = {12, 2, 262}, drawMeshes[4] = {2, 0, 1, 2};
    const std::vector<float> bounds = packDrawBounds(positions, counts, 3, drawMeshes, 4);
    CHECK(p.drawBounds.size() == 24 && std::memcmp(p.drawBounds.data(), bounds.data(), 24 * 4) == 0);
    CHECK(plr::sunraster::scratchBytes(p.triangleCount) == 64u + ((4u * 530u + 15u) & ~15u) + 80u * 530u);

    int code = 0;
    std::string why;
    auto refused = [&](const std::vector<ShadowCasterMesh>& m, const std::vector<ShadowCasterDraw>& d, const char* text) {
        why = refusal(m, d, &code);
        if (code != PLR_ERR_INVALID_ARGUMENT || why != text) { std::printf("FAILED: code %d, \"%s\" instead of \"%s\"\n", code, why.c_str(), text); g_failures++; }
    };
    const std::vector<ShadowCasterDraw> one = {casterDraw(0, 0.f)};
    refused({}, draws, "setShadowCasters: draws without meshes");
    try { packShadowCasters(meshes.data(), 3, nullptr, 4); CHECK(false); } catch (const FramePipelineRefusal& e) { CHECK(std::string(e.what()) == "setShadowCasters: draws without meshes"); }
    {
        ShadowCasterMesh null = caster(a.view);
        null.indices = nullptr;
        refused({meshes[0], null}, one, "setShadowCasters: mesh 1 has null data");
        null = caster(a.view);
        null.positions = nullptr;
        refused({null}, one, "setShadowCasters: mesh 0 has null data");
    }
    OwnedMesh bad = strip(5, false, 0.f);
    {
        ShadowCasterMesh cut = caster(bad.view);
        cut.indexCount = 29;
        refused({cut}, one, "setShadowCasters: mesh 0 has 29 indices, not a triangle list");
    }
    bad.indices[29] = 12; // the vertex count
    refused({meshes[0], caster(bad.view)}, {casterDraw(1, 0.f)}, "setShadowCasters: vertex index out of range: index 29 of mesh 1 is 12, the mesh has 12 vertices");
    refused(meshes, {casterDraw(0, 0.f), casterDraw(3, 0.f)}, "setShadowCasters: mesh index out of range: draw 1 names mesh 3 of 3");
    const char* notAffine1 = "setShadowCasters: the model matrix of draw 1 is not affine (its last row must be exactly (0, 0, 0, 1): the shadow pass does not divide by w)";
    for (int e : {3, 7, 11, 15}) {
        std::vector<ShadowCasterDraw> withBad = draws;
        withBad[1].modelMatrix[e] = 0.5f;
        refused(meshes, withBad, notAffine1);
    }
    refused(meshes, {casterDraw(1, 0.f)}, "setShadowCasters: the draws hold no triangle");
    {
        // 2^32 vertices in all: refused before anything is sized or copied (the meshes' positions are never read: the block is a's)
        ShadowCasterMesh huge = caster(a.view);
        huge.vertexCount = 0x80000000u;
        refused({huge, huge}, one, "setShadowCasters: too many vertices, indices or triangles");
    }
    // which defect is reported when an input has several: the meshes in order, then per draw its mesh index and its matrix
    const char* notAffine0 = "setShadowCasters: the model matrix of draw 0 is not affine (its last row must be exactly (0, 0, 0, 1): the shadow pass does not divide by w)";
    std::vector<ShadowCasterDraw> two = {casterDraw(0, 0.f), casterDraw(9, 0.f)};
    two[0].modelMatrix[11] = 0.01f;
    refused(meshes, two, notAffine0);
    refused({meshes[0], caster(bad.view), meshes[2]}, two, "setShadowCasters: vertex index out of range: index 29 of mesh 1 is 12, the mesh has 12 vertices");
    two[0].mesh = 9;
    refused(meshes, two, "setShadowCasters: mesh index out of range: draw 0 names mesh 9 of 3");
    // the rule on its own, as setShadowCasterTransforms applies it
    try { refuseUnlessAffine(two[0].modelMatrix, 7, "check"); CHECK(false); } catch (const FramePipelineRefusal& e) {
        CHECK(e.code == PLR_ERR_INVALID_ARGUMENT && std::string(e.what()) == "check: the model matrix of draw 7 is not affine (its last row must be exactly (0, 0, 0, 1): the shadow pass does not divide by w)");
    }
    try { refuseUnlessAffine(two[1].modelMatrix, 0, "check"); } catch (const FramePipelineRefusal&) { CHECK(false); }
}

int main() {
    OwnedMesh a = strip(5, true, 0.f), b = strip(0, false, 3.f), c = strip(130, false, -7.f);
    const std::vector<SceneMesh> meshes = {a.view, b.view, c.view};
    const std::vector<SceneDraw> draws = {draw(2, 1.f, 0x11223344u, 0x55667788u), draw(0, 2.f, 1u, 2u), draw(1, 3.f, 3u, 4u), draw(2, 4.f, 5u, 6u)};
    const PackedScene p = packSceneMeshes(meshes.data(), 3, draws.data(), 4);
    CHECK(p.triangleCount == 260 + 10 + 0 + 260);
    CHECK(p.positions.size() == 3u * (12 + 2 + 262) && p.normals.size() == p.positions.size() && p.indices.size() == 30u + 0u + 780u);
    CHECK(p.draws.size() == 24 && p.models.size() == 64);
    // meshes back to back; a mesh without normals packs zeros
    CHECK(std::memcmp(p.positions.data(), a.positions.get(), 36 * 4) == 0 && std::memcmp(p.positions.data() + 36 + 6, c.positions.get(), 786 * 4) == 0);
    CHECK(std::memcmp(p.normals.data(), a.normals.get(), 36 * 4) == 0);
    for (size_t i = 36; i < p.normals.size(); i++) CHECK(p.normals[i] == 0.f);
    CHECK(std::memcmp(p.indices.data() + 30, c.indices.get(), 780 * 4) == 0);
    plr::prepass::Draw d[4];
    std::memcpy(d, p.draws.data(), sizeof(d));
    CHECK(d[0].firstIndex == 30 && d[0].indexCount == 780 && d[0].vertexOffset == 14 && d[0].transformIndex == 0 && d[0].albedo == 0x11223344u && d[0].specular == 0x55667788u);
    CHECK(d[1].firstIndex == 0 && d[1].indexCount == 30 && d[1].vertexOffset == 0 && d[1].transformIndex == 1);
    CHECK(d[2].firstIndex == 30 && d[2].indexCount == 0 && d[2].vertexOffset == 12 && d[2].transformIndex == 2);
    CHECK(d[3].firstIndex == 30 && d[3].vertexOffset == 14 && d[3].transformIndex == 3 && d[3].albedo == 5u);
    for (int k = 0; k < 4; k++) CHECK(std::memcmp(p.models.data() + 16 * k, draws[k].modelMatrix, 64) == 0);
    // every index of a draw, offset, names a packed vertex
    for (int k = 0; k < 4; k++)
        for (uint32_t i = 0; i < d[k].indexCount; i++) CHECK((size_t)p.indices[d[k].firstIndex + i] + d[k].vertexOffset < p.positions.size() / 3);
    CHECK(plr::prepass::scratchBytes(p.triangleCount) == ((((64u + 8u * 530u + 15u) & ~15u) + 24u * 530u + 15u) & ~15u) + 576u * 530u);

    int code = 0;
    std::string why;
    why = refusal(meshes, {draw(3, 0.f, 0, 0)}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("mesh index out of range") != std::string::npos && why.find("draw 0") != std::string::npos);
    {
        OwnedMesh bad = strip(5, false, 0.f);
        bad.indices[29] = 12; // the vertex count
        why = refusal({a.view, bad.view}, {draw(1, 0.f, 0, 0)}, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("vertex index out of range") != std::string::npos && why.find("index 29 of mesh 1") != std::string::npos);
        bad.indices[29] = 11;
        bad.view.indexCount = 29;
        why = refusal({bad.view}, {draw(0, 0.f, 0, 0)}, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("not a triangle list") != std::string::npos);
    }
    for (float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
        std::vector<SceneDraw> withBad = draws;
        withBad[3].modelMatrix[7] = v;
        why = refusal(meshes, withBad, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("non-finite matrix element") != std::string::npos && why.find("element 7") != std::string::npos && why.find("draw 3") != std::string::npos);
    }
    why = refusal(meshes, {draw(1, 0.f, 0, 0)}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("no triangle") != std::string::npos);
    why = refusal({}, draws, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT);
    {
        SceneMesh null = a.view;
        null.positions = nullptr;
        why = refusal({null}, {draw(0, 0.f, 0, 0)}, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why.find("null data") != std::string::npos);
    }
    // which defect is reported when an input has several: the meshes in order, then the mesh index of every draw, then the matrix of every draw
    {
        std::vector<SceneDraw> two = {draw(0, 0.f, 0, 0), draw(9, 0.f, 0, 0)};
        two[0].modelMatrix[5] = std::numeric_limits<float>::quiet_NaN();
        why = refusal(meshes, two, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why == "setSceneMeshes: mesh index out of range: draw 1 names mesh 9 of 3");
        OwnedMesh bad = strip(5, false, 0.f);
        bad.indices[29] = 12;
        why = refusal({a.view, bad.view, c.view}, two, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why == "setSceneMeshes: vertex index out of range: index 29 of mesh 1 is 12, the mesh has 12 vertices");
        two[1].mesh = 2;
        why = refusal(meshes, two, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && why == "setSceneMeshes: non-finite matrix element: element 5 of the model matrix of draw 0");
    }
    {
        std::unique_ptr<float[]> m(new float[32]);
        for (int i = 0; i < 32; i++) m[i] = (float)i;
        m[31] = std::numeric_limits<float>::quiet_NaN();
        try { refuseNonFiniteMatrices(m.get(), 2, "check"); CHECK(false); } catch (const FramePipelineRefusal& e) { CHECK(std::string(e.what()).find("element 15 of the model matrix of draw 1") != std::string::npos); }
        m[31] = 31.f;
        try { refuseNonFiniteMatrices(m.get(), 2, "check"); } catch (const FramePipelineRefusal&) { CHECK(false); }
    }
    checkCasters(a, b, c);
    std::printf(g_failures ? "scene_packing_check: %d check(s) failed\n" : "scene_packing_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
