// Stand-alone check of the scene mesh validation and packing (csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_packing_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_packing_check
//   ./scene_packing_check
// It packs scenes with and without normals, with an empty mesh and with shared meshes, compares every packed element with its source, and sends each kind of
// invalid input through the validation: every refusal must name its cause and none may read outside the caller's arrays (the arrays are heap blocks of exactly
// the stated size, so the sanitizer sees an overrun).
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static std::string refusal(const std::vector<SceneMesh>& meshes, const std::vector<SceneDraw>& draws, int* code) {
    try {
        packSceneMeshes(meshes.data(), (uint32_t)meshes.size(), draws.data(), (uint32_t)draws.size());
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
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
    {
        std::unique_ptr<float[]> m(new float[32]);
        for (int i = 0; i < 32; i++) m[i] = (float)i;
        m[31] = std::numeric_limits<float>::quiet_NaN();
        try { refuseNonFiniteMatrices(m.get(), 2, "check"); CHECK(false); } catch (const FramePipelineRefusal& e) { CHECK(std::string(e.what()).find("element 15 of the model matrix of draw 1") != std::string::npos); }
        m[31] = 31.f;
        try { refuseNonFiniteMatrices(m.get(), 2, "check"); } catch (const FramePipelineRefusal&) { CHECK(false); }
    }
    std::printf(g_failures ? "scene_packing_check: %d check(s) failed\n" : "scene_packing_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
