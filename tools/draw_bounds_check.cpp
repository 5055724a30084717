// Stand-alone check of the per-draw local boxes the host packs for "drawCulling.comp" (packDrawBounds and packSceneMeshes' drawBounds,
// csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/draw_bounds_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o draw_bounds_check
//   ./draw_bounds_check
// It packs meshes whose extreme vertices are the first, the last and one in between, a mesh with a vertex no index names (the box is over ALL vertices), a mesh
// without vertices, a one-vertex mesh and meshes with a NaN and with infinities among their positions, expands them to draws that share meshes, and
// compares every float with a minimum and maximum taken here. The arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/draw_culling.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

struct OwnedPositions {
    std::unique_ptr<float[]> data;
    uint32_t count = 0;
};

static OwnedPositions positions(const std::vector<float>& xyz) {
    OwnedPositions p;
    p.count = (uint32_t)(xyz.size() / 3);
    p.data.reset(new float[xyz.size() ? xyz.size() : 1]);
    if (!xyz.empty()) std::memcpy(p.data.get(), xyz.data(), xyz.size() * sizeof(float));
    return p;
}

static bool sameBits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<OwnedPositions> meshes;
    meshes.push_back(positions({-3.f, 2.f, 5.f, 1.f, -7.f, 0.5f, 0.25f, 9.f, -1.f, 4.f, 0.f, 6.f}));        // 0: extremes spread over the vertices
    meshes.push_back(positions({}));                                                                         // 1: no vertex
    meshes.push_back(positions({1.5f, -2.5f, 3.5f}));                                                        // 2: one vertex: lo == hi
    meshes.push_back(positions({0.f, 0.f, 0.f, 1.f, nan, 2.f, -1.f, 3.f, 4.f}));                             // 3: a NaN on y
    meshes.push_back(positions({0.f, 0.f, 0.f, inf, 1.f, 2.f, -1.f, -inf, 4.f}));                            // 4: infinities
    meshes.push_back(positions({1e-30f, -1e-30f, 16777216.f, -1e-30f, 1e-30f, 16777218.f}));                 // 5: tiny and large values stay exact
    std::vector<const float*> ptrs;
    std::vector<uint32_t> counts;
    for (const OwnedPositions& m : meshes) { ptrs.push_back(m.data.get()); counts.push_back(m.count); }
    const std::vector<uint32_t> drawMeshes = {5, 0, 0, 1, 2, 3, 4, 0};
    const std::vector<float> b = packDrawBounds(ptrs.data(), counts.data(), (uint32_t)ptrs.size(), drawMeshes.data(), (uint32_t)drawMeshes.size());
    CHECK(b.size() == drawMeshes.size() * plr::drawcull::kBoundsFloats);
    for (size_t d = 0; d < drawMeshes.size() && b.size() == drawMeshes.size() * 6u; d++) {
        const OwnedPositions& m = meshes[drawMeshes[d]];
        for (int a = 0; a < 3; a++) {
            float lo = 0.f, hi = 0.f;
            bool anyNan = false;
            for (uint32_t v = 0; v < m.count; v++) {
                const float x = m.data[3 * v + a];
                if (std::isnan(x)) anyNan = true;
                if (v == 0 || x < lo) lo = x;
                if (v == 0 || x > hi) hi = x;
            }
            if (anyNan) CHECK(std::isnan(b[d * 6 + a]) && std::isnan(b[d * 6 + 3 + a]));
            else CHECK(sameBits(b[d * 6 + a], lo) && sameBits(b[d * 6 + 3 + a], hi));
        }
    }
    // spot values: the box is over all vertices, exact
    CHECK(b[6 + 0] == -3.f && b[6 + 1] == -7.f && b[6 + 2] == -1.f && b[6 + 3] == 4.f && b[6 + 4] == 9.f && b[6 + 5] == 6.f);
    CHECK(b[0 + 2] == 16777216.f && b[0 + 5] == 16777218.f && b[0 + 0] == -1e-30f && b[0 + 3] == 1e-30f);
    for (int k = 0; k < 6; k++) CHECK(b[3 * 6 + k] == 0.f); // the mesh without vertices
    CHECK(b[6 * 6 + 3] == inf && b[6 * 6 + 1] == -inf);
    CHECK(std::memcmp(b.data() + 6, b.data() + 12, 24) == 0 && std::memcmp(b.data() + 6, b.data() + 7 * 6, 24) == 0); // draws that share a mesh share its box

    // a draw that names no mesh is refused, and nothing is read for it
    try {
        const std::vector<uint32_t> bad = {0, 6};
        packDrawBounds(ptrs.data(), counts.data(), (uint32_t)ptrs.size(), bad.data(), 2);
        CHECK(false);
    } catch (const FramePipelineRefusal& e) {
        CHECK(e.code == PLR_ERR_INVALID_ARGUMENT && std::string(e.what()).find("draw 1") != std::string::npos);
    }
    CHECK(packDrawBounds(ptrs.data(), counts.data(), (uint32_t)ptrs.size(), nullptr, 0).empty());

    // through packSceneMeshes: one box per draw, of the draw's mesh, whatever the indices name
    {
        std::unique_ptr<uint32_t[]> indices(new uint32_t[3]{0, 1, 2}); // vertex 3 of mesh 0 is named by no index and still counts
        const SceneMesh sm[2] = {SceneMesh{meshes[0].data.get(), nullptr, meshes[0].count, indices.get(), 3}, SceneMesh{meshes[2].data.get(), nullptr, 1, nullptr, 0}};
        SceneDraw draws[3];
        for (int k = 0; k < 3; k++) { draws[k].mesh = k == 1 ? 1u : 0u; draws[k].modelMatrix[0] = draws[k].modelMatrix[5] = draws[k].modelMatrix[10] = draws[k].modelMatrix[15] = 1.f; }
        const PackedScene p = packSceneMeshes(sm, 2, draws, 3);
        CHECK(p.drawBounds.size() == 18);
        if (p.drawBounds.size() == 18) {
            CHECK(p.drawBounds[3] == 4.f && p.drawBounds[5] == 6.f && std::memcmp(p.drawBounds.data(), p.drawBounds.data() + 12, 24) == 0);
            CHECK(p.drawBounds[6] == 1.5f && p.drawBounds[9] == 1.5f && p.drawBounds[7] == -2.5f && p.drawBounds[11] == 3.5f);
        }
    }
    std::printf(g_failures ? "draw_bounds_check: %d check(s) failed\n" : "draw_bounds_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
