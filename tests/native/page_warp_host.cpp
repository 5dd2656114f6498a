// Host build of csrc/page_warp_core.h, the half of the page-flattening kernel (csrc/page_warp.h) in front of the taps: page_warp_sources()
// computes where every output pixel of one page reads it, the way the kernel does (the tile's cell, its four nodes, mesh_source), and
// page_warp_desc_ok() is the descriptor validation surya_warp_mesh runs. tests/test_dewarp_cpu.py holds both to the numpy rule
// (surya_amd/common/imageops.py: warp_mesh). No GPU, no HIP call, plain C++.
//
// The file is also a program of its own, meant to run under the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined tests/native/page_warp_host.cpp -o page_warp_host && ./page_warp_host
//
// main() checks that every node a tile reads lies inside its mesh at the extreme sizes, the form at the nodes and along the edges, and the
// refusals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../surya_amd/csrc/page_warp_core.h"

using namespace sa::pagewarp;

extern "C" int page_warp_sources(int w, int h, int cell, const double* mesh, double* sx, double* sy) {
    if (w <= 0 || h <= 0 || !mesh_cell_ok(cell) || !mesh || !sx || !sy) return -1;
    const long pitch = mesh_nodes(w, cell);
    for (int v0 = 0; v0 < h; v0 += MESH_TILE)
        for (int u0 = 0; u0 < w; u0 += MESH_TILE) {
            const int i = u0 / cell, j = v0 / cell;                  // the tile's cell, as the kernel takes it from the workgroup's index
            const double* node = mesh + 2 * ((long)j * pitch + i);
            for (int v = v0; v < v0 + MESH_TILE && v < h; ++v)
                for (int u = u0; u < u0 + MESH_TILE && u < w; ++u)
                    mesh_source(u, v, i, j, cell, node, node + 2, node + 2 * pitch, node + 2 * pitch + 2, &sx[(size_t)v * w + u],
                                &sy[(size_t)v * w + u]);
        }
    return 0;
}

extern "C" int page_warp_desc_ok(const void* desc, int pix, int max_w, int max_h) {
    return mesh_desc_ok(*static_cast<const MeshDesc*>(desc), pix, max_w, max_h) ? 1 : 0;
}

extern "C" int page_warp_desc_bytes() { return (int)sizeof(MeshDesc); }

static int failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

int main() {
    CHECK(sizeof(MeshDesc) == 40 && page_warp_desc_bytes() == 40);
    // cells
    for (int c = -16; c <= 1100; ++c) CHECK(mesh_cell_ok(c) == (c >= 16 && c <= 1024 && c % 16 == 0));
    CHECK(mesh_nodes(1, 16) == 2 && mesh_nodes(16, 16) == 2 && mesh_nodes(17, 16) == 3 && mesh_nodes(2550, 64) == 41 && mesh_nodes(1, 1024) == 2);
    // every node a page's tiles read lies inside its mesh (the sanitizer watches the vector), sizes around the cell multiples
    const int sizes[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 131, 1023, 1024, 1025};
    for (int cell : {16, 32, 64, 1024})
        for (int w : sizes)
            for (int h : {1, 17, 97}) {
                const int gw = mesh_nodes(w, cell), gh = mesh_nodes(h, cell);
                std::vector<double> mesh((size_t)gw * gh * 2);
                for (size_t k = 0; k < mesh.size(); ++k) mesh[k] = (double)(k % 7) - 3.0;
                std::vector<double> sx((size_t)w * h), sy((size_t)w * h);
                CHECK(page_warp_sources(w, h, cell, mesh.data(), sx.data(), sy.data()) == 0);
            }
    // the form: a zero mesh is the identity; a constant mesh a shift; at a cell's corner pixel the form is close to that node
    {
        const int w = 40, h = 20, cell = 16, gw = mesh_nodes(w, cell), gh = mesh_nodes(h, cell);
        std::vector<double> mesh((size_t)gw * gh * 2, 0.0), sx((size_t)w * h), sy((size_t)w * h);
        CHECK(page_warp_sources(w, h, cell, mesh.data(), sx.data(), sy.data()) == 0);
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) CHECK(sx[(size_t)v * w + u] == (double)u && sy[(size_t)v * w + u] == (double)v);
        for (size_t k = 0; k < mesh.size(); k += 2) { mesh[k] = 3.0; mesh[k + 1] = -2.0; }
        CHECK(page_warp_sources(w, h, cell, mesh.data(), sx.data(), sy.data()) == 0);
        for (int v = 0; v < h; ++v)
            for (int u = 0; u < w; ++u) CHECK(sx[(size_t)v * w + u] == (double)u + 3.0 && sy[(size_t)v * w + u] == (double)v - 2.0);
        // dy = 1 on node row 1 only: pixel row v reads at v + (v + 0.5) / 16 above that row and v + (32 - v - 0.5) / 16 below it
        for (size_t k = 0; k < mesh.size(); ++k) mesh[k] = 0.0;
        for (int i = 0; i < gw; ++i) mesh[2 * ((size_t)1 * gw + i) + 1] = 1.0;
        CHECK(page_warp_sources(w, h, cell, mesh.data(), sx.data(), sy.data()) == 0);
        CHECK(sy[0] == 0.5 / 16.0 + 0.0 && sy[(size_t)15 * w + 39] == 15.0 + 15.5 / 16.0 && sy[(size_t)16 * w + 7] == 16.0 + 15.5 / 16.0);
        CHECK(sx[(size_t)15 * w + 39] == 39.0);
    }
    // refusals
    {
        MeshDesc d = {0, 100, 50, 32, 0, 0, 0};
        CHECK(mesh_desc_ok(d, 3, 100, 50) && mesh_desc_ok(d, 4, 100, 50));
        CHECK(!mesh_desc_ok(d, 3, 99, 50) && !mesh_desc_ok(d, 3, 100, 49));
        MeshDesc e = d; e.w = 0; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.h = -1; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.cell = 24; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.cell = 0; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.cell = 1040; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.reserved = 1; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.page_off = -1; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.out_off = -4; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.mesh_off = -2; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.mesh_off = 3; CHECK(!mesh_desc_ok(e, 3, 100, 50));
        e = d; e.page_off = 6; CHECK(mesh_desc_ok(e, 3, 100, 50) && !mesh_desc_ok(e, 4, 100, 50));
        e = d; e.out_off = 2; CHECK(mesh_desc_ok(e, 3, 100, 50) && !mesh_desc_ok(e, 4, 100, 50));
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("page_warp_host: all checks passed\n");
    return 0;
}
