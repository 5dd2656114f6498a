// Page flattening through a warp mesh: the descriptor, its validation and the bilinear form, shared by the HIP kernel (page_warp.h) and a
// plain-C++ build (tests/native/page_warp_host.cpp). surya_amd/common/imageops.py states the whole rule (warp_mesh); this is its half in
// front of the taps.
//
//   mesh      float64 [gh + 1][gw + 1][2], gw = ceil(w / cell), gh = ceil(h / cell): entry (j, i) is the displacement (dx, dy) at output
//             point (i * cell, j * cell), grid-line coordinates (pixel i covers [i, i + 1)). An output point reads the page at itself plus
//             the displacement.
//   source    output pixel (u, v): X = u + 0.5, Y = v + 0.5, i = u / cell, j = v / cell, fx = (X - i * cell) / cell, fy likewise; per
//             component top = m[j][i] * (1 - fx) + m[j][i + 1] * fx, bot the same one row down, d = top * (1 - fy) + bot * fy;
//             sx = (X + dx) - 0.5, sy = (Y + dy) - 0.5. float64 in this order, no contraction: every machine gives the same bits.
//   cell      a multiple of 16 in 16 .. 1024, so that a 16 x 16 output tile lies in ONE cell: its four nodes are workgroup-uniform.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SA_WARP_HD __host__ __device__ __forceinline__
#else
#define SA_WARP_HD inline
#endif

namespace sa {
namespace pagewarp {

struct MeshDesc {
    int64_t page_off;            // byte offset of the page's first pixel in `pages`
    int32_t w, h;                // the page's size, and the output's
    int32_t cell, reserved;      // mesh cell size; 0
    int64_t out_off;             // byte offset of the output's first pixel in `out`
    int64_t mesh_off;            // doubles into `meshes`: the page's [gh + 1][gw + 1][2], even (16-byte aligned nodes)
};

static_assert(sizeof(MeshDesc) == 40, "MeshDesc layout is part of the C ABI (include/surya_amd.h, preprocess_gpu.py)");

constexpr int MESH_TILE = 16;             // 16 x 16 output pixels per workgroup
constexpr int MESH_MIN_CELL = 16;
constexpr int MESH_MAX_CELL = 1024;

SA_WARP_HD bool mesh_cell_ok(int cell) { return cell >= MESH_MIN_CELL && cell <= MESH_MAX_CELL && cell % MESH_TILE == 0; }

SA_WARP_HD int mesh_nodes(int len, int cell) { return (len + cell - 1) / cell + 1; }        // nodes along an axis of `len` pixels

// what surya_warp_mesh refuses in one descriptor (pix: 3 or 4, checked by the caller)
SA_WARP_HD bool mesh_desc_ok(const MeshDesc& d, int pix, int max_w, int max_h) {
    if (d.w <= 0 || d.h <= 0 || d.w > max_w || d.h > max_h) return false;
    if (!mesh_cell_ok(d.cell) || d.reserved != 0) return false;
    if (d.page_off < 0 || d.out_off < 0 || d.mesh_off < 0 || (d.mesh_off & 1)) return false;
    if (pix == 4 && ((d.page_off | d.out_off) & 3)) return false;
    return true;
}

// The bilinear form: n00 = m[j][i], n01 = m[j][i + 1], n10 = m[j + 1][i], n11 = m[j + 1][i + 1], each (dx, dy); (i, j) the cell of
// output pixel (u, v). Writes where that pixel reads the page, pixel-index coordinates.
SA_WARP_HD void mesh_source(int u, int v, int i, int j, int cell, const double* n00, const double* n01, const double* n10, const double* n11,
                            double* sx, double* sy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double X = (double)u + 0.5, Y = (double)v + 0.5;
    const double c = (double)cell;
    const double fx = (X - (double)(i * cell)) / c, fy = (Y - (double)(j * cell)) / c;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    double d[2];
    for (int k = 0; k < 2; ++k) {
        const double top = n00[k] * gx + n01[k] * fx;
        const double bot = n10[k] * gx + n11[k] * fx;
        d[k] = top * gy + bot * fy;
    }
    *sx = (X + d[0]) - 0.5;
    *sy = (Y + d[1]) - 0.5;
}

}  // namespace pagewarp
}  // namespace sa
