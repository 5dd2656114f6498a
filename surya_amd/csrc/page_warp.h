// Flattening of curled PAGES ON THE DEVICE: every page is resampled through its warp mesh into an output of its own size.
//
// The rule is warp_mesh of surya_amd/common/imageops.py, restated per pixel: output pixel (u, v) lies in mesh cell (u / cell, v / cell), its
// displacement is the bilinear form of the cell's four nodes (page_warp_core.h: mesh_source, float64, no contraction), and it samples its page
// at itself plus that displacement. From there on it is warp_quad's words exactly -- the tap body is rec_rectify.h's warp_sample, the ONE
// function all three warp kernels call.
//
// One thread per output pixel, 16 x 16 pixel workgroups, no LDS. `cell` is a multiple of 16, so a tile lies in one cell: the four nodes
// come from a workgroup-uniform address, one 16-byte load each (scalar loads: the nodes sit in scalar registers like rectify_kernel's
// homography). Descriptors travel in the kernel-argument segment, MESH_BATCH pages per launch; the meshes stay in device memory. The
// values of a mesh are NOT checked here (the host's check_mesh does that): tap_base keeps every read inside the page whatever they are.
//
// Measured and not kept: the tile's source patch staged in LDS as one packed dword per pixel, taps read from there. On 16
// pages of 2550 x 3300 it ran 3.05 ms at either stride against 3.28 ms (RGB) and 2.61 ms (RGBX) for this form in the same process: the
// taps' bytes already come from L1, and what the patch saves in byte loads on RGB pages it loses on RGBX pages to the fill and the barrier.
#pragma once
#include "common.h"
#include "page_warp_core.h"
#include "rec_rectify.h"

namespace sa {
namespace prep {

using pagewarp::MeshDesc;
using pagewarp::MESH_TILE;

static_assert(MESH_TILE == RECTIFY_TILE, "the three warp kernels share one tile");

constexpr int MESH_BATCH = 32;        // descriptors per launch: 32 * 40 B + the header stay below the 4 KB of kernel arguments

struct MeshArgs {
    const unsigned char* pages;
    unsigned char* out;          // may lie in the pages' allocation (disjoint range): no restrict anywhere
    const double* meshes;
    int pix, n;
    MeshDesc d[MESH_BATCH];
};

typedef double mesh_f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void warp_mesh_kernel(MeshArgs a) {
#pragma clang fp contract(off)
    const MeshDesc& D = a.d[blockIdx.z];
    const int u0 = (int)blockIdx.x * MESH_TILE, v0 = (int)blockIdx.y * MESH_TILE;
    if (u0 >= D.w || v0 >= D.h) return;                                                                     // workgroup-uniform
    const int i = u0 / D.cell, j = v0 / D.cell;                                                             // the tile's cell: uniform
    const long pitch = pagewarp::mesh_nodes(D.w, D.cell);
    const mesh_f64x2* node = reinterpret_cast<const mesh_f64x2*>(a.meshes + D.mesh_off) + ((long)j * pitch + i);   // mesh_off is even
    const mesh_f64x2 q00 = node[0], q01 = node[1], q10 = node[pitch], q11 = node[pitch + 1];
    const int u = u0 + (threadIdx.x & (MESH_TILE - 1));
    const int v = v0 + (threadIdx.x / MESH_TILE);
    if (u >= D.w || v >= D.h) return;
    const double n00[2] = {q00.x, q00.y}, n01[2] = {q01.x, q01.y}, n10[2] = {q10.x, q10.y}, n11[2] = {q11.x, q11.y};
    double sx, sy;
    pagewarp::mesh_source(u, v, i, j, D.cell, n00, n01, n10, n11, &sx, &sy);
    warp_sample(a.pages + D.page_off, D.w, D.h, a.pix, sx, sy, a.out + D.out_off + ((long)v * D.w + u) * a.pix);
}

// descs: HOST array of n descriptors, validated here (what the device then reads, it reads unchecked); nothing is launched unless
// every descriptor passes
static inline int warp_mesh_run(const unsigned char* pages, const MeshDesc* descs, int n, const double* meshes, unsigned char* out, int pix,
                                int max_w, int max_h, hipStream_t s) {
    if (n < 0 || (pix != 3 && pix != 4)) return SA_ERR_ARG;
    if (!pages || !descs || !meshes || !out || max_w <= 0 || max_h <= 0) return SA_ERR_ARG;
    if (pix == 4 && ((reinterpret_cast<uintptr_t>(pages) | reinterpret_cast<uintptr_t>(out)) & 3)) return SA_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(meshes) & 15) return SA_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!pagewarp::mesh_desc_ok(descs[i], pix, max_w, max_h)) return SA_ERR_ARG;
    const int tw = cdiv(max_w, MESH_TILE), th = cdiv(max_h, MESH_TILE);
    if (th > 65535) return SA_ERR_ARG;                        // grid.y / grid.z limits
    if (n == 0) return SA_OK;
    for (int i0 = 0; i0 < n; i0 += MESH_BATCH) {
        MeshArgs a;
        a.pages = pages; a.out = out; a.meshes = meshes; a.pix = pix; a.n = n - i0 < MESH_BATCH ? n - i0 : MESH_BATCH;
        for (int i = 0; i < MESH_BATCH; ++i) a.d[i] = descs[i0 + (i < a.n ? i : 0)];
        hipLaunchKernelGGL(warp_mesh_kernel, dim3(tw, th, a.n), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // namespace prep
}  // namespace sa
