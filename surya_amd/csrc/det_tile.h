// Tiled detection (surya_amd/detection/tiling.py states the grid and the ownership rule): the two copies around the model forward.
//   cut_tiles     P x P windows of uint8 pages (RGB or RGBX, any size) -> the uint8 tile batch surya_det_forward_u8 reads; white (255)
//                 outside the page, fourth byte 0 in an RGBX batch.
//   stitch_tiles  the rectangle a tile OWNS of its fp32 heat planes -> the page map. Every map pixel has one owner, so the map is a pure
//                 gather of the tiles' values: nothing is blended, the order of launches does not matter, and numpy states it bit for bit.
// Both take a DEVICE table of descriptors (one launch serves every tile of a model batch, whatever pages they belong to) and are
// memory-bound: a lane moves 16 bytes where the addresses allow it (four RGBX pixels, four floats) and single elements at the edges.
// A descriptor that names something outside the launch's own buffers (tile index, rectangle outside the tile, pixel stride) is skipped
// whole by every lane that reads it; what it addresses in the CALLER's buffers (page, map) is the caller's to keep in bounds.
#pragma once
#include "common.h"

namespace sa {
namespace tile {

struct CutDesc {             // 32 bytes, C layout (include/surya_amd.h)
    const unsigned char* src;    // page [h][w][pix]
    int w, h, pix;               // pix = 3 (RGB) or 4 (RGBX, fourth byte ignored)
    int x0, y0;                  // window origin in the page (may be negative / hang over the page)
    int tile;                    // destination tile index
};
static_assert(sizeof(CutDesc) == 32, "CutDesc layout is part of the ABI");

struct StitchDesc {          // 64 bytes, C layout (include/surya_amd.h)
    float* dst;                  // plane 0 of the page map
    long long pitch;             // floats per map row
    long long plane_stride;      // floats between the planes of the map
    int tile;                    // index in the heat tensor [tiles][labels][P][P]
    int tx0, ty0, tw, th;        // owned rectangle, tile coordinates
    int dx0, dy0;                // where its first pixel goes in the map
    int planes;                  // planes copied (1 .. labels)
    int pad_cols;                // zeros written behind the rectangle's last column on each of its rows (0 .. 3)
    int reserved;
};
static_assert(sizeof(StitchDesc) == 64, "StitchDesc layout is part of the ABI");

constexpr int SA_TILE_THREADS = 256;

__device__ __forceinline__ uint32_t cut_px(const CutDesc& d, int y, int x) {
    if ((unsigned)y >= (unsigned)d.h || (unsigned)x >= (unsigned)d.w) return 0x00FFFFFFu;
    const unsigned char* p = d.src + ((long)y * d.w + x) * d.pix;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// VEC: P % 4 == 0 and the batch is aligned for the wide store (16 bytes for RGBX, 4 for RGB): a lane makes four pixels of a tile row.
// Otherwise a lane makes one pixel with byte stores. Grid (cdiv(P * P / (VEC ? 4 : 1), 256), n descriptors).
template <bool VEC>
__global__ __launch_bounds__(SA_TILE_THREADS) void cut_tiles_kernel(const CutDesc* __restrict__ descs, unsigned char* __restrict__ dst,
                                                                   int n_tiles, int P, int dpix) {
    const CutDesc d = descs[blockIdx.y];                                                 // block-uniform
    if (!d.src || d.w <= 0 || d.h <= 0 || (d.pix != 3 && d.pix != 4) || d.tile < 0 || d.tile >= n_tiles) return;
    const int per_row = VEC ? P / 4 : P;
    const long i = (long)blockIdx.x * SA_TILE_THREADS + threadIdx.x;
    if (i >= (long)per_row * P) return;
    const int ty = (int)(i / per_row), tx = (int)(i % per_row) * (VEC ? 4 : 1);
    unsigned char* o = dst + (((long)d.tile * P + ty) * P + tx) * dpix;
    const long yl = (long)d.y0 + ty, xl = (long)d.x0 + tx;                              // (origins near INT_MAX must not wrap)
    if (!VEC) {
        const uint32_t v = (yl < 0 || yl >= d.h || xl < 0 || xl >= d.w) ? 0x00FFFFFFu : cut_px(d, (int)yl, (int)xl);
        o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
        if (dpix == 4) o[3] = 0;
        return;
    }
    uint32_t p0, p1, p2, p3;
    if (yl < 0 || yl >= d.h || xl + 3 < 0 || xl >= d.w) {                                // the four pixels lie outside the page
        p0 = p1 = p2 = p3 = 0x00FFFFFFu;
    } else if (xl >= 0 && xl + 3 < d.w) {                                                // ... inside it: 16 / 12 contiguous source bytes
        const unsigned char* s = d.src + (yl * d.w + xl) * d.pix;
        const uintptr_t a = (uintptr_t)s;
        if (d.pix == 4 && (a & 15) == 0) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(s);
            p0 = v[0] & 0xFFFFFFu; p1 = v[1] & 0xFFFFFFu; p2 = v[2] & 0xFFFFFFu; p3 = v[3] & 0xFFFFFFu;
        } else if (d.pix == 4 && (a & 3) == 0) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
            p0 = q[0] & 0xFFFFFFu; p1 = q[1] & 0xFFFFFFu; p2 = q[2] & 0xFFFFFFu; p3 = q[3] & 0xFFFFFFu;
        } else if (d.pix == 3 && (a & 3) == 0) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            p0 = d0 & 0xFFFFFFu; p1 = ((d0 >> 24) | (d1 << 8)) & 0xFFFFFFu; p2 = ((d1 >> 16) | (d2 << 16)) & 0xFFFFFFu; p3 = d2 >> 8;
        } else {
            const int y = (int)yl, x = (int)xl;
            p0 = cut_px(d, y, x); p1 = cut_px(d, y, x + 1); p2 = cut_px(d, y, x + 2); p3 = cut_px(d, y, x + 3);
        }
    } else {                                                                             // ... across the page's left or right edge
        const int y = (int)yl, x = (int)xl;
        p0 = cut_px(d, y, x); p1 = cut_px(d, y, x + 1); p2 = cut_px(d, y, x + 2); p3 = cut_px(d, y, x + 3);
    }
    if (dpix == 4) {
        *reinterpret_cast<u32x4*>(o) = u32x4{p0, p1, p2, p3};
    } else {
        uint32_t* q = reinterpret_cast<uint32_t*>(o);
        q[0] = p0 | (p1 << 24); q[1] = (p1 >> 8) | (p2 << 16); q[2] = (p2 >> 16) | (p3 << 8);
    }
}

static inline int cut_tiles_run(const void* descs, int n, unsigned char* dst, int n_tiles, int P, int dpix, hipStream_t s) {
    if (!descs || !dst || n < 0 || n_tiles <= 0 || P <= 0 || (dpix != 3 && dpix != 4)) return SA_ERR_ARG;
    if (n == 0) return SA_OK;
    if (n > 65535) return SA_ERR_ARG;                                                    // grid.y
    const bool vec = P % 4 == 0 && (uintptr_t)dst % (dpix == 4 ? 16 : 4) == 0;
    const long work = (long)P * (vec ? P / 4 : P);
    const dim3 grid((unsigned)cdivl(work, SA_TILE_THREADS), (unsigned)n);
    if (vec) hipLaunchKernelGGL(cut_tiles_kernel<true>, grid, dim3(SA_TILE_THREADS), 0, s, (const CutDesc*)descs, dst, n_tiles, P, dpix);
    else hipLaunchKernelGGL(cut_tiles_kernel<false>, grid, dim3(SA_TILE_THREADS), 0, s, (const CutDesc*)descs, dst, n_tiles, P, dpix);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// A row of the owned rectangle is tw floats, then pad_cols zeros. Lane 0 of a row takes the floats in front of the destination's first
// 16-byte boundary, lane c >= 1 the c-th group of four behind it: one 16-byte store, fed by one 16-byte load when the source is aligned
// the same way (tx0 - dx0 a multiple of four, as with every grid whose stride P - overlap is one), else by four loads.
// Grid (cdiv(P * (P / 4 + 2), 256), n descriptors, labels).
__global__ __launch_bounds__(SA_TILE_THREADS) void stitch_tiles_kernel(const float* __restrict__ heat, int n_tiles, int labels, int P,
                                                                      const StitchDesc* __restrict__ descs) {
    const StitchDesc d = descs[blockIdx.y];                                              // block-uniform
    const int plane = blockIdx.z;
    if (!d.dst || d.pitch <= 0 || d.tile < 0 || d.tile >= n_tiles || d.planes < 1 || d.planes > labels || plane >= d.planes) return;
    if (d.tx0 < 0 || d.ty0 < 0 || d.tw <= 0 || d.th <= 0 || d.tw > P - d.tx0 || d.th > P - d.ty0) return;
    if (d.dx0 < 0 || d.dy0 < 0 || d.pad_cols < 0 || d.pad_cols > 3) return;
    const int per_row = P / 4 + 2;
    const long i = (long)blockIdx.x * SA_TILE_THREADS + threadIdx.x;
    const int r = (int)(i / per_row), c = (int)(i % per_row);
    if (r >= d.th) return;
    const float* src = heat + (((long)d.tile * labels + plane) * P + d.ty0 + r) * P + d.tx0;
    float* dst = d.dst + plane * d.plane_stride + (long)(d.dy0 + r) * d.pitch + d.dx0;
    const int len = d.tw + d.pad_cols;
    const int lead = min(len, (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2));        // (a float pointer: the low two bits are 0)
    const int e0 = c == 0 ? 0 : lead + 4 * (c - 1), e1 = c == 0 ? lead : min(len, e0 + 4);
    if (e0 >= e1) return;
    if (e1 - e0 == 4 && e1 <= d.tw) {
        f32x4 v;
        if (((uintptr_t)(src + e0) & 15) == 0) v = *reinterpret_cast<const f32x4*>(src + e0);
        else v = f32x4{src[e0], src[e0 + 1], src[e0 + 2], src[e0 + 3]};
        *reinterpret_cast<f32x4*>(dst + e0) = v;
        return;
    }
    for (int e = e0; e < e1; ++e) dst[e] = e < d.tw ? src[e] : 0.f;
}

static inline int stitch_tiles_run(const float* heat, int n_tiles, int labels, int P, const void* descs, int n, hipStream_t s) {
    if (!heat || !descs || n < 0 || n_tiles <= 0 || labels <= 0 || labels > 65535 || P <= 0) return SA_ERR_ARG;
    if (n == 0) return SA_OK;
    if (n > 65535) return SA_ERR_ARG;                                                    // grid.y
    const dim3 grid((unsigned)cdivl((long)P * (P / 4 + 2), SA_TILE_THREADS), (unsigned)n, (unsigned)labels);
    hipLaunchKernelGGL(stitch_tiles_kernel, grid, dim3(SA_TILE_THREADS), 0, s, heat, n_tiles, labels, P, (const StitchDesc*)descs);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

}  // namespace tile
}  // namespace sa
