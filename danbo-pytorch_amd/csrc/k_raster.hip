// Triangle rasteriser for the meshes k_mesh.hip extracts, where they lie: in device memory.  Replaces the GL pass of the
// reference's render_mesh.py (orthographic camera, colour 0.5 * normal + 0.5, white background, depth-tested, not culled); the
// definitions -- snapping, coverage, interpolation, visibility -- are those of raster_math.hpp, whose serial rasteriser the tests
// compare these kernels with bit for bit.
//
// Per view, four launches on the stream:
//   k_raster_vertices  one thread per vertex: the snapped position, the depth and the per-vertex colour (FLAT: the view-space
//                      position) into the workspace.
//   k_raster_clear     the visibility buffer, one 64-bit key per pixel, to 0 (a kernel, not a memset node: common.hpp zero_words).
//   k_raster_depth     one lane per triangle.  A triangle whose clipped bounding box holds at most RASTER_LANE_BOX = 64 pixel
//                      centres is walked by its own lane (extracted meshes: 1 - 3 pixels per triangle).  The larger ones of a
//                      wavefront are collected by ballot and walked one after the other by the whole wavefront: the triangle is
//                      broadcast from its lane, the 64 lanes stride over its box -- one screen-filling triangle costs box / 64
//                      steps, not box.  Per covered pixel one no-return 64-bit atomic max on the key, skipped where a plain load
//                      shows a key that already wins (keys only grow: a stale read costs an atomic, never a result).  The maximum
//                      does not depend on the order of arrival: two runs give the same bits.  No float atomics.
//   k_raster_resolve   one thread per pixel: decodes the winner, recomputes its edge functions with the same inline code and
//                      writes rgb / depth / tri_id, whichever were asked for (consecutive lanes, consecutive pixels of a row).
// Workspace: 8 B per pixel + 28 B per vertex (danbo_raster_workspace_bytes).  No allocation, no synchronisation.  gfx950, wave64.
#include "common.hpp"
#include "../../include/danbo_raster.h"
#include "raster_math.hpp"

namespace danbo {

constexpr int RASTER_BLOCK = 256;
// (DANBO_NO_PK_F32 on the kernels with float arithmetic: the compiler paired their fma chains into the packed form of common.hpp's erratum)

struct RasterArgs {
    const float* verts;
    const int* tris;
    const float* attr;
    int n_verts, n_tris, mode, H, W;
    float hx;
    uint64_t* keys;
    RasterVertex* vrec;
    float* vcol;
};

__global__ __launch_bounds__(RASTER_BLOCK) DANBO_NO_PK_F32 void k_raster_vertices(RasterArgs a, const float* __restrict__ view) {
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = view[i];
    const long stride = (long)gridDim.x * RASTER_BLOCK;
    for (long v = (long)blockIdx.x * RASTER_BLOCK + threadIdx.x; v < a.n_verts; v += stride) {
        const float x[3] = {a.verts[3 * v], a.verts[3 * v + 1], a.verts[3 * v + 2]};
        float p[3], col[3], at[3] = {0.f, 0.f, 0.f};
        raster_view_point(M, x, p);
        a.vrec[v] = raster_vertex(p, a.hx, a.H, a.W);
        if (a.mode != RASTER_MODE_FLAT) { at[0] = a.attr[3 * v]; at[1] = a.attr[3 * v + 1]; at[2] = a.attr[3 * v + 2]; }
        raster_vertex_color(a.mode, M, at, p, col);
        a.vcol[3 * v] = col[0]; a.vcol[3 * v + 1] = col[1]; a.vcol[3 * v + 2] = col[2];
    }
}

__global__ __launch_bounds__(RASTER_BLOCK) void k_raster_clear(uint64_t* __restrict__ keys, long n_pix) {
    const long stride = (long)gridDim.x * RASTER_BLOCK;
    for (long i = (long)blockIdx.x * RASTER_BLOCK + threadIdx.x; i < n_pix; i += stride) keys[i] = 0ull;
}

// the key of `tri` at (r, c) into the visibility buffer; (r, c) lies inside the image: raster_tri_setup clipped the box
__device__ __forceinline__ void raster_submit(const RasterTri& t, int tri, int r, int c, int W, uint64_t* __restrict__ keys) {
    const uint64_t key = raster_pixel_key(t, tri, r, c);
    if (key == 0) return;
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(keys) + ((long)r * W + c);
    if (*slot < key) (void)atomicMax(slot, (unsigned long long)key);
}

__device__ __forceinline__ int bcast(int v, int src) { return __shfl(v, src, WAVE); }
__device__ __forceinline__ float bcast(float v, int src) { return __shfl(v, src, WAVE); }

__global__ __launch_bounds__(RASTER_BLOCK) DANBO_NO_PK_F32 void k_raster_depth(RasterArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long stride = (long)gridDim.x * RASTER_BLOCK;
    // `base` is the same in every lane of a wavefront: the whole wavefront stays in the loop for the ballot and the broadcasts
    for (long base = (long)blockIdx.x * RASTER_BLOCK + (threadIdx.x & ~(WAVE - 1)); base < a.n_tris; base += stride) {
        const long tl = base + lane;
        const int tri = (int)tl;
        RasterTri t = {};
        bool live = false;
        if (tl < a.n_tris) {
            const int ia = a.tris[3 * tl], ib = a.tris[3 * tl + 1], ic = a.tris[3 * tl + 2];
            if (raster_index_ok(ia, a.n_verts) && raster_index_ok(ib, a.n_verts) && raster_index_ok(ic, a.n_verts))
                live = raster_tri_setup(a.vrec[ia], a.vrec[ib], a.vrec[ic], a.H, a.W, &t);
        }
        const int box = live ? t.nx * t.ny : 0;        // <= 4096 * 4096
        if (box > 0 && box <= RASTER_LANE_BOX) {
            for (int r = t.y0; r < t.y0 + t.ny; ++r)
                for (int c = t.x0; c < t.x0 + t.nx; ++c) raster_submit(t, tri, r, c, a.W, a.keys);
        }
        uint64_t big = __ballot(box > RASTER_LANE_BOX);
        while (big) {
            const int src = __ffsll((unsigned long long)big) - 1;
            big &= big - 1;
            RasterTri s;
            s.ax = bcast(t.ax, src); s.ay = bcast(t.ay, src); s.bx = bcast(t.bx, src); s.by = bcast(t.by, src);
            s.cx = bcast(t.cx, src); s.cy = bcast(t.cy, src);
            s.za = bcast(t.za, src); s.zb = bcast(t.zb, src); s.zc = bcast(t.zc, src);
            s.x0 = bcast(t.x0, src); s.y0 = bcast(t.y0, src); s.nx = bcast(t.nx, src); s.ny = bcast(t.ny, src);
            s.swapped = 0;
            s.area2 = raster_edge(s.ax, s.ay, s.bx, s.by, s.cx, s.cy);      // (oriented: > 0, the value the owning lane holds)
            const int stri = (int)(base + src), n = s.nx * s.ny;
            for (int i = lane; i < n; i += WAVE) {
                const int dr = i / s.nx;
                raster_submit(s, stri, s.y0 + dr, s.x0 + (i - dr * s.nx), a.W, a.keys);
            }
        }
    }
}

__global__ __launch_bounds__(RASTER_BLOCK) DANBO_NO_PK_F32 void k_raster_resolve(RasterArgs a, const float* __restrict__ background, float* __restrict__ rgb,
                                                                 float* __restrict__ depth, int* __restrict__ tri_id) {
    const float bg[3] = {background[0], background[1], background[2]};
    const long n_pix = (long)a.H * a.W, stride = (long)gridDim.x * RASTER_BLOCK;
    for (long i = (long)blockIdx.x * RASTER_BLOCK + threadIdx.x; i < n_pix; i += stride) {
        const int r = (int)(i / a.W), c = (int)(i - (long)r * a.W);
        raster_resolve_pixel(a.keys[i], r, c, a.tris, a.vrec, a.vcol, a.mode, a.H, a.W, bg, rgb ? rgb + 3 * i : nullptr,
                             depth ? depth + i : nullptr, tri_id ? tri_id + i : nullptr);
    }
}

}  // namespace danbo

using namespace danbo;

extern "C" size_t danbo_raster_workspace_bytes(int n_verts, int height, int width) { return raster_workspace_size(n_verts, height, width); }

extern "C" int danbo_raster_mesh(const float* verts, int n_verts, const int* tris, int n_tris, const float* attr, int attr_mode,
                                 const float* views, int n_views, float half_extent_x, int height, int width, const float* background,
                                 void* workspace, float* rgb, float* depth, int* tri_id, void* stream) {
    DANBO_CHECK_ARG(raster_args_ok(verts, n_verts, tris, n_tris, attr, attr_mode, views, n_views, half_extent_x, height, width, background,
                                   workspace, rgb, depth, tri_id));
    char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    RasterArgs a{verts, tris, attr, n_verts, n_tris, attr_mode, height, width, half_extent_x, reinterpret_cast<uint64_t*>(base),
                 reinterpret_cast<RasterVertex*>(base + raster_keys_bytes(height, width)),
                 reinterpret_cast<float*>(base + raster_keys_bytes(height, width) + raster_vrec_bytes(n_verts))};
    const long n_pix = (long)height * width;
    const hipStream_t st = (hipStream_t)stream;
    const int grid_pix = stream_grid(n_pix, RASTER_BLOCK);
    for (int view = 0; view < n_views; ++view) {
        const long o = (long)view * n_pix;
        if (n_verts > 0)
            hipLaunchKernelGGL(k_raster_vertices, dim3(stream_grid(n_verts, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, st, a, views + 12 * (long)view);
        hipLaunchKernelGGL(k_raster_clear, dim3(grid_pix), dim3(RASTER_BLOCK), 0, st, a.keys, n_pix);
        if (n_verts > 0 && n_tris > 0)
            hipLaunchKernelGGL(k_raster_depth, dim3(stream_grid(n_tris, RASTER_BLOCK)), dim3(RASTER_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_raster_resolve, dim3(grid_pix), dim3(RASTER_BLOCK), 0, st, a, background, rgb ? rgb + 3 * o : nullptr,
                           depth ? depth + o : nullptr, tri_id ? tri_id + o : nullptr);
    }
    DANBO_LAUNCH_RET();
}
