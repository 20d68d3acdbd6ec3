// Per-vertex / per-pixel arithmetic of the triangle rasteriser (turntable normal maps of the extracted meshes; reference
// render_mesh.py: an orthographic GL camera, colour 0.5 * normal + 0.5 per vertex, white background, depth-tested, not culled).
//
// Like mesh_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels (k_raster.hip) and compiled by g++ for the
// serial rasteriser at the end of this file, which the CPU tests check against numpy and the GPU tests compare the kernels with,
// bit for bit.  -ffp-contract=off: a fused multiply-add only where this file says fmaf.  Definitions (tests/test_raster_host.py
// relies on them):
//   * vertex stage, per vertex v and view M (3x4, row-major, model -> view; view space: x right, y up, z towards the viewer):
//       p_r = fma(M[r][2], v.z, fma(M[r][1], v.y, fma(M[r][0], v.x, M[r][3])))
//       x_pix = (p.x / (2 hx) + 0.5) * W;   y_pix = 0.5 * H - p.y * (W / (2 hx))     (square pixels, row 0 at the top; every
//       operation one fp32 rounding);   X = (int)rintf(256 * x_pix), Y likewise (1/256 pixel, ties to even);   depth z = p.z, the
//       larger the nearer.  A vertex with a non-finite p, or |X| or |Y| >= 2^28, is invalid; a triangle with an invalid vertex
//       or an index outside [0, V) draws nothing.
//   * coverage, exact in int64: the centre of pixel (r, c) is P = (256 c + 128, 256 r + 128);
//       area2 = (Bx-Ax)(Cy-Ay) - (By-Ay)(Cx-Ax); 0: nothing is drawn; < 0: B and C change places, with their depths and attributes
//       (both windings are drawn); for every directed edge U -> V of the oriented triangle E = (Vx-Ux)(Py-Uy) - (Vy-Uy)(Px-Ux);
//       covered iff every edge has E > 0, or E == 0 and (dy > 0, or dy == 0 and dx < 0) with (dx, dy) = V - U: a pixel centre on
//       an edge shared by two triangles belongs to exactly one of them.
//   * interpolation at a covered pixel: w0 = E_BC, w1 = E_CA, w2 = E_AB; b1 = (float)w1 / (float)area2, b2 = (float)w2 /
//       (float)area2, b0 = (1 - b1) - b2; a value a is fma(b2, aC, fma(b1, aB, b0 * aA)) -- the depth and every channel.
//   * visibility: the largest depth wins, at equal depth bits (-0 read as +0) the lowest triangle index; a pixel whose
//       interpolated depth is a NaN is not drawn.  As one number: key = (ordered image of the depth bits) << 32 | ~triangle
//       index, the unsigned maximum over the triangles that cover the pixel; no triangle: 0.  Nothing else enters the result.
//   * colour: COLOR -- attr [V,3] interpolated as it is; NORMAL -- per vertex n' = (M3x3 n) / |M3x3 n| (rows
//       fma(M[r][2], n.z, fma(M[r][1], n.y, M[r][0] * n.x)), |.| = norm3_torch, 0 where the length is 0 or not finite), the
//       colour fma(0.5, n', 0.5) is interpolated; FLAT -- per triangle the unit normal of cross(pB - pA, pC - pA) of the view-
//       space corners in the ORIGINAL winding (separately rounded differences and products, the same normalisation), fma(0.5, n,
//       0.5), the same at every pixel of the triangle (not interpolated).  Background: background[3], depth -inf, triangle -1.
#pragma once
#include "sample_math.hpp"

namespace danbo {

constexpr int RASTER_MAX_DIM = 4096;             // height, width: 1 .. 4096
constexpr int RASTER_SUB_BITS = 8;               // vertices snap to 1/256 pixel
constexpr int RASTER_COORD_LIMIT = 1 << 28;      // |X|, |Y| below this: every product of two differences fits an int64 with room
constexpr int RASTER_LANE_BOX = 64;              // a clipped bounding box of up to 64 pixel centres is walked by one lane
constexpr int RASTER_MODE_COLOR = 0, RASTER_MODE_NORMAL = 1, RASTER_MODE_FLAT = 2;      // = DANBO_RASTER_* of danbo_raster.h

// one vertex after the vertex stage (16 bytes: one load)
struct RasterVertex {
    int X, Y;        // 1/256 pixel
    float z;         // view-space depth
    int valid;
};

DANBO_HD bool raster_finite(float x) { return x - x == 0.f; }

DANBO_HD float raster_affine_row(const float* r, const float* v) { return fmaf(r[2], v[2], fmaf(r[1], v[1], fmaf(r[0], v[0], r[3]))); }
DANBO_HD float raster_rotate_row(const float* r, const float* n) { return fmaf(r[2], n[2], fmaf(r[1], n[1], mul_rn(r[0], n[0]))); }

// view-space position of a vertex
DANBO_HD void raster_view_point(const float* M, const float* v, float* p) {
    p[0] = raster_affine_row(M, v); p[1] = raster_affine_row(M + 4, v); p[2] = raster_affine_row(M + 8, v);
}

DANBO_HD RasterVertex raster_vertex(const float* p, float hx, int H, int W) {
    const float two_hx = mul_rn(2.f, hx);
    const float x_pix = mul_rn(add_rn(div_rn(p[0], two_hx), 0.5f), (float)W);
    const float y_pix = sub_rn(mul_rn(0.5f, (float)H), mul_rn(p[1], div_rn((float)W, two_hx)));
    const float fx = rintf(mul_rn(256.f, x_pix)), fy = rintf(mul_rn(256.f, y_pix));
    RasterVertex o;
    o.valid = raster_finite(p[0]) && raster_finite(p[1]) && raster_finite(p[2]) && fabsf(fx) < (float)RASTER_COORD_LIMIT &&
              fabsf(fy) < (float)RASTER_COORD_LIMIT;       // (a NaN fails the comparison)
    o.X = o.valid ? (int)fx : 0;
    o.Y = o.valid ? (int)fy : 0;
    o.z = p[2];
    return o;
}

// v / |v|, 0 where the length is 0 or not finite
DANBO_HD void raster_unit(const float* v, float* n) {
    const float len = norm3_torch(v[0], v[1], v[2]);
    const bool ok = raster_finite(len) && len > 0.f;
    n[0] = ok ? div_rn(v[0], len) : 0.f; n[1] = ok ? div_rn(v[1], len) : 0.f; n[2] = ok ? div_rn(v[2], len) : 0.f;
}

DANBO_HD void raster_normal_color(const float* n, float* col) {
    col[0] = fmaf(0.5f, n[0], 0.5f); col[1] = fmaf(0.5f, n[1], 0.5f); col[2] = fmaf(0.5f, n[2], 0.5f);
}

// what the vertex stage keeps beside the RasterVertex, float[3]: COLOR the attribute, NORMAL the colour of the rotated normal,
// FLAT the view-space position (the triangle's normal is made of it)
DANBO_HD void raster_vertex_color(int mode, const float* M, const float* attr_v, const float* p, float* col) {
    if (mode == RASTER_MODE_COLOR) { col[0] = attr_v[0]; col[1] = attr_v[1]; col[2] = attr_v[2]; return; }
    if (mode == RASTER_MODE_FLAT) { col[0] = p[0]; col[1] = p[1]; col[2] = p[2]; return; }
    const float r[3] = {raster_rotate_row(M, attr_v), raster_rotate_row(M + 4, attr_v), raster_rotate_row(M + 8, attr_v)};
    float n[3];
    raster_unit(r, n);
    raster_normal_color(n, col);
}

// FLAT: the colour of the triangle with the view-space corners pa, pb, pc (original winding)
DANBO_HD void raster_flat_color(const float* pa, const float* pb, const float* pc, float* col) {
    const float u[3] = {sub_rn(pb[0], pa[0]), sub_rn(pb[1], pa[1]), sub_rn(pb[2], pa[2])};
    const float v[3] = {sub_rn(pc[0], pa[0]), sub_rn(pc[1], pa[1]), sub_rn(pc[2], pa[2])};
    const float c[3] = {sub_rn(mul_rn(u[1], v[2]), mul_rn(u[2], v[1])), sub_rn(mul_rn(u[2], v[0]), mul_rn(u[0], v[2])),
                        sub_rn(mul_rn(u[0], v[1]), mul_rn(u[1], v[0]))};
    float n[3];
    raster_unit(c, n);
    raster_normal_color(n, col);
}

// ---- coverage ----
// the oriented triangle (area2 > 0) and the pixel centres its bounding box holds inside the image: columns x0 .. x0 + nx - 1,
// rows y0 .. y0 + ny - 1
struct RasterTri {
    int ax, ay, bx, by, cx, cy;
    float za, zb, zc;
    int64_t area2;
    int x0, y0, nx, ny;
    int swapped;         // B and C changed places
};

DANBO_HD int64_t raster_edge(int ux, int uy, int vx, int vy, int px, int py) {
    return (int64_t)(vx - ux) * (int64_t)(py - uy) - (int64_t)(vy - uy) * (int64_t)(px - ux);
}
DANBO_HD bool raster_edge_owns(int64_t E, int dx, int dy) { return E > 0 || (E == 0 && (dy > 0 || (dy == 0 && dx < 0))); }
DANBO_HD int raster_min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
DANBO_HD int raster_max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// false: the triangle draws nothing (an invalid corner, no area, no pixel centre of the image in its bounding box)
DANBO_HD bool raster_tri_setup(const RasterVertex& A, const RasterVertex& B, const RasterVertex& C, int H, int W, RasterTri* t) {
    if (!(A.valid && B.valid && C.valid)) return false;
    const int64_t area2 = raster_edge(A.X, A.Y, B.X, B.Y, C.X, C.Y);
    if (area2 == 0) return false;
    const bool sw = area2 < 0;
    t->ax = A.X; t->ay = A.Y; t->za = A.z;
    t->bx = sw ? C.X : B.X; t->by = sw ? C.Y : B.Y; t->zb = sw ? C.z : B.z;
    t->cx = sw ? B.X : C.X; t->cy = sw ? B.Y : C.Y; t->zc = sw ? B.z : C.z;
    t->area2 = sw ? -area2 : area2;
    t->swapped = sw ? 1 : 0;
    // centre 256 c + 128 in [min, max]: c from ceil((min - 128) / 256) to floor((max - 128) / 256) (arithmetic shifts)
    int x0 = (raster_min3(A.X, B.X, C.X) + 127) >> RASTER_SUB_BITS, x1 = (raster_max3(A.X, B.X, C.X) - 128) >> RASTER_SUB_BITS;
    int y0 = (raster_min3(A.Y, B.Y, C.Y) + 127) >> RASTER_SUB_BITS, y1 = (raster_max3(A.Y, B.Y, C.Y) - 128) >> RASTER_SUB_BITS;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > W - 1) x1 = W - 1;
    if (y1 > H - 1) y1 = H - 1;
    t->x0 = x0; t->y0 = y0; t->nx = x1 - x0 + 1; t->ny = y1 - y0 + 1;
    return t->nx > 0 && t->ny > 0;
}

// is the centre of pixel (r, c) covered; w = (E_BC, E_CA, E_AB)
DANBO_HD bool raster_covers(const RasterTri& t, int r, int c, int64_t* w) {
    const int px = (c << RASTER_SUB_BITS) + 128, py = (r << RASTER_SUB_BITS) + 128;
    w[0] = raster_edge(t.bx, t.by, t.cx, t.cy, px, py);
    w[1] = raster_edge(t.cx, t.cy, t.ax, t.ay, px, py);
    w[2] = raster_edge(t.ax, t.ay, t.bx, t.by, px, py);
    return raster_edge_owns(w[0], t.cx - t.bx, t.cy - t.by) && raster_edge_owns(w[1], t.ax - t.cx, t.ay - t.cy) &&
           raster_edge_owns(w[2], t.bx - t.ax, t.by - t.ay);
}

DANBO_HD void raster_bary(const int64_t* w, int64_t area2, float* b) {
    const float a = (float)area2;
    b[1] = div_rn((float)w[1], a);
    b[2] = div_rn((float)w[2], a);
    b[0] = sub_rn(sub_rn(1.f, b[1]), b[2]);
}
DANBO_HD float raster_interp(const float* b, float aA, float aB, float aC) { return fmaf(b[2], aC, fmaf(b[1], aB, mul_rn(b[0], aA))); }

// ---- visibility ----
// 0: not drawn (a NaN depth); else larger = wins
DANBO_HD uint64_t raster_key(float depth, int tri) {
    if (depth != depth) return 0;
    if (depth == 0.f) depth = 0.f;       // -0 -> +0
    uint32_t u;
    __builtin_memcpy(&u, &depth, 4);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)~(uint32_t)tri;
}
DANBO_HD int raster_key_tri(uint64_t key) { return (int)~(uint32_t)key; }

// the key of triangle `tri` at pixel (r, c), 0 where it does not cover it
DANBO_HD uint64_t raster_pixel_key(const RasterTri& t, int tri, int r, int c) {
    int64_t w[3];
    if (!raster_covers(t, r, c, w)) return 0;
    float b[3];
    raster_bary(w, t.area2, b);
    return raster_key(raster_interp(b, t.za, t.zb, t.zc), tri);
}

DANBO_HD bool raster_index_ok(int i, int n_verts) { return i >= 0 && i < n_verts; }

// one pixel of the result from its key: colour, depth, triangle (what k_raster_resolve and the serial code both do)
DANBO_HD void raster_resolve_pixel(uint64_t key, int r, int c, const int* tris, const RasterVertex* vrec, const float* vcol, int mode,
                                   int H, int W, const float* background, float* rgb, float* depth, int* tri_id) {
    if (key == 0) {
        if (rgb) { rgb[0] = background[0]; rgb[1] = background[1]; rgb[2] = background[2]; }
        if (depth) *depth = -INFINITY;
        if (tri_id) *tri_id = -1;
        return;
    }
    const int tri = raster_key_tri(key);
    const int ia = tris[3 * (long)tri], ib = tris[3 * (long)tri + 1], ic = tris[3 * (long)tri + 2];
    RasterTri t;
    raster_tri_setup(vrec[ia], vrec[ib], vrec[ic], H, W, &t);
    int64_t w[3];
    raster_covers(t, r, c, w);
    float b[3];
    raster_bary(w, t.area2, b);
    if (tri_id) *tri_id = tri;
    if (depth) {
        const float d = raster_interp(b, t.za, t.zb, t.zc);
        *depth = d == 0.f ? 0.f : d;
    }
    if (!rgb) return;
    if (mode == RASTER_MODE_FLAT) {
        raster_flat_color(vcol + 3 * (long)ia, vcol + 3 * (long)ib, vcol + 3 * (long)ic, rgb);
        return;
    }
    const float* ca = vcol + 3 * (long)ia;
    const float* cb = vcol + 3 * (long)(t.swapped ? ic : ib);
    const float* cc = vcol + 3 * (long)(t.swapped ? ib : ic);
    rgb[0] = raster_interp(b, ca[0], cb[0], cc[0]);
    rgb[1] = raster_interp(b, ca[1], cb[1], cc[1]);
    rgb[2] = raster_interp(b, ca[2], cb[2], cc[2]);
}

// ---- workspace: one 64-bit key per pixel, one RasterVertex and one float[3] per vertex, each at a 256-byte boundary ----
DANBO_HD bool raster_dims_ok(int n_verts, int height, int width) {
    return n_verts >= 0 && height >= 1 && height <= RASTER_MAX_DIM && width >= 1 && width <= RASTER_MAX_DIM;
}
DANBO_HD size_t raster_align256(size_t n) { return (n + 255) & ~(size_t)255; }
DANBO_HD size_t raster_keys_bytes(int height, int width) { return raster_align256((size_t)height * width * 8); }
DANBO_HD size_t raster_vrec_bytes(int n_verts) { return raster_align256((size_t)n_verts * sizeof(RasterVertex)); }
DANBO_HD size_t raster_workspace_size(int n_verts, int height, int width) {
    if (!raster_dims_ok(n_verts, height, width)) return 0;
    return 256 + raster_keys_bytes(height, width) + raster_vrec_bytes(n_verts) + raster_align256((size_t)n_verts * 12);
}
DANBO_HD bool raster_args_ok(const float* verts, int n_verts, const int* tris, int n_tris, const float* attr, int mode,
                             const float* views, int n_views, float hx, int height, int width, const float* background,
                             const void* workspace, const float* rgb, const float* depth, const int* tri_id) {
    return raster_dims_ok(n_verts, height, width) && n_tris >= 0 && n_views >= 1 &&
           (mode == RASTER_MODE_COLOR || mode == RASTER_MODE_NORMAL || mode == RASTER_MODE_FLAT) &&
           (attr || mode == RASTER_MODE_FLAT) && raster_finite(hx) && hx > 0.f && (verts || !n_verts) && (tris || !n_tris) &&
           views && background && workspace && (rgb || depth || tri_id) && (uintptr_t)verts % 4 == 0 && (uintptr_t)tris % 4 == 0 &&
           (uintptr_t)attr % 4 == 0 && (uintptr_t)views % 4 == 0 && (uintptr_t)background % 4 == 0 && (uintptr_t)workspace % 8 == 0 &&
           (uintptr_t)rgb % 4 == 0 && (uintptr_t)depth % 4 == 0 && (uintptr_t)tri_id % 4 == 0;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial rasteriser (host): the same call as danbo_raster_mesh, the same definitions, one triangle and one pixel after the other.
// Returns 0, or -22 for a rejected argument.
inline void raster_vertices_host(const float* verts, int n_verts, const float* attr, int mode, const float* M, float hx, int H, int W,
                                 RasterVertex* vrec, float* vcol) {
    for (int v = 0; v < n_verts; ++v) {
        float p[3];
        raster_view_point(M, verts + 3 * (long)v, p);
        vrec[v] = raster_vertex(p, hx, H, W);
        raster_vertex_color(mode, M, attr ? attr + 3 * (long)v : nullptr, p, vcol + 3 * (long)v);
    }
}

inline int raster_mesh_host(const float* verts, int n_verts, const int* tris, int n_tris, const float* attr, int mode,
                            const float* views, int n_views, float hx, int H, int W, const float* background, void* workspace,
                            float* rgb, float* depth, int* tri_id) {
    if (!raster_args_ok(verts, n_verts, tris, n_tris, attr, mode, views, n_views, hx, H, W, background, workspace, rgb, depth, tri_id))
        return -22;
    char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    uint64_t* keys = reinterpret_cast<uint64_t*>(base);
    RasterVertex* vrec = reinterpret_cast<RasterVertex*>(base + raster_keys_bytes(H, W));
    float* vcol = reinterpret_cast<float*>(base + raster_keys_bytes(H, W) + raster_vrec_bytes(n_verts));
    const long n_pix = (long)H * W;
    for (int view = 0; view < n_views; ++view) {
        raster_vertices_host(verts, n_verts, attr, mode, views + 12 * (long)view, hx, H, W, vrec, vcol);
        for (long i = 0; i < n_pix; ++i) keys[i] = 0;
        for (int tri = 0; tri < n_tris; ++tri) {
            const int ia = tris[3 * (long)tri], ib = tris[3 * (long)tri + 1], ic = tris[3 * (long)tri + 2];
            if (!(raster_index_ok(ia, n_verts) && raster_index_ok(ib, n_verts) && raster_index_ok(ic, n_verts))) continue;
            RasterTri t;
            if (!raster_tri_setup(vrec[ia], vrec[ib], vrec[ic], H, W, &t)) continue;
            for (int r = t.y0; r < t.y0 + t.ny; ++r)
                for (int c = t.x0; c < t.x0 + t.nx; ++c) {
                    const uint64_t key = raster_pixel_key(t, tri, r, c);
                    if (key > keys[(long)r * W + c]) keys[(long)r * W + c] = key;
                }
        }
        for (long i = 0; i < n_pix; ++i) {
            const long o = (long)view * n_pix + i;
            raster_resolve_pixel(keys[i], (int)(i / W), (int)(i % W), tris, vrec, vcol, mode, H, W, background, rgb ? rgb + 3 * o : nullptr,
                                 depth ? depth + o : nullptr, tri_id ? tri_id + o : nullptr);
        }
    }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
