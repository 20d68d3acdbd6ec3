// Per-point / per-cell arithmetic of the isosurface extraction (marching cubes on the density grid; reference run_render.py:1265-1281:
// mcubes.marching_cubes(np.maximum(raw, 0), threshold)).
//
// Like sample_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels (k_mesh.hip) and compiled by g++ for the
// serial extractor at the end of this file, which the CPU tests check against numpy and the GPU tests compare the kernels with,
// bit for bit.  Definitions (tests/test_mesh_extract.py relies on them):
//   * grid sigma[nx][ny][nz], element (i, j, k) at sigma[i * stride_x + j * stride_y + k] (a transposed view is read as it is);
//   * a value is read as s = fmaxf(sigma, floor) (the reference's np.maximum(raw, 0): floor = 0; -inf: none), a NaN as -inf;
//     a point is INSIDE iff s >= iso;
//   * cell (i, j, k) has the corners (i + a, j + b, k + c), corner number a + 2b + 4c, case = mask of inside corners;
//   * one vertex per grid edge whose ends differ in inside-ness, owned by the edge's lower end p and its axis ax: p + t e_ax with
//     t = (iso - s0) / (s1 - s0) in fp32 (IEEE division), clamped to [0, 1], 0.5 if it is not finite; every cell around the edge
//     uses the same index (welded);
//   * order: vertices ascending by (linear index of p) * 3 + ax, triangles ascending by the cell's linear index (both of the
//     LOGICAL index ((i * ny + j) * nz + k), not of the memory offset), inside a cell in the order of mc_table.inc;
//   * triangles are oriented so that the normals point from inside (high density) to outside;
//   * v_out[c] = v_index[c] * scale + offset[c], evaluated as fma(t, scale, fma(p, scale, offset)): two roundings, the first of
//     the lower end alone -- exact for scale = 1 / 2^n and a centring offset -- so that an output centred on 0 carries t with the
//     granularity of the OUTPUT coordinate, not of p + t (scale 1, offset 0: fl(p + t), as before).
// Vertex normals (k_mesh_normals, mesh_normals_host; tests/test_mesh_normals.py relies on them): the normalised negative gradient
// of the floored grid, interpolated along the vertex's edge --
//   * d(a, b) = v(b) - v(a) in fp32 with v = mesh_value, 0 where it is not finite (a NaN read as -inf, floor = -inf);
//   * gradient at a grid point q, per axis a: 0.5f d(q - e_a, q + e_a) inside, d(q, q + e_a) on the low face, d(q - e_a, q) on the
//     high face (every dimension is >= 2: one of them exists);
//   * at the vertex (p, ax, t), per component: g = fma(t, g(p + e_ax) - g(p), g(p));
//   * m = max |g_a|: where m is 0 or a component is not finite the normal is the unit vector along ax from the inside end to the
//     outside end (+e_ax if s0 >= iso, else -e_ax); else h = g / m (IEEE division: grids near the ends of the fp32 range neither
//     overflow nor flush), len = sqrtf((hx hx + hy hy) + hz hz), n = -h / len: from high density to low, as the triangles'
//     orientation.  Every operation is a separately rounded fp32 one but the fma of the interpolation.
#pragma once
#include "sample_math.hpp"

namespace danbo {

constexpr int MESH_MIN_DIM = 2, MESH_MAX_DIM = 1024;
// points per workgroup of the kernels = the unit of the two-level ranks: a point's word holds its ranks inside its chunk
constexpr int MESH_CHUNK = 256;

DANBO_HD float mesh_value(float sigma, float floor) { return sigma != sigma ? -INFINITY : fmaxf(sigma, floor); }
DANBO_HD bool mesh_inside(float s, float iso) { return s >= iso; }

// position of the crossing along an edge with the (floored) end values s0, s1
DANBO_HD float mesh_edge_t(float s0, float s1, float iso) {
    const float t = div_rn(sub_rn(iso, s0), sub_rn(s1, s0));
    if (!(t - t == 0.f)) return 0.5f;       // inf or NaN: an infinite or NaN end
    return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
}

// one output coordinate: (p + t) * scale + offset as (p * scale + offset) + t * scale, each a single-rounded fma -- part of the
// contract like norm3_torch's (t = 0 on the two axes the edge does not run along)
DANBO_HD float mesh_coord(int p, float t, float scale, float offset) {
    return fmaf(t, scale, fmaf((float)p, scale, offset));
}

// ---- vertex normals ----
// the floored value at a grid point, read through the grid's strides
struct MeshReader {
    const float* sigma;
    long sx, sy;
    float floor;
    DANBO_HD float operator()(int i, int j, int k) const { return mesh_value(sigma[i * sx + j * sy + k], floor); }
};

// d(a, b) = v(b) - v(a), 0 where it is not finite
DANBO_HD float mesh_diff(float va, float vb) {
    const float d = sub_rn(vb, va);
    return d - d == 0.f ? d : 0.f;
}

// one component of the gradient at the grid point (i, j, k): along the axis with the unit step (di, dj, dk), the point's index on
// that axis q of n
DANBO_HD float mesh_gradient_axis(const MeshReader& at, int i, int j, int k, int di, int dj, int dk, int q, int n) {
    if (q > 0 && q + 1 < n) return mul_rn(0.5f, mesh_diff(at(i - di, j - dj, k - dk), at(i + di, j + dj, k + dk)));
    if (q + 1 < n) return mesh_diff(at(i, j, k), at(i + di, j + dj, k + dk));
    return mesh_diff(at(i - di, j - dj, k - dk), at(i, j, k));
}

DANBO_HD void mesh_gradient(const MeshReader& at, int nx, int ny, int nz, int i, int j, int k, float* g) {
    g[0] = mesh_gradient_axis(at, i, j, k, 1, 0, 0, i, nx);
    g[1] = mesh_gradient_axis(at, i, j, k, 0, 1, 0, j, ny);
    g[2] = mesh_gradient_axis(at, i, j, k, 0, 0, 1, k, nz);
}

// the normal of the vertex at t on the edge along ax: g0, g1 the gradients at the edge's lower and upper end, inside0 = the lower
// end is inside
DANBO_HD void mesh_normal(const float* g0, const float* g1, float t, int ax, bool inside0, float* n) {
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = fmaf(t, sub_rn(g1[c], g0[c]), g0[c]);
    const float m = fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2]));
    const bool finite = g[0] - g[0] == 0.f && g[1] - g[1] == 0.f && g[2] - g[2] == 0.f;       // (fmaxf drops a NaN)
    if (!finite || !(m > 0.f)) {
        const float e = inside0 ? 1.f : -1.f;
        n[0] = ax == 0 ? e : 0.f; n[1] = ax == 1 ? e : 0.f; n[2] = ax == 2 ? e : 0.f;
        return;
    }
    const float hx = div_rn(g[0], m), hy = div_rn(g[1], m), hz = div_rn(g[2], m);
    const float len = sqrtf(add_rn(add_rn(mul_rn(hx, hx), mul_rn(hy, hy)), mul_rn(hz, hz)));
    n[0] = div_rn(-hx, len); n[1] = div_rn(-hy, len); n[2] = div_rn(-hz, len);
}

// the normal of the vertex owned by the grid point (i, j, k) and the axis ax; g0 = mesh_gradient there (shared by the point's edges)
DANBO_HD void mesh_vertex_normal(const MeshReader& at, int nx, int ny, int nz, int i, int j, int k, int ax, float iso, const float* g0,
                                 float* n) {
    const int i1 = i + (ax == 0), j1 = j + (ax == 1), k1 = k + (ax == 2);
    const float s0 = at(i, j, k);
    float g1[3];
    mesh_gradient(at, nx, ny, nz, i1, j1, k1, g1);
    mesh_normal(g0, g1, mesh_edge_t(s0, at(i1, j1, k1), iso), ax, mesh_inside(s0, iso), n);
}

// ---- the 256-case table (tools/gen_mc_table.py -> mc_table.inc) ----
DANBO_HD int mc_ntri(uint64_t entry) { return (int)(entry & 15u); }
DANBO_HD int mc_edge(uint64_t entry, int n) { return (int)((entry >> (4 + 4 * n)) & 15u); }   // n = 3 * triangle + corner
// cube edge e = 4 * ax + r: runs along ax from the corner whose two other coordinates are (r & 1, r >> 1)
DANBO_HD void mc_edge_owner(int e, int* di, int* dj, int* dk, int* ax) {
    const int a = e >> 2, lo = e & 1, hi = (e >> 1) & 1;
    *ax = a;
    *di = a == 0 ? 0 : lo;
    *dj = a == 1 ? 0 : (a == 0 ? lo : hi);
    *dk = a == 2 ? 0 : hi;
}

// ---- the per-point word of the workspace (4 B per grid point) ----
// bits 0-2: owned crossing edges (bit ax), 3-10: case of the cell whose corner 0 the point is (0 where there is no cell),
// 11-20: vertices owned by earlier points of the chunk (<= 3 * 255), 21-31: triangles of earlier cells of the chunk (<= 5 * 255)
DANBO_HD uint32_t mesh_word(int emask, int cell_case, int vrank, int trank) {
    return (uint32_t)emask | ((uint32_t)cell_case << 3) | ((uint32_t)vrank << 11) | ((uint32_t)trank << 21);
}
DANBO_HD int mesh_word_emask(uint32_t w) { return (int)(w & 7u); }
DANBO_HD int mesh_word_case(uint32_t w) { return (int)((w >> 3) & 255u); }
DANBO_HD int mesh_word_vrank(uint32_t w) { return (int)((w >> 11) & 1023u); }
DANBO_HD int mesh_word_trank(uint32_t w) { return (int)(w >> 21); }
DANBO_HD int mesh_popc3(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1); }

// the same argument checks for the library and the serial extractor
DANBO_HD bool mesh_dims_ok(int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso) {
    return nx >= MESH_MIN_DIM && ny >= MESH_MIN_DIM && nz >= MESH_MIN_DIM && nx <= MESH_MAX_DIM && ny <= MESH_MAX_DIM &&
           nz <= MESH_MAX_DIM && (long)nx * ny * nz < (1L << 31) && stride_x >= 0 && stride_y >= 0 && iso - iso == 0.f &&
           floor < INFINITY;     // (a NaN floor fails the comparison)
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial extractor (host): the same two calls as danbo_mesh_count / danbo_mesh_extract, the same definitions, one point after the
// other.  workspace: one int32 per grid point (vertices owned by earlier points).  Returns 0, or -22 for a rejected argument.
static const uint64_t MC_CASE[256] = {
#include "mc_table.inc"
};

struct MeshGrid {
    const float* sigma;
    int nx, ny, nz;
    long sx, sy;
    float floor, iso;
    float at(int i, int j, int k) const { return mesh_value(sigma[i * sx + j * sy + k], floor); }
    bool in(int i, int j, int k) const { return mesh_inside(at(i, j, k), iso); }
    int emask(int i, int j, int k) const {
        const bool c = in(i, j, k);
        return (i + 1 < nx && in(i + 1, j, k) != c ? 1 : 0) | (j + 1 < ny && in(i, j + 1, k) != c ? 2 : 0) |
               (k + 1 < nz && in(i, j, k + 1) != c ? 4 : 0);
    }
    int cell_case(int i, int j, int k) const {
        int m = 0;
        for (int c = 0; c < 8; ++c) m |= (in(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) ? 1 : 0) << c;
        return m;
    }
};

inline int mesh_count_host(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                           int32_t* workspace, int* counts) {
    if (!sigma || !workspace || !counts || !mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso)) return -22;
    const MeshGrid g{sigma, nx, ny, nz, stride_x, stride_y, floor, iso};
    long V = 0, T = 0, n = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k, ++n) {
                workspace[n] = (int32_t)(V < 0x7fffffffL ? V : 0x7fffffffL);
                V += mesh_popc3(g.emask(i, j, k));
                if (i + 1 < nx && j + 1 < ny && k + 1 < nz) T += mc_ntri(MC_CASE[g.cell_case(i, j, k)]);
            }
    counts[0] = (int)(V < 0x7fffffffL ? V : 0x7fffffffL);
    counts[1] = (int)(T < 0x7fffffffL ? T : 0x7fffffffL);
    return 0;
}

inline int mesh_extract_host(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                             const int32_t* workspace, float scale, float off_x, float off_y, float off_z, float* verts, int cap_v,
                             int* tris, int cap_t) {
    if (!sigma || !workspace || !mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso) || cap_v < 0 || cap_t < 0 ||
        (cap_v && !verts) || (cap_t && !tris) || !(scale - scale == 0.f) || !(off_x - off_x == 0.f) || !(off_y - off_y == 0.f) ||
        !(off_z - off_z == 0.f))
        return -22;
    const MeshGrid g{sigma, nx, ny, nz, stride_x, stride_y, floor, iso};
    long n = 0, T = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k, ++n) {
                const int em = g.emask(i, j, k);
                long v = workspace[n];
                for (int ax = 0; ax < 3; ++ax) {
                    if (!((em >> ax) & 1)) continue;
                    if (v < cap_v) {
                        const float t = mesh_edge_t(g.at(i, j, k), g.at(i + (ax == 0), j + (ax == 1), k + (ax == 2)), iso);
                        verts[3 * v + 0] = mesh_coord(i, ax == 0 ? t : 0.f, scale, off_x);
                        verts[3 * v + 1] = mesh_coord(j, ax == 1 ? t : 0.f, scale, off_y);
                        verts[3 * v + 2] = mesh_coord(k, ax == 2 ? t : 0.f, scale, off_z);
                    }
                    ++v;
                }
                if (!(i + 1 < nx && j + 1 < ny && k + 1 < nz)) continue;
                const uint64_t entry = MC_CASE[g.cell_case(i, j, k)];
                for (int c = 0; c < 3 * mc_ntri(entry); ++c) {
                    int di, dj, dk, ax;
                    mc_edge_owner(mc_edge(entry, c), &di, &dj, &dk, &ax);
                    const long q = n + ((long)di * ny + dj) * nz + dk;
                    const long t = T + c / 3;
                    if (t < cap_t) tris[3 * t + c % 3] = (int)(workspace[q] + mesh_popc3(g.emask(i + di, j + dj, k + dk) & ((1 << ax) - 1)));
                }
                T += mc_ntri(entry);
            }
    return 0;
}

// the normals of the vertices mesh_extract_host writes, float[V][3] in vertex order (the same grid and workspace)
inline int mesh_normals_host(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                             const int32_t* workspace, float* normals, int cap_v) {
    if (!sigma || !workspace || !normals || !mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso) || cap_v < 0) return -22;
    const MeshGrid g{sigma, nx, ny, nz, stride_x, stride_y, floor, iso};
    const MeshReader at{sigma, stride_x, stride_y, floor};
    long n = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k, ++n) {
                const int em = g.emask(i, j, k);
                if (!em) continue;
                float g0[3];
                mesh_gradient(at, nx, ny, nz, i, j, k, g0);
                long v = workspace[n];
                for (int ax = 0; ax < 3; ++ax) {
                    if (!((em >> ax) & 1)) continue;
                    if (v < cap_v) mesh_vertex_normal(at, nx, ny, nz, i, j, k, ax, iso, g0, normals + 3 * v);
                    ++v;
                }
            }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
