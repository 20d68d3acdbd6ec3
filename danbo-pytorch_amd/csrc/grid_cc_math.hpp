// Connected components of the inside set of a density grid, and the filter that drops the components a caller does not want (the
// floaters of an extracted mesh) BEFORE marching cubes -- include/danbo_grid_cc.h, k_grid_cc.hip.  The reference has no such step.
//
// Like mesh_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels and compiled by g++ for the serial
// restatement at the end of this file (grid_cc_host / grid_keep_host), which the CPU tests check against scipy.ndimage.label and
// the GPU tests compare the kernels with, bit for bit.  Definitions (tests/test_grid_cc_host.py relies on them):
//   * grid, strides, value and inside-ness are mesh_math.hpp's: element (i, j, k) at sigma[i * stride_x + j * stride_y + k],
//     v = mesh_value(sigma, floor) (a NaN reads as -inf), a point is INSIDE iff mesh_inside(v, iso);
//   * a point's linear index is the LOGICAL one, p = (i * ny + j) * nz + k, whatever the memory layout;
//   * two inside points are connected iff they differ by one step along one axis (6-connectivity); a component is a class of the
//     transitive closure;
//   * label[p] = the smallest linear index of p's component, -1 for a point outside;
//   * sizes[c] = the number of points of the component whose label is c, 0 at every index that is not a label;
//   * stats[4] = {points inside, components, size of the largest component, its label}; the largest is the greatest size, among
//     equal sizes the smallest label; {0, 0, 0, -1} when nothing is inside;
//   * a component is KEPT iff size >= min_points and (keep_largest == 0 or its label is stats[3]);
//   * out[p] = the 32 bits of sigma[p] if p is outside or its component is kept, else `fill`, which must itself be outside
//     (mesh_value(fill, floor) < iso); kept[2] = {components kept, points kept}.
// Two properties follow:
//   * VERTICES SURVIVE UNCHANGED.  The six neighbours of a kept inside point are in its own component or outside; neither is
//     touched.  So both ends of every crossing edge of a kept component keep their values, and every vertex of the filtered mesh
//     that lies on a kept component is, bit for bit, a vertex of the unfiltered mesh.  The same does not hold for a whole cell's
//     triangles (a cell may also hold a corner of a dropped component), and normals are the gradient of the FILTERED grid: they can
//     differ from the unfiltered mesh's where a dropped component came within two grid steps.
//   * THE RESULT IS A FUNCTION OF THE GRID ALONE.  Every output is an integer or a copied word: two calls give the same bits
//     (integer atomics on the device, no float atomics).
#pragma once
#include <stddef.h>
#include "mesh_math.hpp"
#if !defined(__HIPCC__)
#include <string.h>
#include <vector>
#endif

namespace danbo {

// points per workgroup of the kernels, and the bytes at the head of the workspace that hold the counters of the statistics
constexpr int CC_CHUNK = 256;
constexpr size_t CC_HEAD_BYTES = 256;

DANBO_HD bool cc_dims_ok(int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso) {
    return mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso);
}
DANBO_HD bool cc_inside(float sigma, float floor, float iso) { return mesh_inside(mesh_value(sigma, floor), iso); }
// the value written over a dropped component must read as outside
DANBO_HD bool cc_fill_ok(float fill, float floor, float iso) { return mesh_value(fill, floor) < iso; }

// `out` must hold every grid point at an address of its own: the rows of k inside one another either as (x, y, z) or as (y, x, z)
// (a contiguous array, a slice of one, or its x-y transposed view)
DANBO_HD bool cc_out_layout_ok(int nx, int ny, int nz, long sx, long sy) {
    return (sy >= nz && sx >= (long)ny * sy) || (sx >= nz && sy >= (long)nx * sx);
}
// floats from the first to one past the last element of a grid
DANBO_HD long cc_extent(int nx, int ny, int nz, long sx, long sy) { return (long)(nx - 1) * sx + (long)(ny - 1) * sy + nz; }
// out may be sigma itself with sigma's strides (in place); otherwise the two must not share an address
DANBO_HD bool cc_overlap_ok(const void* sigma, long sx, long sy, const void* out, long osx, long osy, int nx, int ny, int nz) {
    if (sigma == out && sx == osx && sy == osy) return true;
    const uintptr_t s0 = (uintptr_t)sigma, s1 = s0 + 4u * (uintptr_t)cc_extent(nx, ny, nz, sx, sy);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4u * (uintptr_t)cc_extent(nx, ny, nz, osx, osy);
    return s1 <= o0 || o1 <= s0;
}

// a point is inside iff its label is one: labels are memory the caller hands back, so a word that is no index reads as outside
// before it is used as one
DANBO_HD bool cc_label_inside(int label, long n_pts) { return label >= 0 && label < n_pts; }

// the keep rule
DANBO_HD bool cc_keep(int size, int label, int keep_largest, int min_points, int largest_label) {
    return size >= min_points && (keep_largest == 0 || label == largest_label);
}

// "greatest size, among equal sizes the smallest label" as ONE unsigned comparison (the device takes the maximum of these keys with
// an integer atomic); 0 = no component
DANBO_HD uint64_t cc_size_key(int size, int label) { return ((uint64_t)(uint32_t)size << 32) | (uint32_t)(0x7fffffff - label); }
DANBO_HD int cc_key_size(uint64_t key) { return (int)(key >> 32); }
DANBO_HD int cc_key_label(uint64_t key) { return key >> 32 ? 0x7fffffff - (int)(uint32_t)key : -1; }

// the word written at a point
DANBO_HD uint32_t cc_out_word(uint32_t sigma_bits, bool inside, bool kept, uint32_t fill_bits) {
    return !inside || kept ? sigma_bits : fill_bits;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial restatement (host): the same two calls as danbo_grid_cc_label / danbo_grid_cc_keep without workspace and stream, the same
// definitions, one point after the other.  Returns 0, or -22 for a rejected argument.
// root of x in a forest with parent[x] <= x; halves the path on its way (still parent[x] <= x)
inline int32_t cc_find_host(int32_t* parent, int32_t x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

inline int grid_cc_host(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                        int32_t* labels, int32_t* sizes, int32_t* stats) {
    if (!sigma || !labels || !stats || !cc_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso)) return -22;
    const long n_pts = (long)nx * ny * nz, step_i = (long)ny * nz, step_j = nz;
    long n = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k, ++n) {
                if (!cc_inside(sigma[i * stride_x + j * stride_y + k], floor, iso)) { labels[n] = -1; continue; }
                labels[n] = (int32_t)n;
                const long back[3] = {k > 0 ? 1 : 0, j > 0 ? step_j : 0, i > 0 ? step_i : 0};
                for (int ax = 0; ax < 3; ++ax) {
                    if (!back[ax] || labels[n - back[ax]] < 0) continue;
                    const int32_t a = cc_find_host(labels, (int32_t)n), b = cc_find_host(labels, (int32_t)(n - back[ax]));
                    if (a != b) labels[a > b ? a : b] = a > b ? b : a;        // the smaller index stays the root
                }
            }
    std::vector<int32_t> own;
    if (!sizes) { own.resize((size_t)n_pts); sizes = own.data(); }
    for (long p = 0; p < n_pts; ++p) sizes[p] = 0;
    long inside = 0;
    for (long p = 0; p < n_pts; ++p) {
        if (labels[p] < 0) continue;
        labels[p] = cc_find_host(labels, (int32_t)p);        // (ascending: the parent of p is flat already)
        ++sizes[labels[p]];
        ++inside;
    }
    uint64_t best = 0;
    int comps = 0;
    for (long p = 0; p < n_pts; ++p) {
        if (sizes[p] == 0) continue;
        ++comps;
        const uint64_t key = cc_size_key(sizes[p], (int)p);
        if (key > best) best = key;
    }
    stats[0] = (int32_t)inside; stats[1] = comps; stats[2] = cc_key_size(best); stats[3] = cc_key_label(best);
    return 0;
}

inline int grid_keep_host(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                          const int32_t* labels, const int32_t* sizes, const int32_t* stats, int keep_largest, int min_points,
                          float fill, float* out, long out_stride_x, long out_stride_y, int32_t* kept) {
    if (!sigma || !labels || !sizes || !stats || !out || !cc_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso) || min_points < 0 ||
        !cc_fill_ok(fill, floor, iso) || !cc_out_layout_ok(nx, ny, nz, out_stride_x, out_stride_y) ||
        !cc_overlap_ok(sigma, stride_x, stride_y, out, out_stride_x, out_stride_y, nx, ny, nz))
        return -22;
    uint32_t fill_bits;
    memcpy(&fill_bits, &fill, 4);
    const int largest = stats[3];
    const long n_pts = (long)nx * ny * nz;
    long n = 0, comps = 0, points = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k, ++n) {
                uint32_t word;
                memcpy(&word, sigma + i * stride_x + j * stride_y + k, 4);
                const int label = labels[n];
                const bool inside = cc_label_inside(label, n_pts), keep = inside && cc_keep(sizes[label], label, keep_largest, min_points, largest);
                word = cc_out_word(word, inside, keep, fill_bits);
                memcpy(out + i * out_stride_x + j * out_stride_y + k, &word, 4);
                points += keep;
                comps += keep && label == n;
            }
    if (kept) { kept[0] = (int32_t)comps; kept[1] = (int32_t)points; }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
