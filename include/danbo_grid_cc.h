/*
 * libdanbo_hip.so -- C ABI of the connected components of a density grid's inside set and of the filter that drops the components
 * a caller does not want (the floaters of an extracted mesh), run BEFORE danbo_mesh_count / danbo_mesh_extract so that vertices,
 * faces, normals and colours all see one filtered grid (csrc/k_grid_cc.hip; csrc/grid_cc_math.hpp states every definition once,
 * for the kernels and for the serial restatement grid_cc_host / grid_keep_host that the tests compare the kernels with bit for bit).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_grid_cc.h").
 *
 * Definitions.  The grid, its strides, the value read and inside-ness are those of danbo_mesh_count: element (i, j, k) at
 * sigma[i * stride_x + j * stride_y + k], v = max(sigma, floor) with a NaN read as -inf, a point is INSIDE iff v >= iso.  A point's
 * linear index is the LOGICAL one, p = (i * ny + j) * nz + k, whatever the memory layout.  Two inside points are connected iff they
 * differ by one step along one axis (6-connectivity); a component is a class of the transitive closure.
 *   labels[p]  the smallest linear index of p's component; -1 for a point outside
 *   sizes[c]   the number of points of the component whose label is c; 0 at every index that is not a label
 *   stats[4]   {points inside, components, size of the largest component, its label}: the greatest size, among equal sizes the
 *              smallest label; {0, 0, 0, -1} when nothing is inside
 * A component is KEPT iff size >= min_points and (keep_largest == 0 or its label is stats[3]).  out[p] holds the 32 bits of
 * sigma[p] if p is outside or its component is kept, `fill` otherwise; kept[2] = {components kept, points kept}.
 *
 * Every output is an integer or a copied word and only integer atomics are used: the result is a function of the grid alone, two
 * calls give the same bits.  A kept inside point's six neighbours are in its own component or outside, and neither is touched: every
 * vertex of the filtered grid's isosurface that lies on a kept component is, bit for bit, a vertex of the unfiltered one (not so a
 * whole cell's triangles, where a cell also holds a corner of a dropped component; and normals are the gradient of the filtered grid).
 */
#ifndef DANBO_GRID_CC_H
#define DANBO_GRID_CC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace danbo_grid_cc_label needs for an nx x ny x nz grid; 0 for an unsupported grid (the limits of
 * danbo_mesh_workspace_bytes: every dimension 2 .. 1024, fewer than 2^31 points). */
size_t danbo_grid_cc_workspace_bytes(int nx, int ny, int nz);

/* Labels, sizes and statistics of the grid's components.  labels [nx*ny*nz] int32 in logical order, sizes the same shape or NULL
 * (not wanted), stats [4] int32; all three are written entirely, of the workspace only its first danbo_grid_cc_workspace_bytes.
 * Five launches on `stream`, none of which waits for another workgroup; the same bits on every call.
 * DANBO_EINVAL before any launch: sigma, workspace, labels or stats null; sigma, labels, sizes or stats not 4-byte aligned, the
 * workspace not 8-byte aligned; dimensions or strides outside the limits of danbo_mesh_count; iso not finite; floor +inf or NaN. */
int danbo_grid_cc_label(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                        void* workspace, int32_t* labels /*[nx*ny*nz]*/, int32_t* sizes /*[nx*ny*nz] or NULL*/,
                        int32_t* stats /*[4]*/, void* stream);

/* The filter.  labels, sizes and stats are what danbo_grid_cc_label wrote for the same grid, floor and iso; stats is read on the
 * device (no host read is needed between the two calls); a label that is no index of the grid reads as outside.  out: element
 * (i, j, k) at out[i * out_stride_x + j * out_stride_y + k], every point at an address of its own (out_stride_y >= nz and
 * out_stride_x >= ny * out_stride_y, or out_stride_x >= nz and out_stride_y >= nx * out_stride_x: a contiguous array or its x-y
 * transposed view); out == sigma with sigma's strides is allowed (in place).  kept [2] int32 or NULL.  out and kept are written
 * entirely.  keep_largest = 0, min_points = 0: out is a copy of sigma.
 * DANBO_EINVAL before any launch: what danbo_grid_cc_label rejects of the grid; sigma, labels, sizes, stats or out null; any pointer
 * not 4-byte aligned; min_points < 0; a fill that is not outside (max(fill, floor) >= iso; a NaN fill reads as -inf and passes); an
 * out layout other than the two above; out sharing an address with sigma without being the in-place case. */
int danbo_grid_cc_keep(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                       const int32_t* labels /*[nx*ny*nz]*/, const int32_t* sizes /*[nx*ny*nz]*/, const int32_t* stats /*[4]*/,
                       int keep_largest, int min_points, float fill, float* out, long out_stride_x, long out_stride_y,
                       int32_t* kept /*[2] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
