/*
 * libdanbo_hip.so -- C ABI of the depth and normal maps of the volume renderer: the expected depth sum_k w_k z_k and a level
 * (median) depth of every ray from the weights and sorted depths the final composite made, and the normal map of an assembled
 * depth frame (csrc/k_depth.hip; csrc/depth_math.hpp states every definition once, for the kernels and for the serial restatement
 * depth_composite_host / depth_normals_host that the tests compare the kernels with bit for bit).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_depth.h").
 *
 * Both results are functions of the inputs alone: every operation is a separately rounded fp32 one in an order depth_math.hpp
 * fixes, no atomics; two calls give the same bits.
 */
#ifndef DANBO_DEPTH_H
#define DANBO_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per ray r, over the n = S + Sf positions of its sorted order (1 <= n <= 320), weights [R,n] the final composite's (T_i of the
 * frame's result) and z_sorted [R,n] its depths:
 *   depth[r]       = sum_k w_k z_k: lane l of the ray's wavefront adds positions l, l + 64, ... in order, one fixed tree adds the 64
 *                    partial sums (the order of danbo_composite_colors_fwd); a position of weight 0 contributes +0
 *   depth_level[r] = z_k of the first position k whose inclusive prefix sum of w (in the fixed order of depth_math.hpp) is >= level,
 *                    0 < level <= 1 (0.5: the median depth); +0 when no position reaches it
 * ray_list / ray_count (both or neither; the list of danbo_flat_rays): only rays ray_list[0 .. *ray_count) are read and written --
 * the z_sorted rows of the other rays (rays of constants) need not exist; the caller pre-zeroes the outputs, those rays' exact
 * result.  An entry of the list is read clamped to 0 .. R - 1, the count to 0 .. R.  One launch, one wavefront per ray.
 * DANBO_EINVAL before any launch: weights, z_sorted, depth or depth_level null; R < 0; n outside 1 .. 320; level outside (0, 1]
 * or NaN; only one of ray_list / ray_count. */
int danbo_depth_composite_fwd(const float* weights /*[R,n]*/, const float* z_sorted /*[R,n]*/, int R, int n, float level,
                              const int32_t* ray_list /*[R] or NULL*/, const int32_t* ray_count /*[1] or NULL*/, float* depth /*[R]*/,
                              float* depth_level /*[R]*/, void* stream);

/* The normal map of N assembled frames.  depth, acc [N,H,W] (0 outside the cast box); cast_mask [N,H,W] uint8 (0: the pixel was
 * not cast) or NULL (every pixel was); c2w [N,3,4] row-major; intr [N,4] = (fx, fy, cx, cy) per frame.  Pixel depth D = depth /
 * acc; a pixel is usable iff cast, acc >= acc_min and D > 0; its camera-space point is (D (x - cx) / fx, -D (y - cy) / fy, -D);
 * the normal is the normalised cross product of the central (one-sided at a hole or border) differences of the points along the
 * row and the column, turned towards the camera; jump > 0 leaves out a neighbour whose D differs by more than jump.  space 0:
 * camera space (x right, y up, z towards the camera), 1: world space (rotated by c2w[:3,:3]).  out_rgb [N,H,W,3] = 0.5 n + 0.5,
 * `background` in all three channels where the pixel has no normal; out_valid [N,H,W] uint8 or NULL: 1 with a normal, else 0.
 * Both outputs are written entirely.  One launch, one thread per pixel: a gather.
 * DANBO_EINVAL before any launch: depth, acc, c2w, intr or out_rgb null; N outside 1 .. 2^20; H or W outside 1 .. 4096; space other
 * than 0 or 1; jump negative or NaN. */
int danbo_depth_normals(const float* depth /*[N,H,W]*/, const float* acc /*[N,H,W]*/, const uint8_t* cast_mask /*[N,H,W] or NULL*/,
                        const float* c2w /*[N,3,4]*/, const float* intr /*[N,4]*/, int N, int H, int W, float acc_min, float jump,
                        int space, float background, float* out_rgb /*[N,H,W,3]*/, uint8_t* out_valid /*[N,H,W] or NULL*/,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif
