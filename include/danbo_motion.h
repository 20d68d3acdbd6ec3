/*
 * libdanbo_hip.so -- C ABI of the motion set-up: everything in front of a rendered frame of a pose sequence.  Axis-angle poses to
 * rotation matrices, the kinematic chain of the 24-joint SMPL tree with its rigid inverses, joint positions and bounding cylinders,
 * and the rays of the pixels of one camera's image box (csrc/k_motion.hip; csrc/motion_math.hpp states the per-element arithmetic of
 * the chain and of the rays once, for the kernels and for the serial restatement motion_chain_host / motion_box_rays_host that the
 * tests compare the kernels with bit for bit).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer to float32 (int64 where said) aligned to
 * its element, no function retains a pointer past the call, every kernel is enqueued on `stream` (a hipStream_t passed as void*),
 * nothing allocates or synchronises; the return value is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected
 * argument, before any launch and with no output touched.  The entries are additive in ABI 9 (danbo_abi_version() of danbo_hip.h
 * stays 9).  This header declares no struct.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/motion.py parses it with _hip.bind_headers beside the headers of _hip.HEADERS and danbo_mesh_score.h and
 * sets the types of its entries on the library.
 *
 * Every result is a function of the inputs alone: no atomics, two calls give the same bits.  danbo_pose_chain and danbo_box_rays
 * are fp32 operations in the one order motion_math.hpp fixes (no contraction); danbo_pose_rotations calls the device's sinf, which
 * is why it is an entry of its own: what follows the matrices is exact against the restatement, the matrices are checked against
 * float64.
 */
#ifndef DANBO_MOTION_H
#define DANBO_MOTION_H

#include <stddef.h>
#include <stdint.h>

#define DANBO_MOTION_MAX_POSES 1048576 /* N of danbo_pose_rotations / danbo_pose_chain: 1 .. 2^20 */
#define DANBO_MOTION_MAX_DIM 32768     /* W and y1 of danbo_box_rays */

#ifdef __cplusplus
extern "C" {
#endif

/* Axis-angle to rotation matrices (the rotation step of get_smpl_l2ws, reference core/utils/skeleton_utils.py:349-350: scipy's
 * Rotation.from_rotvec(p).as_matrix(), joint by joint on the host).  For every joint's v = (x, y, z), with t2 = (x x + y y) + z z
 * and t = sqrt(t2): R = I + a K + b K^2, K the cross-product matrix of the un-normalised v, a = sin t / t, b = 2 sin^2(t / 2) / t2;
 * for t < 2^-6 the series a = 1 - t2 / 6, b = 1 / 2 - t2 / 24 (their truncation, t^4 / 120 and t^4 / 720, is below 2^-30 there).
 * v = 0 gives the exact identity.  One thread per joint: a NaN or infinity among a joint's three numbers stays in that joint's
 * matrix.  One launch.
 * DANBO_EINVAL: a null pointer; N outside 1 .. DANBO_MOTION_MAX_POSES. */
int danbo_pose_rotations(const float* bones /*[N,24,3]*/, int N, float* rots /*[N,24,3,3]*/, void* stream);

/* The kinematic chain of N poses (get_smpl_l2ws, reference core/utils/skeleton_utils.py:334-376, called pose by pose and followed
 * by np.linalg.inv in every loader of run_render.py, e.g. :717-720; get_kp_bounding_cylinder, :568-618, called by kp_to_valid_rays, ray_utils.py:84-138).
 * The tree is SMPL's 24-joint tree, a table of the library.  The root's local-to-world matrix is [R_0 | rest_pose[0]], every other
 * joint's is parent . [R_j | rest_pose[j] - rest_pose[parent]]; roots[n] (when given) is then added to every translation of pose n.
 *   l2ws [N,24,4,4]  the local-to-world matrices, last row (0, 0, 0, 1)
 *   skts [N,24,4,4]  their rigid inverses in closed form, [R^T | -R^T t]
 *   kps  [N,24,3]    the joint positions: the translations
 *   cyls [N,5]       get_kp_bounding_cylinder(kps, head='-y'): (root x, root z, max_j |(kp_j - root)_xz| + ext, -(max_j(-y_j) + ext_top),
 *                    -(min_j(-y_j) - ext_bot)); ext, ext_top, ext_bot are the float32 values of extend x ext_scale, of that times
 *                    the top ratio and of that times the bottom ratio, rounded by the caller
 * Any of the four outputs may be NULL (it is not written), not all of them.  One launch: one lane per joint, two poses per
 * wavefront, the tree walked level by level.
 * DANBO_EINVAL: rots or rest_pose null; every output null; N outside 1 .. DANBO_MOTION_MAX_POSES. */
int danbo_pose_chain(const float* rots /*[N,24,3,3]*/, const float* rest_pose /*[24,3]*/, const float* roots /*[N,3] or NULL*/, int N,
                     float* l2ws /*[N,24,4,4] or NULL*/, float* skts /*[N,24,4,4] or NULL*/, float* kps /*[N,24,3] or NULL*/,
                     float* cyls /*[N,5] or NULL*/, float ext, float ext_top, float ext_bot, void* stream);

/* The rays of the pixels x0 <= x < x1, y0 <= y < y1 of one pinhole camera that looks down -z (get_rays indexed by the box: reference
 * core/utils/ray_utils.py:7-30 and :84-138, kp_to_valid_rays), in row-major order of the box, n = (x1 - x0) (y1 - y0) of them:
 *   dir    = ((x - cx) / fx, -((y - cy) / fy), -1)
 *   rays_d = ((dir0 c2w[r][0] + dir1 c2w[r][1]) + dir2 c2w[r][2]) for r = 0, 1, 2;  rays_o = (c2w[0][3], c2w[1][3], c2w[2][3])
 *   idx    = y W + x
 * An empty box (x1 == x0 or y1 == y0) returns 0 without a launch.  One launch, one thread per pixel.
 * DANBO_EINVAL: a null pointer; W outside 1 .. DANBO_MOTION_MAX_DIM; not 0 <= x0 <= x1 <= W; not 0 <= y0 <= y1 <= DANBO_MOTION_MAX_DIM. */
int danbo_box_rays(const float* c2w /*[4,4], rows 0 .. 2 are read*/, float fx, float fy, float cx, float cy, int W, int x0, int y0, int x1,
                   int y1, float* rays_o /*[n,3]*/, float* rays_d /*[n,3]*/, int64_t* idx /*[n]*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
