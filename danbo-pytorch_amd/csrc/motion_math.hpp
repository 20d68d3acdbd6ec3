// The set-up of a frame of a pose sequence: the kinematic chain of the 24-joint SMPL tree (get_smpl_l2ws, reference
// core/utils/skeleton_utils.py:334-376) with its rigid inverses, joint positions and bounding cylinders (get_kp_bounding_cylinder,
// :568-618, head='-y'), and the rays of the pixels of an image box (get_rays / kp_to_valid_rays, core/utils/ray_utils.py:7-30,
// 84-138) -- include/danbo_motion.h, k_motion.hip.
//
// Like skel_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels and compiled by g++ for the serial
// restatement at the end of this file (motion_chain_host / motion_box_rays_host), which the CPU tests check against
// tests/motion_ref.py (numpy float32) and the GPU tests compare the kernels with, bit for bit.  Built with -ffp-contract=off; this
// file says fmaf nowhere.  Every product of a row with a column has the one order ((p0 m0 + p1 m1) + p2 m2) [+ t].
//
// A 4 x 4 rigid matrix is held as its first three rows, m[12] row-major (m[3], m[7], m[11]: the translation); the fourth row
// (0, 0, 0, 1) exists only where a matrix is stored.
//
// CHAIN, per pose: joint 0: [R_0 | rest_0]; joint j > 0: parent . [R_j | rest_j - rest_parent] (the difference in float32),
//     rotation    out[r][c] = (P[r][0] R[0][c] + P[r][1] R[1][c]) + P[r][2] R[2][c]
//     translation out[r][3] = ((P[r][0] t0 + P[r][1] t1) + P[r][2] t2) + P[r][3]
// then, when roots are given, roots[n] is added to the three translations of every joint (after the chain, as the loaders of
// run_render.py do: the chain itself never sees the root position).
// INVERSE: S[r][c] = M[c][r],  S[r][3] = -((M[0][r] t0 + M[1][r] t1) + M[2][r] t2) with t the translation of M.
// CYLINDER: root = kp_0;  dist_j = sqrt(dx dx + dz dz), d = kp_j - root;  (root_x, root_z, max_j dist_j + ext,
//     -(max_j(-y_j) + ext_top), -(min_j(-y_j) - ext_bot)).  max and min propagate NaN as numpy's do and order -0 below +0, so they are
//     associative and commutative: a serial sweep and a wave reduction give the same bits.
// RAY of pixel (x, y): dir = ((x - cx) / fx, -((y - cy) / fy), -1);  d[r] = (dir0 c[r][0] + dir1 c[r][1]) + dir2 c[r][2];
//     o[r] = c[r][3].
#pragma once
#include "sample_math.hpp"

namespace danbo {

constexpr int MOTION_LEVELS = 9;                  // depths 0 .. 8 of the tree; joints 22 and 23 sit at depth 8
constexpr int MOTION_MAX_POSES = 1 << 20, MOTION_MAX_DIM = 1 << 15;

// SMPLSkeleton.joint_trees and every joint's depth (tests/test_motion_host.py holds both tables to the Python tree)
DANBO_HD int motion_parent(int j) {
    constexpr int8_t parent[J] = {0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
    return parent[j];
}
DANBO_HD int motion_depth(int j) {
    constexpr int8_t depth[J] = {0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 6, 6, 7, 7, 8, 8};
    return depth[j];
}

DANBO_HD float motion_dot3(float p0, float m0, float p1, float m1, float p2, float m2) {
    return add_rn(add_rn(mul_rn(p0, m0), mul_rn(p1, m1)), mul_rn(p2, m2));
}

// the translation of joint j's local matrix
DANBO_HD void motion_local_t(const float* rest, int j, float* t) {
    const int p = motion_parent(j);
    for (int k = 0; k < 3; ++k) t[k] = j == 0 ? rest[k] : sub_rn(rest[3 * j + k], rest[3 * p + k]);
}

// out = P . [R | t]  (P, out: 3 x 4; R: 3 x 3 row-major); out may not alias P
DANBO_HD void motion_compose(const float* P, const float* R, const float* t, float* out) {
    for (int r = 0; r < 3; ++r) {
        const float p0 = P[4 * r], p1 = P[4 * r + 1], p2 = P[4 * r + 2];
        for (int c = 0; c < 3; ++c) out[4 * r + c] = motion_dot3(p0, R[c], p1, R[3 + c], p2, R[6 + c]);
        out[4 * r + 3] = add_rn(motion_dot3(p0, t[0], p1, t[1], p2, t[2]), P[4 * r + 3]);
    }
}

// S = M^-1 of a rigid M
DANBO_HD void motion_inverse(const float* M, float* S) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) S[4 * r + c] = M[4 * c + r];
        S[4 * r + 3] = -motion_dot3(M[r], M[3], M[4 + r], M[7], M[8 + r], M[11]);
    }
}

DANBO_HD bool motion_negative(float a) { return __builtin_signbitf(a) != 0; }
DANBO_HD float motion_max(float a, float b) {
    if (a != a || b != b) return add_rn(a, b);
    if (a == b) return motion_negative(a) ? b : a;      // -0 < +0
    return a > b ? a : b;
}
DANBO_HD float motion_min(float a, float b) {
    if (a != a || b != b) return add_rn(a, b);
    if (a == b) return motion_negative(a) ? a : b;
    return a < b ? a : b;
}
// the horizontal distance of a joint at (x, z) from the root at (rx, rz)
DANBO_HD float motion_dist(float x, float z, float rx, float rz) {
    const float dx = sub_rn(x, rx), dz = sub_rn(z, rz);
    return sqrtf(add_rn(mul_rn(dx, dx), mul_rn(dz, dz)));
}
// cyl[5] from the root and the three extrema of a pose
DANBO_HD void motion_cylinder(float rx, float rz, float dist, float hi, float lo, float ext, float ext_top, float ext_bot, float* cyl) {
    cyl[0] = rx;
    cyl[1] = rz;
    cyl[2] = add_rn(dist, ext);
    cyl[3] = -add_rn(hi, ext_top);
    cyl[4] = -sub_rn(lo, ext_bot);
}

// the ray of pixel (x, y) through c [3 rows of 4]
DANBO_HD void motion_ray(const float* c, float fx, float fy, float cx, float cy, int x, int y, float* o, float* d) {
    const float d0 = div_rn(sub_rn((float)x, cx), fx), d1 = -div_rn(sub_rn((float)y, cy), fy), d2 = -1.f;
    for (int r = 0; r < 3; ++r) {
        d[r] = motion_dot3(d0, c[4 * r], d1, c[4 * r + 1], d2, c[4 * r + 2]);
        o[r] = c[4 * r + 3];
    }
}

DANBO_HD bool motion_box_ok(int W, int x0, int y0, int x1, int y1) {
    return W >= 1 && W <= MOTION_MAX_DIM && x0 >= 0 && x0 <= x1 && x1 <= W && y0 >= 0 && y0 <= y1 && y1 <= MOTION_MAX_DIM;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial restatement (host): the same calls as danbo_pose_chain / danbo_box_rays without the stream, the same definitions, one
// pose, one joint and one pixel after the other.  Returns 0, or -22 for a rejected argument.
inline int motion_chain_host(const float* rots, const float* rest, const float* roots, int N, float* l2ws, float* skts, float* kps,
                             float* cyls, float ext, float ext_top, float ext_bot) {
    if (!rots || !rest || (!l2ws && !skts && !kps && !cyls) || N < 1 || N > MOTION_MAX_POSES) return -22;
    for (long n = 0; n < N; ++n) {
        float M[J][12];
        for (int j = 0; j < J; ++j) {
            const float* R = rots + (n * J + j) * 9;
            float t[3];
            motion_local_t(rest, j, t);
            if (j == 0) {
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) M[0][4 * r + c] = R[3 * r + c];
                    M[0][4 * r + 3] = t[r];
                }
            } else {
                motion_compose(M[motion_parent(j)], R, t, M[j]);
            }
        }
        if (roots)
            for (int j = 0; j < J; ++j)
                for (int r = 0; r < 3; ++r) M[j][4 * r + 3] = add_rn(M[j][4 * r + 3], roots[3 * n + r]);
        float dist = 0.f, hi = 0.f, lo = 0.f;
        for (int j = 0; j < J; ++j) {
            float S[12];
            motion_inverse(M[j], S);
            const float d = motion_dist(M[j][3], M[j][11], M[0][3], M[0][11]), ny = -M[j][7];
            dist = j ? motion_max(dist, d) : d;
            hi = j ? motion_max(hi, ny) : ny;
            lo = j ? motion_min(lo, ny) : ny;
            for (int k = 0; k < 16; ++k) {
                const float last = k == 15 ? 1.f : 0.f;
                if (l2ws) l2ws[(n * J + j) * 16 + k] = k < 12 ? M[j][k] : last;
                if (skts) skts[(n * J + j) * 16 + k] = k < 12 ? S[k] : last;
            }
            if (kps)
                for (int r = 0; r < 3; ++r) kps[(n * J + j) * 3 + r] = M[j][4 * r + 3];
        }
        if (cyls) motion_cylinder(M[0][3], M[0][11], dist, hi, lo, ext, ext_top, ext_bot, cyls + n * 5);
    }
    return 0;
}

inline int motion_box_rays_host(const float* c2w, float fx, float fy, float cx, float cy, int W, int x0, int y0, int x1, int y1,
                                float* rays_o, float* rays_d, int64_t* idx) {
    if (!c2w || !rays_o || !rays_d || !idx || !motion_box_ok(W, x0, y0, x1, y1)) return -22;
    long t = 0;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x, ++t) {
            motion_ray(c2w, fx, fy, cx, cy, x, y, rays_o + 3 * t, rays_d + 3 * t);
            idx[t] = (int64_t)y * W + x;
        }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
