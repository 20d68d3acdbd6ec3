// The motion set-up (include/danbo_motion.h): rotation matrices from axis-angles, the kinematic chain of N poses with inverses,
// joints and bounding cylinders, and the rays of an image box.  The arithmetic of the chain and of the rays is motion_math.hpp's,
// whose serial restatement the tests compare these kernels with bit for bit; the rotations call the device's sinf and are checked
// against float64.
//   k_pose_rotations  one thread per (pose, joint): 3 floats in, 9 out.
//   k_pose_chain      one lane per joint, 32 lanes per pose (24 live), two poses per wavefront, 8 per workgroup.  Every lane holds
//                     its local [R | t] and its 3 x 4 result in registers.  The tree is walked level by level (MOTION_LEVELS - 1 = 8
//                     steps): all 64 lanes fetch their parent's 12 numbers with a lane permute (__shfl: ds_bpermute, no LDS
//                     allocation, no barrier), and the lanes whose depth is the step's compose.  A parent has a smaller depth, so
//                     it is final when it is read.  The cylinder's max / min are xor-butterflies over the 32 lanes of a pose; the
//                     8 idle lanes carry the root's values, which the set holds anyway.  No atomics, no dependence on order.
//                     Every lane executes every permute: nothing returns early, dead lanes only skip loads and stores.
//   k_box_rays        one thread per pixel of the box.
// Bounds: a live lane has n < N and j < 24 and touches rots[(n 24 + j) 9 ..+9], roots[3 n ..+3], the 16 / 16 / 3 values of its joint
// and (lane 0 of a pose) cyls[5 n ..+5]; the 16-byte stores are taken only for a 16-byte aligned base, where every joint's matrix
// (64 bytes) is aligned too.  A ray thread has t < (x1 - x0)(y1 - y0) <= 2^30.
// DANBO_NO_PK_F32 (common.hpp): the rows' products invite packed fp32 multiplies in the operand form that is wrong on gfx950 beside
// MFMA wavefronts, and these kernels may run beside a frame's.
#include "common.hpp"
#include "motion_math.hpp"
#include "../../include/danbo_motion.h"

namespace danbo {

static_assert(MOTION_MAX_POSES == DANBO_MOTION_MAX_POSES && MOTION_MAX_DIM == DANBO_MOTION_MAX_DIM, "motion_math.hpp / danbo_motion.h");

constexpr int MOTION_BLOCK = 256, MOTION_LANES = 32;      // lanes of a pose
constexpr float MOTION_SERIES_BELOW = 0.015625f;          // 2^-6: below it a and b are their series (danbo_motion.h)

// R = I + a K + b K^2 with K^2 = v v^T - t2 I
__device__ __forceinline__ void motion_rotation(float x, float y, float z, float* R) {
    const float xx = mul_rn(x, x), yy = mul_rn(y, y), zz = mul_rn(z, z);
    const float t2 = add_rn(add_rn(xx, yy), zz), t = sqrtf(t2);
    float a, b;
    if (t < MOTION_SERIES_BELOW) {
        a = sub_rn(1.f, div_rn(t2, 6.f));
        b = sub_rn(0.5f, div_rn(t2, 24.f));
    } else {      // also NaN and infinity: the matrix is NaN
        const float s = sinf(mul_rn(0.5f, t));
        a = div_rn(sinf(t), t);
        b = div_rn(mul_rn(2.f, mul_rn(s, s)), t2);
    }
    const float bxy = mul_rn(b, mul_rn(x, y)), bxz = mul_rn(b, mul_rn(x, z)), byz = mul_rn(b, mul_rn(y, z));
    const float ax = mul_rn(a, x), ay = mul_rn(a, y), az = mul_rn(a, z);
    R[0] = sub_rn(1.f, mul_rn(b, add_rn(yy, zz)));
    R[1] = sub_rn(bxy, az);
    R[2] = add_rn(bxz, ay);
    R[3] = add_rn(bxy, az);
    R[4] = sub_rn(1.f, mul_rn(b, add_rn(xx, zz)));
    R[5] = sub_rn(byz, ax);
    R[6] = sub_rn(bxz, ay);
    R[7] = add_rn(byz, ax);
    R[8] = sub_rn(1.f, mul_rn(b, add_rn(xx, yy)));
}

__global__ __launch_bounds__(MOTION_BLOCK) DANBO_NO_PK_F32 void k_pose_rotations(const float* __restrict__ bones, int N,
                                                                                  float* __restrict__ rots) {
    const long t = (long)blockIdx.x * MOTION_BLOCK + threadIdx.x;
    if (t >= (long)N * J) return;
    float R[9];
    motion_rotation(bones[3 * t], bones[3 * t + 1], bones[3 * t + 2], R);
#pragma unroll
    for (int k = 0; k < 9; ++k) rots[9 * t + k] = R[k];
}

// a joint's 3 x 4 and the last row, 16 floats at p
__device__ __forceinline__ void motion_store(float* p, const float* m, bool wide) {
    if (wide) {
        f32x4* q = reinterpret_cast<f32x4*>(p);
        q[0] = f32x4{m[0], m[1], m[2], m[3]};
        q[1] = f32x4{m[4], m[5], m[6], m[7]};
        q[2] = f32x4{m[8], m[9], m[10], m[11]};
        q[3] = f32x4{0.f, 0.f, 0.f, 1.f};
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) p[k] = m[k];
        p[12] = 0.f; p[13] = 0.f; p[14] = 0.f; p[15] = 1.f;
    }
}

__global__ __launch_bounds__(MOTION_BLOCK) DANBO_NO_PK_F32 void k_pose_chain(const float* __restrict__ rots, const float* __restrict__ rest,
                                                                              const float* __restrict__ roots, int N,
                                                                              float* __restrict__ l2ws, float* __restrict__ skts,
                                                                              float* __restrict__ kps, float* __restrict__ cyls, float ext,
                                                                              float ext_top, float ext_bot) {
    const int lane = threadIdx.x & 63, slot = lane & (MOTION_LANES - 1), half = lane & MOTION_LANES;
    const long n = ((long)blockIdx.x * MOTION_BLOCK + threadIdx.x) / MOTION_LANES;
    const bool live = n < N && slot < J;
    const int j = slot < J ? slot : 0;
    float R[9], t[3], M[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = live ? rots[(n * J + j) * 9 + k] : 0.f;
    if (live) motion_local_t(rest, j, t);
    else t[0] = t[1] = t[2] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[4 * r] = R[3 * r]; M[4 * r + 1] = R[3 * r + 1]; M[4 * r + 2] = R[3 * r + 2]; M[4 * r + 3] = t[r];
    }
    const int parent_lane = half | motion_parent(j), depth = motion_depth(j);
    for (int d = 1; d < MOTION_LEVELS; ++d) {
        float P[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = __shfl(M[k], parent_lane, 64);
        if (depth == d) motion_compose(P, R, t, M);
    }
    if (roots) {      // (the same in every lane)
#pragma unroll
        for (int r = 0; r < 3; ++r) M[4 * r + 3] = add_rn(M[4 * r + 3], live ? roots[3 * n + r] : 0.f);
    }
    const long at = n * J + j;
    if (live && l2ws) motion_store(l2ws + at * 16, M, ((uintptr_t)l2ws & 15) == 0);
    if (live && skts) {
        float S[12];
        motion_inverse(M, S);
        motion_store(skts + at * 16, S, ((uintptr_t)skts & 15) == 0);
    }
    if (live && kps) {
        kps[at * 3] = M[3]; kps[at * 3 + 1] = M[7]; kps[at * 3 + 2] = M[11];
    }
    if (!cyls) return;      // (the same in every lane: no permute follows a lane that left)
    const float rx = __shfl(M[3], half, 64), ry = __shfl(M[7], half, 64), rz = __shfl(M[11], half, 64);
    const bool joint = slot < J;       // an idle lane carries the root
    float dist = motion_dist(joint ? M[3] : rx, joint ? M[11] : rz, rx, rz), hi = -(joint ? M[7] : ry), lo = hi;
#pragma unroll
    for (int w = MOTION_LANES / 2; w >= 1; w >>= 1) {
        dist = motion_max(dist, __shfl_xor(dist, w, 64));
        hi = motion_max(hi, __shfl_xor(hi, w, 64));
        lo = motion_min(lo, __shfl_xor(lo, w, 64));
    }
    if (live && slot == 0) {
        float c[5];
        motion_cylinder(rx, rz, dist, hi, lo, ext, ext_top, ext_bot, c);
#pragma unroll
        for (int k = 0; k < 5; ++k) cyls[n * 5 + k] = c[k];
    }
}

__global__ __launch_bounds__(MOTION_BLOCK) DANBO_NO_PK_F32 void k_box_rays(const float* __restrict__ c2w, float fx, float fy, float cx,
                                                                            float cy, int W, int x0, int y0, int bw, int count,
                                                                            float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                                            int64_t* __restrict__ idx) {
    const int t = blockIdx.x * MOTION_BLOCK + threadIdx.x;      // count <= 2^30
    if (t >= count) return;
    const int by = t / bw, x = x0 + (t - by * bw), y = y0 + by;
    float c[12], o[3], d[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = c2w[k];
    motion_ray(c, fx, fy, cx, cy, x, y, o, d);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        rays_o[3 * (long)t + r] = o[r];
        rays_d[3 * (long)t + r] = d[r];
    }
    idx[t] = (int64_t)y * W + x;
}

}  // namespace danbo

using namespace danbo;

extern "C" int danbo_pose_rotations(const float* bones, int N, float* rots, void* stream) {
    DANBO_CHECK_ARG(bones && rots && N >= 1 && N <= MOTION_MAX_POSES);
    hipLaunchKernelGGL(k_pose_rotations, dim3(ceil_div((long)N * J, MOTION_BLOCK)), dim3(MOTION_BLOCK), 0, (hipStream_t)stream, bones, N,
                       rots);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_pose_chain(const float* rots, const float* rest_pose, const float* roots, int N, float* l2ws, float* skts, float* kps,
                                float* cyls, float ext, float ext_top, float ext_bot, void* stream) {
    DANBO_CHECK_ARG(rots && rest_pose && (l2ws || skts || kps || cyls) && N >= 1 && N <= MOTION_MAX_POSES);
    hipLaunchKernelGGL(k_pose_chain, dim3(ceil_div((long)N * MOTION_LANES, MOTION_BLOCK)), dim3(MOTION_BLOCK), 0, (hipStream_t)stream, rots,
                       rest_pose, roots, N, l2ws, skts, kps, cyls, ext, ext_top, ext_bot);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_box_rays(const float* c2w, float fx, float fy, float cx, float cy, int W, int x0, int y0, int x1, int y1, float* rays_o,
                              float* rays_d, int64_t* idx, void* stream) {
    DANBO_CHECK_ARG(c2w && rays_o && rays_d && idx && motion_box_ok(W, x0, y0, x1, y1));
    const int bw = x1 - x0, count = bw * (y1 - y0);
    if (count == 0) return 0;
    hipLaunchKernelGGL(k_box_rays, dim3(ceil_div(count, MOTION_BLOCK)), dim3(MOTION_BLOCK), 0, (hipStream_t)stream, c2w, fx, fy, cx, cy, W, x0,
                       y0, bw, count, rays_o, rays_d, idx);
    DANBO_LAUNCH_RET();
}
