/*
 * libdanbo_hip.so -- C ABI of the skeleton overlay: the posed 24-joint skeleton projected into every frame and drawn over it, the
 * `skel/` output of the reference's run_render.py (draw_skeletons_3d), made where the frames lie (csrc/k_skel.hip;
 * csrc/skel_math.hpp states every definition once, for the kernels and for the serial restatement skel_project_host /
 * skel_draw_host that the tests compare the kernels with bit for bit).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_skel.h").
 *
 * Definitions (csrc/skel_math.hpp has them in full).  Frames are [N,H,W,3], N 1 .. 2^20, H and W 1 .. 4096.  ends [N,24,4] int32
 * holds per frame and bone j the segment {ax, ay, bx, by} from joint j to its parent in pixels, x along W; ax = INT32_MIN marks a
 * bone that is not drawn, every other coordinate is read clamped to [-2^30, 2^30].  A pixel (x, y) is covered by a segment at
 * width w iff its centre lies within w / 2 of it, decided exactly in integers; it takes the colour of the largest covering bone,
 * else the source pixel: a uint8 source copied, a float32 source as min(max(trunc(255 c), 0), 255) with NaN as 0.  Every output
 * is an integer: the result is a function of the inputs alone, two calls give the same bits; no atomics.
 */
#ifndef DANBO_SKEL_H
#define DANBO_SKEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The segment ends of every bone of every frame, in float32 with separately rounded operations: the joint through w2c (the
 * world-to-camera matrix, rows 0 .. 2), u = fx x / (z + 1e-8) + ox (a quotient of +inf reads as 0), v likewise; the ends rounded
 * to nearest-even; a NaN or -inf coordinate marks the bone as not drawn.  focals holds focal_stride (1: one focal, 2: fx, fy)
 * values per frame; centers [N,2] holds (ox, oy) per frame, NULL: (W / 2, H / 2).  One launch.
 * DANBO_EINVAL before any launch: kps, w2c, focals or ends null; a pointer not 4-byte aligned; focal_stride other than 1 or 2;
 * N, H or W outside the limits above. */
int danbo_skel_project(const float* kps /*[N,24,3]*/, const float* w2c /*[N,3,4]*/, const float* focals /*[N,focal_stride]*/,
                       int focal_stride, const float* centers /*[N,2] or NULL*/, int N, int H, int W, int32_t* ends /*[N,24,4]*/,
                       void* stream);

/* The overlay.  src [N,H,W,3] float32 (src_is_float = 1) or uint8 (0), colours [24,3] uint8 (r, g, b of every bone), width 1 .. 64,
 * dst [N,H,W,3] uint8, written entirely.  One launch; a gather: every thread writes pixels of its own.
 * DANBO_EINVAL before any launch: src, ends, colours or dst null; a float32 src or ends not 4-byte aligned; src_is_float other than
 * 0 or 1; width, N, H or W outside their limits; dst sharing an address with src. */
int danbo_skel_draw(const void* src, int src_is_float, const int32_t* ends /*[N,24,4]*/, const uint8_t* colours /*[24,3]*/, int width,
                    int N, int H, int W, uint8_t* dst /*[N,H,W,3]*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
