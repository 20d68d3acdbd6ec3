// The skeleton overlay (include/danbo_skel.h): the 24 bones of every frame projected to integer segment ends, and the frames
// quantised and painted in one pass where they lie.  Every definition is skel_math.hpp's, whose serial restatement the tests
// compare these kernels with bit for bit.
//   k_skel_project  one thread per (frame, bone): the joint and its parent through the frame's camera, the four ends stored together.
//   k_skel_draw     a gather.  A workgroup works on one frame: its 24 segments (clamped ends + grown bounding boxes, skel_segment)
//                   and the packed colours go into LDS once, then every thread takes groups of SKEL_PIX = 4 consecutive pixels of
//                   a row, group after group with the workgroup's stride.  A whole group is 48 B of a float32 source (three
//                   16-byte loads), 12 B of a uint8 source and 12 B of the overlay (three dwords each) wherever those addresses are
//                   aligned -- always for W % 4 == 0 and an aligned tensor --, else and in the tail of a row bytes and single floats.
//                   Consecutive lanes hold consecutive groups: a wavefront's accesses cover one contiguous range.  Every lane of a
//                   wavefront reads the same segment from LDS at the same time (a broadcast: no bank conflict); a group whose row
//                   and four columns miss a segment's box skips it with four comparisons, and only pixels inside a box reach the
//                   64 / 128-bit rule.  15 B (float32) or 6 B (uint8) of traffic per pixel; no atomics, no dependence on order.
// Bounds: a group lies inside its row (cnt = min(4, W - x0) pixels); the wide paths are taken only for cnt == 4, so they touch
// exactly the group's 48 / 12 bytes; g < H * ceil(W / 4) keeps the row inside the frame and n = blockIdx.x / per_frame < N.
#include "common.hpp"
#include "skel_math.hpp"
#include "../../include/danbo_skel.h"

namespace danbo {

constexpr int SKEL_BLOCK = 256;

// the four ends of a bone as one store (alignment 4: the pointer's)
struct SkelEnds {
    int32_t v[4];
};

__global__ __launch_bounds__(SKEL_BLOCK) void k_skel_project(const float* __restrict__ kps, const float* __restrict__ w2c,
                                                              const float* __restrict__ focals, int focal_stride,
                                                              const float* __restrict__ centers, int N, int H, int W,
                                                              int32_t* __restrict__ ends) {
    const long t = (long)blockIdx.x * SKEL_BLOCK + threadIdx.x;
    if (t >= (long)N * J) return;
    const int n = (int)(t / J), j = (int)(t - (long)n * J);
    float fx, fy, ox, oy;
    skel_camera(focals, focal_stride, centers, n, H, W, &fx, &fy, &ox, &oy);
    SkelEnds e;
    skel_bone(kps + (long)n * J * 3, w2c + (long)n * 12, fx, fy, ox, oy, j, e.v);
    *reinterpret_cast<SkelEnds*>(ends + t * 4) = e;
}

// four pixels of a uint8 frame (alignment 4: what the wide paths check)
struct SkelWords {
    uint32_t w[3];
};

__global__ __launch_bounds__(SKEL_BLOCK) void k_skel_draw(const void* __restrict__ src, int src_is_float, const int32_t* __restrict__ ends,
                                                           const uint8_t* __restrict__ colours, int width, int H, int W, int per_frame,
                                                           uint8_t* __restrict__ dst) {
    __shared__ SkelSegment s_seg[J];
    __shared__ uint32_t s_colour[J];
    const int n = blockIdx.x / per_frame, part = blockIdx.x - n * per_frame;
    if (threadIdx.x < J) {
        const int j = threadIdx.x;
        s_seg[j] = skel_segment(ends + ((long)n * J + j) * 4, width);
        s_colour[j] = skel_pack(colours[3 * j], colours[3 * j + 1], colours[3 * j + 2]);
    }
    __syncthreads();
    const int per_row = (W + SKEL_PIX - 1) / SKEL_PIX, groups = H * per_row;      // <= 2^22
    for (int g = part * SKEL_BLOCK + threadIdx.x; g < groups; g += per_frame * SKEL_BLOCK) {
        const int y = g / per_row, x0 = (g - y * per_row) * SKEL_PIX;
        const int cnt = W - x0 < SKEL_PIX ? W - x0 : SKEL_PIX;
        const long at = (((long)n * H + y) * W + x0) * 3;       // the group's first value
        uint32_t rgb[SKEL_PIX] = {0u, 0u, 0u, 0u};
        if (src_is_float) {
            const float* s = static_cast<const float*>(src) + at;
            if (cnt == SKEL_PIX && ((uintptr_t)s & 15) == 0) {
                const f32x4 a = reinterpret_cast<const f32x4*>(s)[0], b = reinterpret_cast<const f32x4*>(s)[1],
                            c = reinterpret_cast<const f32x4*>(s)[2];
                rgb[0] = skel_pack(skel_quant(a[0]), skel_quant(a[1]), skel_quant(a[2]));
                rgb[1] = skel_pack(skel_quant(a[3]), skel_quant(b[0]), skel_quant(b[1]));
                rgb[2] = skel_pack(skel_quant(b[2]), skel_quant(b[3]), skel_quant(c[0]));
                rgb[3] = skel_pack(skel_quant(c[1]), skel_quant(c[2]), skel_quant(c[3]));
            } else {
#pragma unroll
                for (int k = 0; k < SKEL_PIX; ++k)
                    if (k < cnt) rgb[k] = skel_pack(skel_quant(s[3 * k]), skel_quant(s[3 * k + 1]), skel_quant(s[3 * k + 2]));
            }
        } else {
            const uint8_t* s = static_cast<const uint8_t*>(src) + at;
            if (cnt == SKEL_PIX && ((uintptr_t)s & 3) == 0) {
                const SkelWords v = *reinterpret_cast<const SkelWords*>(s);
                rgb[0] = v.w[0] & 0xffffffu;
                rgb[1] = (v.w[0] >> 24) | ((v.w[1] & 0xffffu) << 8);
                rgb[2] = (v.w[1] >> 16) | ((v.w[2] & 0xffu) << 16);
                rgb[3] = v.w[2] >> 8;
            } else {
#pragma unroll
                for (int k = 0; k < SKEL_PIX; ++k)
                    if (k < cnt) rgb[k] = skel_pack(s[3 * k], s[3 * k + 1], s[3 * k + 2]);
            }
        }
        // paint order: ascending j, a later bone overwrites (skel_paint, with the group's reject in front of the pixels')
        for (int j = 0; j < J; ++j) {
            const SkelSegment seg = s_seg[j];
            if (y < seg.y0 || y > seg.y1 || x0 + cnt - 1 < seg.x0 || x0 > seg.x1) continue;
            const uint32_t colour = s_colour[j];
#pragma unroll
            for (int k = 0; k < SKEL_PIX; ++k)
                if (k < cnt && skel_in_box(seg, x0 + k, y) && skel_covers(seg, x0 + k, y, width)) rgb[k] = colour;
        }
        uint8_t* d = dst + at;
        if (cnt == SKEL_PIX && ((uintptr_t)d & 3) == 0) {
            SkelWords v;
            v.w[0] = rgb[0] | (rgb[1] << 24);
            v.w[1] = (rgb[1] >> 8) | (rgb[2] << 16);
            v.w[2] = (rgb[2] >> 16) | (rgb[3] << 8);
            *reinterpret_cast<SkelWords*>(d) = v;
        } else {
#pragma unroll
            for (int k = 0; k < SKEL_PIX; ++k)
                if (k < cnt) {
                    d[3 * k] = (uint8_t)rgb[k];
                    d[3 * k + 1] = (uint8_t)(rgb[k] >> 8);
                    d[3 * k + 2] = (uint8_t)(rgb[k] >> 16);
                }
        }
    }
}

static inline bool skel_aligned(const void* p, uintptr_t to) { return (uintptr_t)p % to == 0; }

}  // namespace danbo

using namespace danbo;

extern "C" int danbo_skel_project(const float* kps, const float* w2c, const float* focals, int focal_stride, const float* centers, int N,
                                  int H, int W, int32_t* ends, void* stream) {
    DANBO_CHECK_ARG(kps && w2c && focals && ends && (focal_stride == 1 || focal_stride == 2) && skel_dims_ok(N, H, W));
    DANBO_CHECK_ARG(skel_aligned(kps, 4) && skel_aligned(w2c, 4) && skel_aligned(focals, 4) && skel_aligned(centers, 4) &&
                    skel_aligned(ends, 4));
    hipLaunchKernelGGL(k_skel_project, dim3(ceil_div((long)N * J, SKEL_BLOCK)), dim3(SKEL_BLOCK), 0, (hipStream_t)stream, kps, w2c, focals,
                       focal_stride, centers, N, H, W, ends);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_skel_draw(const void* src, int src_is_float, const int32_t* ends, const uint8_t* colours, int width, int N, int H,
                               int W, uint8_t* dst, void* stream) {
    DANBO_CHECK_ARG(src && ends && colours && dst && (src_is_float == 0 || src_is_float == 1) && width >= 1 && width <= SKEL_MAX_WIDTH &&
                    skel_dims_ok(N, H, W));
    DANBO_CHECK_ARG(skel_aligned(ends, 4) && (!src_is_float || skel_aligned(src, 4)));
    const size_t n_values = (size_t)N * H * W * 3;
    DANBO_CHECK_ARG(skel_disjoint(src, n_values * (src_is_float ? 4 : 1), dst, n_values));
    // workgroups per frame: enough for the frame's groups, and no more than fill the device eight deep over all frames
    const long groups = (long)H * ((W + SKEL_PIX - 1) / SKEL_PIX);
    long per_frame = (groups + SKEL_BLOCK - 1) / SKEL_BLOCK;
    const long share = ((long)num_cu() * 8 + N - 1) / N;
    if (per_frame > share) per_frame = share;
    hipLaunchKernelGGL(k_skel_draw, dim3((unsigned)(N * per_frame)), dim3(SKEL_BLOCK), 0, (hipStream_t)stream, src, src_is_float, ends,
                       colours, width, H, W, (int)per_frame, dst);
    DANBO_LAUNCH_RET();
}
