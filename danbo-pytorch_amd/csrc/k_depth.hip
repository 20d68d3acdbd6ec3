// Depth and normal maps (include/danbo_depth.h).  Every definition is depth_math.hpp's, whose serial restatement the tests compare
// these kernels with bit for bit.
//   k_depth_composite  one wavefront per ray, like k_composite_colors: strip after strip of 64 positions, lane l reads w and z of
//                      position 64 s + l (a wavefront's loads cover one contiguous range of the two rows), adds its term into its
//                      own partial sum and takes part in the strip's DPP scan of the weights; the first lane of the first strip
//                      whose prefix reaches the level hands over its z.  One more DPP tree adds the 64 partial sums.  With a ray
//                      list only the listed rays are read and written.  8 n bytes read and 8 written per ray; no atomics, no LDS.
//   k_depth_normals    a gather, one thread per pixel: depth, acc (and cast) of the pixel and of its four neighbours -- rows of the
//                      frame that consecutive lanes read side by side --, 12 B (+1) out.
// Bounds: a position is read only for k < n inside row r < R (a list entry is clamped to 0 .. R - 1, the count to 0 .. R); a
// neighbour is read only inside its frame (depth_neighbour); the pixel index stays below N H W <= 2^44 (long).
#include "common.hpp"
#include "depth_math.hpp"
#include "../../include/danbo_depth.h"

namespace danbo {

constexpr int DEPTH_BLOCK = 256;

__global__ __launch_bounds__(DEPTH_BLOCK) void k_depth_composite(const float* __restrict__ weights, const float* __restrict__ z_sorted,
                                                                 int R, int n, float level, const int32_t* __restrict__ ray_list,
                                                                 const int32_t* __restrict__ ray_count, float* __restrict__ depth,
                                                                 float* __restrict__ depth_level) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int count = ray_list ? min(max(*ray_count, 0), R) : R;
    for (int i = wave; i < count; i += nwaves) {
        const int r = ray_list ? min(max(ray_list[i], 0), R - 1) : i;
        const float* w_row = weights + (size_t)r * n;
        const float* z_row = z_sorted + (size_t)r * n;
        float part = 0.f, carry = 0.f, at_level = 0.f;
        bool found = false;
        for (int base = 0; base < n; base += 64) {
            const int k = base + lane;
            const bool in = k < n;
            const float w = in ? w_row[k] : 0.f;
            const float z = in ? z_row[k] : 0.f;
            if (in) part = add_rn(part, depth_term(w, z));
            const float prefix = depth_prefix(carry, wave_scan_add(w));
            if (!found) {      // (wave-uniform)
                const unsigned long long hit = __ballot(in && depth_reached(prefix, level));
                if (hit != 0ull) {
                    found = true;
                    at_level = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, z), __ffsll(hit) - 1));
                }
            }
            carry = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, prefix), 63));
        }
        part = wave_total(part);
        if (lane == 0) depth[r] = part, depth_level[r] = at_level;
    }
}

__global__ __launch_bounds__(DEPTH_BLOCK) void k_depth_normals(const float* __restrict__ depth, const float* __restrict__ acc,
                                                               const uint8_t* __restrict__ cast, const float* __restrict__ c2w,
                                                               const float* __restrict__ intr, int N, int H, int W, float acc_min,
                                                               float jump, int space, float background, float* __restrict__ out_rgb,
                                                               uint8_t* __restrict__ out_valid) {
    const long total = (long)N * H * W, stride = (long)gridDim.x * DEPTH_BLOCK;
    for (long at = (long)blockIdx.x * DEPTH_BLOCK + threadIdx.x; at < total; at += stride) {
        const int n = (int)(at / ((long)H * W));
        const int rest = (int)(at - (long)n * H * W);
        const int y = rest / W, x = rest - y * W;
        float rgb[3];
        const int ok = depth_normal_pixel(depth, acc, cast, c2w, intr, n, H, W, x, y, acc_min, jump, space, background, rgb);
        out_rgb[3 * at] = rgb[0], out_rgb[3 * at + 1] = rgb[1], out_rgb[3 * at + 2] = rgb[2];
        if (out_valid) out_valid[at] = (uint8_t)ok;
    }
}

}  // namespace danbo

using namespace danbo;

extern "C" int danbo_depth_composite_fwd(const float* weights, const float* z_sorted, int R, int n, float level, const int32_t* ray_list,
                                         const int32_t* ray_count, float* depth, float* depth_level, void* stream) {
    DANBO_CHECK_ARG(depth_composite_ok(weights, z_sorted, R, n, level, ray_list, ray_count, depth, depth_level));
    if (R == 0) return 0;
    hipLaunchKernelGGL(k_depth_composite, dim3(stream_grid((long)R * 64, DEPTH_BLOCK)), dim3(DEPTH_BLOCK), 0, (hipStream_t)stream, weights,
                       z_sorted, R, n, level, ray_list, ray_count, depth, depth_level);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_depth_normals(const float* depth, const float* acc, const uint8_t* cast_mask, const float* c2w, const float* intr,
                                   int N, int H, int W, float acc_min, float jump, int space, float background, float* out_rgb,
                                   uint8_t* out_valid, void* stream) {
    DANBO_CHECK_ARG(depth_normals_ok(depth, acc, c2w, intr, N, H, W, jump, space, out_rgb));
    hipLaunchKernelGGL(k_depth_normals, dim3(stream_grid((long)N * H * W, DEPTH_BLOCK)), dim3(DEPTH_BLOCK), 0, (hipStream_t)stream, depth,
                       acc, cast_mask, c2w, intr, N, H, W, acc_min, jump, space, background, out_rgb, out_valid);
    DANBO_LAUNCH_RET();
}
