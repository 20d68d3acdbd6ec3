// Bone-assignment maps (--render_confd / --render_entropy): the colour of every sample from its 24 assignment logits, and the
// composite of those colours with the weights the ordinary render already made.  Reference: get_confidence_rgb / get_entropy_rgb
// (core/networks/misc.py:620-673) inside raw2outputs (core/networks/nerf.py:306-313), where the colour replaces sigmoid(raw[..., :3])
// and rgb_map = sum_k w_k c_k.  Nothing here changes a weight: the two kernels only read what the frame's composites wrote.
#include "common.hpp"
#include "../../include/danbo_partmap.h"

namespace danbo {

constexpr int PC_BLOCK = 256;
constexpr float PC_INV_LOG_J = 0.31465838776377636f;   // 1 / ln 24
constexpr float PC_EPS = 1e-7f;                         // get_entropy_rgb's eps

// One lane per row: six 16-byte loads of the row's 96 B of logits (consecutive lanes read consecutive rows, so a wavefront consumes
// whole cache lines), 12 B out.  Row i belongs to sample m = list ? list[i] : i; rows at or beyond *count are not touched.
//   mode 0: the palette colour of the bone with the largest logit, the lowest index on a tie (torch.argmax)
//   mode 1: lerp((0,0,1), (1,0,0), H / ln 24), H = -sum p log(p + 1e-7), p = softmax(logits): (t, 0, 1 - t)
//   valid_only: bones whose bit of valid_bits[m] is clear take no part in the argmax / the softmax (p = 0); no bone at all: colour 0
// expf / logf are the accurate library functions: the entropy is within a few 1e-6 of its float64 value.
__global__ __launch_bounds__(PC_BLOCK) void k_part_colors(const f32x4* __restrict__ confd, const uint32_t* __restrict__ bits,
                                                          const int32_t* __restrict__ list, const int32_t* __restrict__ count, int n_cap,
                                                          int mode, int valid_only, const float* __restrict__ palette,
                                                          float* __restrict__ rgb) {
    const int n = resolve_count(count, n_cap);
    const long stride = (long)gridDim.x * PC_BLOCK;
    for (long i = (long)blockIdx.x * PC_BLOCK + threadIdx.x; i < n; i += stride) {
        float x[J];
#pragma unroll
        for (int q = 0; q < J / 4; ++q) {
            const f32x4 v = confd[i * (J / 4) + q];
            x[4 * q] = v[0], x[4 * q + 1] = v[1], x[4 * q + 2] = v[2], x[4 * q + 3] = v[3];
        }
        const long m = list ? (long)list[i] : i;
        if (m < 0) continue;
        const uint32_t live = valid_only ? (bits[m] & ((1u << J) - 1u)) : ((1u << J) - 1u);
        float mx = -INFINITY;
        int arg = -1;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool on = ((live >> j) & 1u) != 0u;
            if (on && (arg < 0 || x[j] > mx)) mx = x[j], arg = j;      // strict >: the lowest index keeps a tie
        }
        float r = 0.f, g = 0.f, b = 0.f;
        if (arg >= 0) {
            if (mode == 0) {
                r = palette[3 * arg], g = palette[3 * arg + 1], b = palette[3 * arg + 2];
            } else {
                float e[J], sum = 0.f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    e[j] = ((live >> j) & 1u) ? expf(x[j] - mx) : 0.f;
                    sum += e[j];
                }
                float ent = 0.f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const float p = e[j] / sum;
                    ent -= p * logf(p + PC_EPS);
                }
                const float t = ent * PC_INV_LOG_J;
                r = t, b = 1.f - t;
            }
        }
        rgb[3 * m] = r, rgb[3 * m + 1] = g, rgb[3 * m + 2] = b;
    }
}

// One wavefront per ray, like the composites: lane l takes positions l, l + 64, ... of the ray's sorted order, adds w c for each
// into its own three sums (products and sums rounded separately), and the wavefront's DPP tree adds the 64 partial sums -- a fixed
// order, so the map is a pure function of the inputs.  A sample of weight 0 contributes +0 and its colour is not loaded (most
// samples of a frame); a sample whose in-volume word is 0 has no colour row and is not read either.
__global__ __launch_bounds__(PC_BLOCK) void k_composite_colors(const float* __restrict__ rgb_a, const float* __restrict__ rgb_b,
                                                               const uint32_t* __restrict__ bits_a, const uint32_t* __restrict__ bits_b,
                                                               const int32_t* __restrict__ sorted_idx, const float* __restrict__ weights,
                                                               int R, int S, int Sf, const int32_t* __restrict__ ray_list,
                                                               const int32_t* __restrict__ ray_count, float* __restrict__ rgb_map) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int n = ray_list ? min(max(*ray_count, 0), R) : R;
    const int N = S + Sf;
    for (int i = wave; i < n; i += nwaves) {
        const int r = ray_list ? min(max(ray_list[i], 0), R - 1) : i;
        float sr = 0.f, sg = 0.f, sb = 0.f;
        for (int k = lane; k < N; k += 64) {
            const size_t at = (size_t)r * N + k;
            const float w = weights[at];
            if (w == 0.f) continue;
            const int src = sorted_idx ? min(max(sorted_idx[at], 0), N - 1) : k;
            const bool fine = src >= S;
            const size_t m = fine ? (size_t)r * Sf + (src - S) : (size_t)r * S + src;
            const uint32_t* bits = fine ? bits_b : bits_a;
            if (bits != nullptr && bits[m] == 0u) continue;
            const float* c = (fine ? rgb_b : rgb_a) + 3 * m;
            sr = add_rn(sr, mul_rn(w, c[0]));
            sg = add_rn(sg, mul_rn(w, c[1]));
            sb = add_rn(sb, mul_rn(w, c[2]));
        }
        sr = wave_total(sr), sg = wave_total(sg), sb = wave_total(sb);
        if (lane == 0) rgb_map[3 * (size_t)r] = sr, rgb_map[3 * (size_t)r + 1] = sg, rgb_map[3 * (size_t)r + 2] = sb;
    }
}

}  // namespace danbo

using namespace danbo;

extern "C" int danbo_part_colors_fwd(const float* confd, const uint32_t* valid_bits, const int32_t* list, const int32_t* count, int n,
                                     int mode, int valid_only, const float* palette, float* rgb, void* stream) {
    DANBO_CHECK_ARG((mode == 0 || mode == 1) && n >= 0);
    DANBO_CHECK_ARG(!valid_only || valid_bits != nullptr);
    DANBO_CHECK_ARG(mode != 0 || palette != nullptr);
    DANBO_CHECK_ARG(confd != nullptr && rgb != nullptr && ((uintptr_t)confd & 15) == 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_part_colors, dim3(stream_grid(n, PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x4*>(confd), valid_bits, list, count, n, mode, valid_only ? 1 : 0, palette, rgb);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_composite_colors_fwd(const float* rgb_a, const float* rgb_b, const uint32_t* bits_a, const uint32_t* bits_b,
                                          const int32_t* sorted_idx, const float* weights, int R, int S, int Sf,
                                          const int32_t* ray_list, const int32_t* ray_count, float* rgb_map, void* stream) {
    DANBO_CHECK_ARG(R >= 0 && S >= 1 && Sf >= 0 && Sf <= 64);
    // the identity form carries an already sorted row of up to 256 + 64 samples in rgb_a
    DANBO_CHECK_ARG(sorted_idx != nullptr ? S <= 256 : (S <= 256 + 64 && Sf == 0 && rgb_b == nullptr));
    DANBO_CHECK_ARG((ray_list == nullptr) == (ray_count == nullptr));
    DANBO_CHECK_ARG(rgb_a != nullptr && weights != nullptr && rgb_map != nullptr && (Sf == 0 || rgb_b != nullptr));
    if (R == 0) return 0;
    hipLaunchKernelGGL(k_composite_colors, dim3(stream_grid((long)R * 64, PC_BLOCK)), dim3(PC_BLOCK), 0, (hipStream_t)stream, rgb_a,
                       rgb_b, bits_a, bits_b, sorted_idx, weights, R, S, Sf, ray_list, ray_count, rgb_map);
    DANBO_LAUNCH_RET();
}
