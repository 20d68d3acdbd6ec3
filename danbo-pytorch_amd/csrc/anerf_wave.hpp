// The per-ray pieces of A-NeRF's view branch that the render kernels (k_anerf.hip) and the training kernels (k_anerf_train.hip)
// share: device code only, one definition each.
#pragma once
#include "common.hpp"

namespace danbo {

// reference: transform_batch_rays (encoders.py:305-317) -> VecNormEncoder -> the frequency part of CutoffEmbedder._embed with
// dist_inputs (cutoff_embedder.py:156-166), one (ray, joint): e[b * bs + k], k the axis, b = 0 the unit bone-local ray direction
// u, b = 1 + 2 l: sin(2^l u), 2 + 2 l: cos(2^l u).  bs = 3: the order of views_linears.0's view columns of ONE joint (the view
// constants); bs = 72 on e = E[ray] + 3 j: the encoding of all joints (k_anerf_view_pe)
__device__ __forceinline__ void av_ray_pe(const float* __restrict__ rays_d, const float* __restrict__ skts, int R, int G, int L, int ray, int j,
                                          float* __restrict__ e, int bs) {
    const int rays_per_pose = R / G;
    const float* M = skts + ((size_t)min(ray / rays_per_pose, G - 1) * J + j) * 16;
    const float d[3] = {rays_d[3 * ray], rays_d[3 * ray + 1], rays_d[3 * ray + 2]};
    float q[3];
    rotate_unfused(M, d, q);
    normalize3(q);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = q[k];
        e[k] = u;
        for (int l = 0; l < L; ++l) {
            float sn, cs;
            sincosf(mul_rn(u, (float)(1 << l)), &sn, &cs);
            e[(1 + 2 * l) * bs + k] = sn;
            e[(2 + 2 * l) * bs + k] = cs;
        }
    }
}

// reference: the view branch of NeRF.inference (nerf.py:196-209) on encode_views' output (nerf.py:252-279).
// One wavefront per ray: the ray's 24 x VW joint vectors stay in registers while its S samples stream by.
//   x[c]   = relu(featv[row][c] + table[t][c] + sum_j w[row][j] * C[j][ray][c])
//   raw    = (rgb_w x + rgb_b, alpha[row])
// ray = ray0 + rl, row = rl * S + s: featv / w / alpha (and hv) hold the rows of the launch's rays, C and raw_out those of all.
// TRAIN = false: t = the ray's camera code (cam_idx; the mean code, row n_codes, without one or below 0).
// TRAIN = true: t = ray (a table row per ray, k_anerf_ray_table; cam_idx / n_codes unread), and hv [rows, VW] = x is kept for
// the backward.
template <bool TRAIN>
__device__ __forceinline__ void anerf_color_body(const float* __restrict__ featv, int ldf, const float* __restrict__ w,
                                                 const float* __restrict__ C, const float* __restrict__ table,
                                                 const int64_t* __restrict__ cam_idx, int n_codes, int R_total, int ray0, int nrays, int S,
                                                 int VW, const float* __restrict__ rgb_w, const float* __restrict__ rgb_b,
                                                 const float* __restrict__ alpha, int lda, float* __restrict__ hv,
                                                 float* __restrict__ raw_out) {
    const int lane = threadIdx.x & 63;
    const int wave_global = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    float rw[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rw[ch][i] = c < VW ? rgb_w[ch * VW + c] : 0.f;
    }
    const float rb0 = rgb_b[0], rb1 = rgb_b[1], rb2 = rgb_b[2];
    for (int rl = wave_global; rl < nrays; rl += nwaves) {
        const int ray = ray0 + rl;
        float cj[J][4];
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                cj[j][i] = c < VW ? C[((size_t)j * R_total + ray) * VW + c] : 0.f;
            }
        long t = ray;
        if (!TRAIN) {
            t = n_codes;  // the mean code (Optcodes eval with idx < 0)
            if (cam_idx) {
                const long idx = cam_idx[ray];
                if (idx >= 0) t = idx < n_codes ? idx : n_codes - 1;
            }
        }
        float tb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            tb[i] = c < VW ? table[(size_t)t * VW + c] : 0.f;
        }
        // four samples per trip: all their loads (16 feature values and 4 x 24 cutoff weights) are issued before the first
        // FMA, so one memory latency is paid per four samples instead of per sample (a wavefront walks its ray alone)
        constexpr int U = 4;
        for (int s0 = 0; s0 < S; s0 += U) {
            float x[U][4], wj[U][J], al[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t row = (size_t)rl * S + min(s0 + u, S - 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = lane + 64 * i;
                    x[u][i] = c < VW ? featv[row * ldf + c] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < J; ++j) wj[u][j] = w[row * J + j];
                al[u] = alpha[row * lda];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[u][i] = (lane + 64 * i) < VW ? x[u][i] + tb[i] : 0.f;
#pragma unroll
                for (int j = 0; j < J; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[u][i] = fmaf(wj[u][j], cj[j][i], x[u][i]);
                float pr = 0.f, pg = 0.f, pb = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float xr = fmaxf(x[u][i], 0.f);
                    if (TRAIN && s0 + u < S && lane + 64 * i < VW) hv[((size_t)rl * S + s0 + u) * VW + lane + 64 * i] = xr;
                    pr = fmaf(xr, rw[0][i], pr);
                    pg = fmaf(xr, rw[1][i], pg);
                    pb = fmaf(xr, rw[2][i], pb);
                }
                pr = wave_total(pr); pg = wave_total(pg); pb = wave_total(pb);   // DPP scan: no LDS-crossbar shuffles
                if (lane == 0 && s0 + u < S)
                    reinterpret_cast<float4*>(raw_out)[(size_t)ray * S + s0 + u] = make_float4(pr + rb0, pg + rb1, pb + rb2, al[u]);
            }
        }
    }
}

}  // namespace danbo
