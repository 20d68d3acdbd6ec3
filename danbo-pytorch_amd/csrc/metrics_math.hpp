// Per-pixel arithmetic, tile shape and summation trees of the image metrics (PSNR / SSIM of rendered frames; what
// core/utils/evaluation_helpers.py evaluate_in_boxes / evaluate_metric compute with ssim_map on the host).
//
// Like raster_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels (k_metrics.hip) and compiled by g++ for
// the serial restatement at the end of this file (image_metrics_host), which the CPU tests check against float64 and the GPU tests
// compare the kernels with, bit for bit.  -ffp-contract=off, and every product, sum, difference and quotient below is one fp32
// rounding (mul_rn / add_rn / sub_rn / div_rn).  Definitions (tests/test_image_metrics_host.py relies on them):
//   * layout: pred, gt, ssim_map [N,H,W,3], masks [N,H,W]; x = pred, y = gt.
//   * box of image n: boxes[4 n ..] = x0, y0, x1, y1, half open, each clamped to [0, W] / [0, H] (a negative corner is 0: not
//     numpy's from-the-end); no boxes: the whole image; x1 <= x0 or y1 <= y0: empty.  Everything below is OF THE CROP: a pixel
//     outside the box reads as +0 wherever a window reaches it, which is the zero padding of the cropped image.
//   * local moments of a channel: the five fields x, y, x x, y y, x y (products rounded), filtered first over H, then over W (the
//     order of _blur), each pass acc = +0; acc = acc + w[t] * f[t] for t = 0 .. win - 1 in that order; the tap t of the pixel at
//     row r reads row r + t - win / 2.
//   * ssim = ((2 mu1) mu2 + C1) / (mu1 mu1 + mu2 mu2 + C1) * ((2 s12 + C2) / (s1 + s2 + C2)), s1 = E[xx] - mu1 mu1, s2 = E[yy] -
//     mu2 mu2, s12 = E[xy] - mu1 mu2, C1 = 1e-4f, C2 = 9e-4f (K = (0.01, 0.03), unit data range), in the grouping of ssim_map.
//   * se = (y - x)^2.
//   * the 8 numbers of a pixel, each acc = +0; acc = acc + v_c for c = 0, 1, 2:  0: se_c   1: ssim_c   2: se_c a   3: ssim_c a
//     5: se_c b   6: ssim_c b, and 4: a, 7: b themselves (a, b: the pixel's weights in mask_a / mask_b; without the mask all of
//     its three numbers are +0).  A pixel outside the box has eight +0.
//   * tile: METRICS_TILE_H x METRICS_TILE_W pixels, anchored at the image's origin; pixel (ly, lx) of it is leaf ly * TILE_W + lx
//     of the tile's tree.  metrics_tree is the one tree: for s = n / 2, n / 4, .., 1: u[i] = u[i] + u[i + s] for i < s.  n is a power
//     of two: the tile's METRICS_TILE_PIX leaves, then per image the tile partials in row-major tile order, padded with +0 to
//     metrics_pad_tiles() leaves.  No atomics: the same bits on every call, and the serial code below gives the kernel's bits.
#pragma once
#include <stddef.h>
#include "sample_math.hpp"

namespace danbo {

constexpr int METRICS_MAX_DIM = 4096;            // height, width: 1 .. 4096
constexpr int METRICS_MAX_WIN = 15;              // window: odd, 1 .. 15
constexpr int METRICS_TILE_W = 32, METRICS_TILE_H = 16;
constexpr int METRICS_TILE_PIX = METRICS_TILE_W * METRICS_TILE_H;
constexpr int METRICS_SUMS = 8;                  // numbers per pixel / tile / image
constexpr float METRICS_C1 = 1e-4f, METRICS_C2 = 9e-4f;

DANBO_HD int metrics_tiles_x(int width) { return (width + METRICS_TILE_W - 1) / METRICS_TILE_W; }
DANBO_HD int metrics_tiles_y(int height) { return (height + METRICS_TILE_H - 1) / METRICS_TILE_H; }
// leaves of an image's tree: the tile count rounded up to a power of two
DANBO_HD int metrics_pad_tiles(int height, int width) {
    const int t = metrics_tiles_x(width) * metrics_tiles_y(height);
    int p = 1;
    while (p < t) p <<= 1;
    return p;
}
DANBO_HD bool metrics_size_ok(long n_images, int height, int width) {
    if (n_images < 0 || height < 1 || height > METRICS_MAX_DIM || width < 1 || width > METRICS_MAX_DIM) return false;
    return n_images * metrics_tiles_x(width) * metrics_tiles_y(height) <= 0x7fffffffL;      // one workgroup per tile in one grid
}
// bytes of the workspace: [N][METRICS_SUMS][metrics_pad_tiles] floats; 0 for a rejected size
DANBO_HD size_t metrics_workspace_size(int n_images, int height, int width) {
    if (!metrics_size_ok(n_images, height, width)) return 0;
    const size_t n = n_images > 0 ? (size_t)n_images : 1;      // (never 0 for an accepted size: 0 says "rejected")
    return n * METRICS_SUMS * (size_t)metrics_pad_tiles(height, width) * sizeof(float);
}
DANBO_HD bool metrics_win_ok(int win) { return win >= 1 && win <= METRICS_MAX_WIN && (win & 1) == 1; }

struct MetricsBox {
    int x0, y0, x1, y1;
};
DANBO_HD int metrics_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
DANBO_HD MetricsBox metrics_box(const int32_t* boxes, int n, int height, int width) {
    MetricsBox b = {0, 0, width, height};
    if (boxes != nullptr) {
        b.x0 = metrics_clamp(boxes[4 * n], width), b.y0 = metrics_clamp(boxes[4 * n + 1], height);
        b.x1 = metrics_clamp(boxes[4 * n + 2], width), b.y1 = metrics_clamp(boxes[4 * n + 3], height);
    }
    return b;
}
DANBO_HD bool metrics_in_box(const MetricsBox& b, int y, int x) { return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1; }

// one filter pass over `win` samples `stride` floats apart
DANBO_HD float metrics_filter(const float* f, int stride, const float* w, int win) {
    float acc = 0.f;
    for (int t = 0; t < win; ++t) acc = add_rn(acc, mul_rn(w[t], f[t * stride]));
    return acc;
}
// the H pass of the five fields from the x and y samples of one column (`stride` floats between rows)
DANBO_HD void metrics_pass_h(const float* x, const float* y, int stride, const float* w, int win, float* out5) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
    for (int t = 0; t < win; ++t) {
        const float xv = x[t * stride], yv = y[t * stride], wt = w[t];
        a0 = add_rn(a0, mul_rn(wt, xv));
        a1 = add_rn(a1, mul_rn(wt, yv));
        a2 = add_rn(a2, mul_rn(wt, mul_rn(xv, xv)));
        a3 = add_rn(a3, mul_rn(wt, mul_rn(yv, yv)));
        a4 = add_rn(a4, mul_rn(wt, mul_rn(xv, yv)));
    }
    out5[0] = a0, out5[1] = a1, out5[2] = a2, out5[3] = a3, out5[4] = a4;
}
DANBO_HD float metrics_ssim(float mu1, float mu2, float exx, float eyy, float exy) {
    const float m11 = mul_rn(mu1, mu1), m22 = mul_rn(mu2, mu2), m12 = mul_rn(mu1, mu2);
    const float s1 = sub_rn(exx, m11), s2 = sub_rn(eyy, m22), s12 = sub_rn(exy, m12);
    const float cs = div_rn(add_rn(mul_rn(2.f, s12), METRICS_C2), add_rn(add_rn(s1, s2), METRICS_C2));
    const float l = div_rn(add_rn(mul_rn(mul_rn(2.f, mu1), mu2), METRICS_C1), add_rn(add_rn(m11, m22), METRICS_C1));
    return mul_rn(l, cs);
}
DANBO_HD float metrics_sqerr(float x, float y) {
    const float d = sub_rn(y, x);
    return mul_rn(d, d);
}
// adds channel c's se and ssim to the pixel's eight numbers (v[4], v[7] hold a, b: set by the caller)
DANBO_HD void metrics_add_channel(float se, float ss, bool has_a, float a, bool has_b, float b, float* v) {
    v[0] = add_rn(v[0], se), v[1] = add_rn(v[1], ss);
    if (has_a) v[2] = add_rn(v[2], mul_rn(se, a)), v[3] = add_rn(v[3], mul_rn(ss, a));
    if (has_b) v[5] = add_rn(v[5], mul_rn(se, b)), v[6] = add_rn(v[6], mul_rn(ss, b));
}

// THE tree, for nq arrays of n = 2^k leaves `qstride` floats apart, walked by `nthreads` cooperating threads (serial: tid 0 of 1,
// sync a no-op); the sum of array q ends in u[q * qstride]
template <class Sync>
DANBO_HD void metrics_tree(float* u, int n, int nq, size_t qstride, int tid, int nthreads, Sync sync) {
    int ls = 0;
    while ((2 << ls) <= n) ++ls;                               // n = 2^ls leaves, 2^(ls-1) sums at the first level
    for (--ls; ls >= 0; --ls) {
        const int s = 1 << ls;
        for (int idx = tid; idx < nq * s; idx += nthreads) {   // (nq * s < 2^31: at most 8 * 2^14)
            float* p = u + (size_t)(idx >> ls) * qstride + (idx & (s - 1));
            p[0] = add_rn(p[0], p[s]);
        }
        sync();
    }
}

// the argument checks of danbo_image_metrics, shared with the serial code
DANBO_HD bool metrics_args_ok(const void* pred, const void* gt, int n_images, int height, int width, const void* window, int win,
                              const void* workspace, const void* sums, const void* ssim_map) {
    if (pred == nullptr || gt == nullptr || window == nullptr || workspace == nullptr || sums == nullptr) return false;
    if (!metrics_size_ok(n_images, height, width) || !metrics_win_ok(win)) return false;
    return (((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)ssim_map) & 15) == 0 && ((uintptr_t)workspace & 3) == 0;
}

// ------------------------------------------------------------------------------------------------ serial restatement
// danbo_image_metrics on host memory, tile by tile in the kernel's order; returns 0 or -22 (DANBO_EINVAL) as the C entry does.
inline int image_metrics_host(const float* pred, const float* gt, const float* mask_a, const float* mask_b, const int32_t* boxes,
                              int n_images, int height, int width, const float* window, int win, void* workspace, float* sums,
                              float* ssim_map) {
    if (!metrics_args_ok(pred, gt, n_images, height, width, window, win, workspace, sums, ssim_map)) return -22;
    const int H = height, W = width, half = win / 2, TX = metrics_tiles_x(W), TY = metrics_tiles_y(H), P = metrics_pad_tiles(H, W);
    float* ws = static_cast<float*>(workspace);
    const auto no_sync = [] {};
    for (int n = 0; n < n_images; ++n) {
        const MetricsBox box = metrics_box(boxes, n, H, W);
        const size_t img = (size_t)n * H * W;
        float* part = ws + (size_t)n * METRICS_SUMS * P;
        for (int tile = 0; tile < TX * TY; ++tile) {
            const int ty0 = (tile / TX) * METRICS_TILE_H, tx0 = (tile % TX) * METRICS_TILE_W;
            float leaf[METRICS_SUMS * METRICS_TILE_PIX];
            for (int i = 0; i < METRICS_TILE_PIX; ++i) {
                const int Y = ty0 + i / METRICS_TILE_W, X = tx0 + i % METRICS_TILE_W;
                float v[METRICS_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (metrics_in_box(box, Y, X)) {
                    const float a = mask_a ? mask_a[img + (size_t)Y * W + X] : 0.f, b = mask_b ? mask_b[img + (size_t)Y * W + X] : 0.f;
                    v[4] = a, v[7] = b;
                    for (int c = 0; c < 3; ++c) {
                        float hp[5][METRICS_MAX_WIN];             // the H pass at the win columns the W pass reads
                        for (int t = 0; t < win; ++t) {
                            float xs[METRICS_MAX_WIN], ys[METRICS_MAX_WIN], o[5];
                            for (int r = 0; r < win; ++r) {
                                const int yy = Y + r - half, xx = X + t - half;
                                const bool in = metrics_in_box(box, yy, xx);
                                xs[r] = in ? pred[(img + (size_t)yy * W + xx) * 3 + c] : 0.f;
                                ys[r] = in ? gt[(img + (size_t)yy * W + xx) * 3 + c] : 0.f;
                            }
                            metrics_pass_h(xs, ys, 1, window, win, o);
                            for (int k = 0; k < 5; ++k) hp[k][t] = o[k];
                        }
                        float m[5];
                        for (int k = 0; k < 5; ++k) m[k] = metrics_filter(hp[k], 1, window, win);
                        const float ss = metrics_ssim(m[0], m[1], m[2], m[3], m[4]);
                        const float se = metrics_sqerr(pred[(img + (size_t)Y * W + X) * 3 + c], gt[(img + (size_t)Y * W + X) * 3 + c]);
                        metrics_add_channel(se, ss, mask_a != nullptr, a, mask_b != nullptr, b, v);
                        if (ssim_map) ssim_map[(img + (size_t)Y * W + X) * 3 + c] = ss;
                    }
                }
                for (int q = 0; q < METRICS_SUMS; ++q) leaf[q * METRICS_TILE_PIX + i] = v[q];
            }
            metrics_tree(leaf, METRICS_TILE_PIX, METRICS_SUMS, METRICS_TILE_PIX, 0, 1, no_sync);
            for (int q = 0; q < METRICS_SUMS; ++q) part[(size_t)q * P + tile] = leaf[q * METRICS_TILE_PIX];
        }
        for (int q = 0; q < METRICS_SUMS; ++q)
            for (int t = TX * TY; t < P; ++t) part[(size_t)q * P + t] = 0.f;
        metrics_tree(part, P, METRICS_SUMS, (size_t)P, 0, 1, no_sync);
        for (int q = 0; q < METRICS_SUMS; ++q) sums[(size_t)n * METRICS_SUMS + q] = part[(size_t)q * P];
    }
    return 0;
}

}  // namespace danbo
