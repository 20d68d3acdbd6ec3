// Per-ray arithmetic and row copies of the training-batch gather (danbo_batch.h; what core/load_data.py
// PoseImageDataset.sample_batch computes in numpy from the images and pixels it drew, which stays the statement of WHAT is computed).
//
// Like metrics_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernel (k_batch.hip) and compiled by g++ for the
// serial restatement at the end of this file (batch_gather_host), which the CPU tests compare with the numpy path and the GPU tests
// compare the kernel with, bit for bit.  -ffp-contract=off, and every product, sum, difference and quotient below is one fp32
// rounding (mul_rn / add_rn / sub_rn / div_rn).  Definitions (tests/test_batch_host.py relies on them):
//   * ray r of a batch of G picks x `per` pixels belongs to pick r / per; its image is i = clamp(picks[r / per], 0, N - 1), its pixel
//     pix = clamp(pixels[r], 0, H W - 1), its background b = clamp(bg_idxs[i], 0, B - 1).  The clamps stand before any address
//     is formed: picks, pixels and bg_idxs are device memory that the C side cannot validate.
//   * the ray (PoseImageDataset._rays): x = float(pix % W), y = float(pix / W); (cx, cy) = (W * 0.5f, H * 0.5f) or centers[i];
//     dirs = ((x - cx) / f, (-(y - cy)) / f, -1), f = focals[i];  rays_d[j] = (dirs0 R[j][0] + dirs1 R[j][1]) + dirs2 R[j][2] and
//     rays_o[j] = c2w[j][3] with R = c2ws[i][:3,:3] (numpy's sum over an axis of three: the first two, then the third; it starts
//     from +0, which shows only in the sign of a zero: three products of -0 sum to +0).
//   * the colours, per channel, fg = fgs[i][pix]:  bg = bgs[b][pix];  with noise: bg = (1 - fg) noise[r] + fg bg;  target =
//     imgs[i][pix];  with mask_image: target = target fg + (1 - fg) bg.  fg itself is copied.
//   * the pose rows kp3d [24,3], bones [24,3], skts [24,4,4], cyls [5] of image i are copied to ray r's rows, words unchanged.
//   * cam_idxs[r] = cam_idxs[i], kp_idx[r] = i, both widened to 64 bits.
#pragma once
#include <stddef.h>
#include "sample_math.hpp"

namespace danbo {

constexpr int BATCH_KP_ROW = J * 3, BATCH_BONE_ROW = J * 3, BATCH_SKT_ROW = J * 16, BATCH_CYL_ROW = 5;    // floats per pose row
constexpr int BATCH_RAYS_PER_GROUP = 8;          // rays whose pose rows one workgroup writes
constexpr int BATCH_BLOCK = 256;                 // threads of a workgroup; rays of one per-ray workgroup

// the resident tables, this batch's draws and the eleven outputs: the arguments of danbo_batch_gather, as the kernel gets them
struct BatchTables {
    const float *imgs, *fgs, *bgs;
    const int32_t *bg_idxs, *cam_idxs;
    const float *c2ws, *focals, *centers, *kp3d, *bones, *skts, *cyls;
    int N, B, H, W;
};
struct BatchDraw {
    const int32_t *picks, *pixels;
    const float* noise;
    int G, per, mask_image;
};
struct BatchOut {
    float *rays_o, *rays_d, *target, *fgs, *bgs, *kp3d, *bones, *skts, *cyls;
    long long *cam_idxs, *kp_idx;
};

DANBO_HD int batch_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// the image of ray r
DANBO_HD int batch_image_of(const BatchTables& t, const BatchDraw& d, long r) { return batch_clamp(d.picks[r / d.per], t.N); }

// pinhole ray of flat pixel `pix` of a W-wide image through c2w [4,4] (row-major), focal f, principal point (cx, cy)
DANBO_HD void batch_ray(const float* c2w, float f, float cx, float cy, int pix, int W, float* o, float* d) {
    const float x = (float)(pix % W), y = (float)(pix / W);
    const float d0 = div_rn(sub_rn(x, cx), f), d1 = div_rn(-sub_rn(y, cy), f), d2 = -1.f;
    for (int j = 0; j < 3; ++j) {
        const float* R = c2w + 4 * j;
        d[j] = add_rn(add_rn(add_rn(0.f, mul_rn(d0, R[0])), mul_rn(d1, R[1])), mul_rn(d2, R[2]));
        o[j] = R[3];
    }
}
// one channel of the background a ray is trained against: random outside the mask if there is noise (perturb_bg)
DANBO_HD float batch_bg(float bg, float fg, const float* noise) {
    return noise == nullptr ? bg : add_rn(mul_rn(sub_rn(1.f, fg), *noise), mul_rn(fg, bg));
}
// one channel of the target: composited over that background outside the mask (mask_image)
DANBO_HD float batch_target(float img, float fg, float bg, int mask_image) {
    return mask_image ? add_rn(mul_rn(img, fg), mul_rn(sub_rn(1.f, fg), bg)) : img;
}

// everything of ray r that is not a pose row
DANBO_HD void batch_ray_values(const BatchTables& t, const BatchDraw& d, const BatchOut& out, long r) {
    const int i = batch_image_of(t, d, r);
    const int HW = t.H * t.W, pix = batch_clamp(d.pixels[r], HW), b = batch_clamp(t.bg_idxs[i], t.B);
    const float cx = t.centers ? t.centers[2 * (size_t)i] : mul_rn((float)t.W, 0.5f);
    const float cy = t.centers ? t.centers[2 * (size_t)i + 1] : mul_rn((float)t.H, 0.5f);
    float o[3], dir[3];
    batch_ray(t.c2ws + 16 * (size_t)i, t.focals[i], cx, cy, pix, t.W, o, dir);
    const size_t at = (size_t)i * HW + pix, bat = (size_t)b * HW + pix;
    const float fg = t.fgs[at];
    for (int c = 0; c < 3; ++c) {
        const float bg = batch_bg(t.bgs[3 * bat + c], fg, d.noise ? d.noise + 3 * (size_t)r + c : nullptr);
        out.rays_o[3 * (size_t)r + c] = o[c];
        out.rays_d[3 * (size_t)r + c] = dir[c];
        out.target[3 * (size_t)r + c] = batch_target(t.imgs[3 * at + c], fg, bg, d.mask_image);
        out.bgs[3 * (size_t)r + c] = bg;
    }
    out.fgs[r] = fg;
    out.cam_idxs[r] = (long long)t.cam_idxs[i];
    out.kp_idx[r] = (long long)i;
}

// rows [r0, r1) of one per-ray output := the rows of the rays' images in `table`, `row` floats each, moved as values of type V
// (float, or a 16-byte tuple where `row` and both addresses allow it) by `nthreads` cooperating threads (serial: tid 0 of 1).
// Consecutive threads take consecutive V of a row, then the next ray's row.
template <class V>
DANBO_HD void batch_copy_rows(const float* table, float* dst, int row, const BatchTables& t, const BatchDraw& d, long r0, long r1,
                              int tid, int nthreads) {
    const int w = row / (int)(sizeof(V) / sizeof(float));
    for (long idx = tid; idx < (r1 - r0) * w; idx += nthreads) {
        const long r = r0 + idx / w;
        const int q = (int)(idx % w);
        reinterpret_cast<V*>(dst + (size_t)r * row)[q] =
            reinterpret_cast<const V*>(table + (size_t)batch_image_of(t, d, r) * row)[q];
    }
}
// the four pose rows of rays [r0, r1); V as above for the three tables whose rows are whole 16-byte tuples, cyls word by word
template <class V>
DANBO_HD void batch_pose_rows(const BatchTables& t, const BatchDraw& d, const BatchOut& out, long r0, long r1, int tid, int nthreads) {
    batch_copy_rows<V>(t.skts, out.skts, BATCH_SKT_ROW, t, d, r0, r1, tid, nthreads);
    batch_copy_rows<V>(t.kp3d, out.kp3d, BATCH_KP_ROW, t, d, r0, r1, tid, nthreads);
    batch_copy_rows<V>(t.bones, out.bones, BATCH_BONE_ROW, t, d, r0, r1, tid, nthreads);
    batch_copy_rows<float>(t.cyls, out.cyls, BATCH_CYL_ROW, t, d, r0, r1, tid, nthreads);
}

// the argument checks of danbo_batch_gather, shared with the serial code
DANBO_HD bool batch_args_ok(const BatchTables& t, const BatchDraw& d, const BatchOut& out) {
    if (!t.imgs || !t.fgs || !t.bgs || !t.bg_idxs || !t.cam_idxs || !t.c2ws || !t.focals || !t.kp3d || !t.bones || !t.skts || !t.cyls)
        return false;                                                      // (centers and noise may be null)
    if (!d.picks || !d.pixels) return false;
    if (!out.rays_o || !out.rays_d || !out.target || !out.fgs || !out.bgs || !out.kp3d || !out.bones || !out.skts || !out.cyls ||
        !out.cam_idxs || !out.kp_idx)
        return false;
    if (t.N < 1 || t.B < 1 || t.H < 1 || t.W < 1 || d.per < 1 || d.G < 0) return false;
    return (long long)t.H * t.W <= 0x7fffffffLL && (long long)d.G * d.per <= 0x7fffffffLL;
}

// ------------------------------------------------------------------------------------------------ serial restatement
// danbo_batch_gather on host memory, ray by ray; returns 0 or -22 (DANBO_EINVAL) as the C entry does.
inline int batch_gather_host(const BatchTables& t, const BatchDraw& d, const BatchOut& out) {
    if (!batch_args_ok(t, d, out)) return -22;
    const long R = (long)d.G * d.per;
    for (long r = 0; r < R; ++r) batch_ray_values(t, d, out, r);
    batch_pose_rows<float>(t, d, out, 0, R, 0, 1);
    return 0;
}

}  // namespace danbo
