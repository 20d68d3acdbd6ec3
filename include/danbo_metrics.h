/*
 * libdanbo_hip.so -- C ABI of the image metrics: squared error and SSIM of rendered frames against the ground truth, summed per
 * image inside a box and under up to two masks, without the frames leaving the device (csrc/k_metrics.hip; what
 * core/utils/evaluation_helpers.py evaluate_in_boxes / evaluate_metric compute on the host, which stay the statement of WHAT is
 * computed).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  They stand in a header of their own, like the rasteriser's (danbo_raster.h) and
 * the part maps' (danbo_partmap.h), because danbo_hip.h is the pinned statement of the render and training path
 * (tests/test_abi_binding.py counts its entry points).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_metrics.h");
 * tests/test_abi_binding.py checks what the parser derived against the host compiler's view of this file.
 */
#ifndef DANBO_METRICS_H
#define DANBO_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * danbo_image_metrics: pred, gt [N,H,W,3] float (channels last, as render_path stacks its frames), mask_a / mask_b [N,H,W] float
 * weights (each nullable), boxes [N,4] int32 x0, y0, x1, y1 (nullable: the whole image).
 *
 * Box: half open, rows y0 .. y1 - 1 and columns x0 .. x1 - 1, the [tl[1]:br[1], tl[0]:br[0]] slice of evaluate_in_boxes; each
 * corner is clamped to the image (a negative one to 0), so a box may over-reach; x1 <= x0 or y1 <= y0 is empty.  Box data is
 * device memory: the host cannot and does not validate it.
 * SSIM is computed OF THE CROP: a window tap outside the box reads +0, not the neighbouring pixel -- cropping and then zero
 * padding, as evaluate_in_boxes does; with the whole-image box it is ssim_map's zero padding.  Formula (ssim_map): the five
 * fields x, y, x x, y y, x y (x = pred, y = gt) are filtered with `window` ([win] floats in DEVICE memory: the caller's _gauss(),
 * so that host and device agree on the weights by construction -- nothing evaluates exp here; win odd, 1 .. 15) first over H, then
 * over W (the order of _blur), taps accumulated from tap 0 to tap win - 1 into a sum that starts at +0, product and sum rounded
 * separately (the library is built with -ffp-contract=off); then
 *   ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * ((2 s12 + C2) / (s1 + s2 + C2)),  C1 = 1e-4, C2 = 9e-4 (unit data range),
 * and se = (gt - pred)^2, per pixel and channel.
 *
 * sums[i] = { S se, S ssim,  S se a, S ssim a, S a,  S se b, S ssim b, S b } over the pixels of image i's box: the first two
 * over all 3 channels; a = mask_a, b = mask_b as float weights multiplied into each channel's value, S a and S b over pixels (not
 * times 3); the three slots of a NULL mask are +0.  Pixel counts are integers the host knows ((x1 - x0)(y1 - y0) of the clamped
 * box) and are not summed in float.  An empty box gives eight +0.
 * ssim_map (nullable) [N,H,W,3]: the per-pixel, per-channel SSIM inside the box; pixels outside the box are NOT touched.
 *
 * Summation order, fixed (csrc/metrics_math.hpp states it once, for the kernel and for the serial restatement
 * image_metrics_host that the tests compare the kernel with bit for bit): per pixel each of the eight numbers adds its channels
 * 0, 1, 2 to +0; the image is cut into tiles of 16 rows x 32 columns anchored at its origin, pixel (ly, lx) of a tile being leaf
 * 32 ly + lx of 512 (a pixel outside the box or the image: +0); the tree over n = 2^k leaves is
 *   for s = n / 2, n / 4, .., 1:  u[i] = u[i] + u[i + s]  for every i < s,
 * once per tile, then once per image over the tile partials in row-major tile order padded with +0 to a power of two.  The
 * partials live in `workspace`; a second small launch reduces them.  No float atomics: every call gives the same bits.
 *
 * workspace: danbo_image_metrics_workspace_bytes(n_images, height, width) bytes of device memory, 4-byte aligned; its contents
 * before the call do not matter.  The size is 0 for a size the call rejects.
 * DANBO_EINVAL before any launch (and a workspace size of 0 for the size checks): a null pred, gt, window, workspace or sums;
 * n_images < 0; height or width outside 1 .. 4096; more than 2^31 - 1 tiles in all; an even win or one outside 1 .. 15; a pred,
 * gt or ssim_map that is not 16-byte aligned; a workspace that is not 4-byte aligned.  n_images == 0 returns 0 with nothing
 * launched. */
size_t danbo_image_metrics_workspace_bytes(int n_images, int height, int width);
int danbo_image_metrics(const float* pred /*[N,H,W,3]*/, const float* gt /*[N,H,W,3]*/, const float* mask_a /*[N,H,W] or NULL*/,
                        const float* mask_b /*[N,H,W] or NULL*/, const int32_t* boxes /*[N,4] x0,y0,x1,y1 or NULL*/, int n_images,
                        int height, int width, const float* window /*[win]*/, int win, void* workspace, float* sums /*[N,8]*/,
                        float* ssim_map /*[N,H,W,3] or NULL*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
