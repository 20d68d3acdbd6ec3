/*
 * libdanbo_hip.so -- C ABI of the training-batch gather: the eleven tensors of one ray batch (rays, targets, masks, backgrounds and
 * the per-ray pose rows) from image and pose tables that were uploaded once and the images and pixels the host drew for this step
 * (csrc/k_batch.hip; what core/load_data.py PoseImageDataset.sample_batch computes in numpy, which stays the statement of WHAT is
 * computed).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entry is additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_batch.h").
 */
#ifndef DANBO_BATCH_H
#define DANBO_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * danbo_batch_gather: R = n_picks * per rays; ray r belongs to pick r / per.
 *
 * The resident tables of n_images images of height x width pixels and n_bgs backgrounds: imgs [N,H,W,3], fgs [N,H,W], bgs [B,H,W,3]
 * float; bg_idxs, cam_idxs [N] int32; c2ws [N,4,4] (row-major camera-to-world), focals [N], centers [N,2] (cx, cy; NULL: the middle
 * of the image, width / 2 and height / 2); kp3d [N,24,3], bones [N,24,3], skts [N,24,4,4], cyls [N,5].
 * This batch: picks [n_picks] int32 image indices, pixels [R] int32 flat pixel indices y * width + x, noise [R,3] float (NULL: the
 * backgrounds as stored), mask_image (0: the targets as stored; otherwise composited over the background outside the mask).
 *
 * picks, pixels and bg_idxs are device memory: the host cannot and does not validate them.  Each is clamped before any address is
 * formed -- the image i = clamp(picks[r / per], 0, N - 1), the pixel pix = clamp(pixels[r], 0, H W - 1), the background
 * b = clamp(bg_idxs[i], 0, B - 1) -- so no content of theirs makes the kernel read or write outside the tables and outputs.
 *
 * Per ray (csrc/batch_math.hpp states each formula once, for the kernel and for the serial restatement batch_gather_host that the
 * tests compare the kernel with bit for bit; every product, sum, difference and quotient is one fp32 rounding, the library is built
 * with -ffp-contract=off and the division is correctly rounded):
 *   x = float(pix % W), y = float(pix / W);  dirs = ((x - cx) / f, (-(y - cy)) / f, -1),  f = focals[i]
 *   out_rays_d[r][j] = ((+0 + dirs0 R[j][0]) + dirs1 R[j][1]) + dirs2 R[j][2],  out_rays_o[r][j] = c2ws[i][j][3],  R = c2ws[i][:3,:3]
 *   (the +0 is numpy's start of a sum; it shows only in the sign of a zero result)
 *   fg = fgs[i][pix];  bg = bgs[b][pix], with noise: bg = (1 - fg) noise[r] + fg bg;  target = imgs[i][pix], with mask_image:
 *   target = target fg + (1 - fg) bg;  out_fgs[r] = fg, out_bgs[r] = bg, out_target[r] = target
 *   out_kp3d[r], out_bones[r], out_skts[r], out_cyls[r] = row i of kp3d, bones, skts, cyls, words unchanged
 *   out_cam_idxs[r] = cam_idxs[i], out_kp_idx[r] = i, as 64-bit integers
 * Outputs: out_rays_o, out_rays_d, out_target, out_bgs [R,3], out_fgs [R,1], out_kp3d, out_bones [R,24,3], out_skts [R,24,4,4],
 * out_cyls [R,5] float; out_cam_idxs, out_kp_idx [R] 64-bit.  One launch, no atomics, no workspace: every call gives the same bits.
 * The pose rows move 16 bytes a lane when skts, kp3d, bones and their three outputs are all 16-byte aligned, 4 bytes otherwise.
 *
 * DANBO_EINVAL before any launch: a null pointer other than centers and noise; n_images, n_bgs, height, width or per below 1;
 * n_picks < 0; height * width or n_picks * per above 2^31 - 1.  n_picks == 0 returns 0 with nothing launched. */
int danbo_batch_gather(const float* imgs /*[N,H,W,3]*/, const float* fgs /*[N,H,W]*/, const float* bgs /*[B,H,W,3]*/,
                       const int32_t* bg_idxs /*[N]*/, const int32_t* cam_idxs /*[N]*/, const float* c2ws /*[N,4,4]*/,
                       const float* focals /*[N]*/, const float* centers /*[N,2] or NULL*/, const float* kp3d /*[N,24,3]*/,
                       const float* bones /*[N,24,3]*/, const float* skts /*[N,24,4,4]*/, const float* cyls /*[N,5]*/, int n_images,
                       int n_bgs, int height, int width, const int32_t* picks /*[G]*/, const int32_t* pixels /*[G*per]*/,
                       const float* noise /*[G*per,3] or NULL*/, int n_picks, int per, int mask_image, float* out_rays_o /*[R,3]*/,
                       float* out_rays_d /*[R,3]*/, float* out_target /*[R,3]*/, float* out_fgs /*[R,1]*/, float* out_bgs /*[R,3]*/,
                       float* out_kp3d /*[R,24,3]*/, float* out_bones /*[R,24,3]*/, float* out_skts /*[R,24,4,4]*/,
                       float* out_cyls /*[R,5]*/, long long* out_cam_idxs /*[R]*/, long long* out_kp_idx /*[R]*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
