/*
 * libdanbo_hip.so -- C ABI of the bone-assignment maps (--render_confd / --render_entropy): the colour of every sample from its
 * 24 assignment logits, and the composite of those colours with the weights of the ordinary render (csrc/k_partmap.hip).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  They stand in a header of their own, like the rasteriser's (danbo_raster.h),
 * because danbo_hip.h is the pinned statement of the render and training path (tests/test_abi_binding.py counts its entry points).
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_partmap.h");
 * tests/test_abi_binding.py checks what the parser derived against the host compiler's view of this file.
 */
#ifndef DANBO_PARTMAP_H
#define DANBO_PARTMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * raw2outputs with render_confd / render_entropy (core/networks/nerf.py:306-313) -- the colour of a sample is a function of its 24 assignment logits and replaces
 * sigmoid(raw[..., :3]); the weights are those of the ordinary render, which these two calls only read.
 *
 * danbo_part_colors_fwd: row i of confd belongs to sample m = list ? list[i] : i (the convention of K2 / K3, whose confd rows
 * these are) and its colour goes to rgb[m]; rows i >= *count (device count, NULL: n) and samples that are not listed are not
 * touched.  mode 0 (get_confidence_rgb, core/networks/misc.py:620-640): palette[argmax_j confd[i, j]], the lowest index on a tie
 * as torch.argmax; palette: the 24 joint colours, [24,3] in device memory (required for mode 0 only).  mode 1 (get_entropy_rgb,
 * :642-673): lerp((0,0,1), (1,0,0), H / ln 24) with H = -sum_j p_j log(p_j + 1e-7), p = softmax(confd[i]); accurate exp / log: within
 * 1e-5 of the float64 value.  valid_only != 0 (the masked form the reference sketches in get_entropy_rgb's commented-out block):
 * bones whose bit of valid_bits[m] (indexed by SAMPLE, as danbo_bone_cull writes it) is clear are left out of the argmax / the
 * softmax, the entropy stays relative to ln 24, and a sample inside no volume gets colour 0; valid_bits is required only then.
 * DANBO_EINVAL before any launch: mode other than 0 / 1, n < 0, valid_only without valid_bits, mode 0 without palette, a null or
 * not 16-byte aligned confd, a null rgb. */
int danbo_part_colors_fwd(const float* confd /*[n,24]*/, const uint32_t* valid_bits, const int32_t* list, const int32_t* count, int n,
                          int mode, int valid_only, const float* palette /*[24,3]*/, float* rgb /*[M,3]*/, void* stream);
/* danbo_composite_colors_fwd: rgb_map[r] = sum_k weights[r, k] * colour(r, k) over the S + Sf positions of the sorted order, one
 * wavefront per ray.  Position k reads rgb_a[r, sorted_idx[r, k]] (sorted_idx < S) or rgb_b[r, sorted_idx - S]; sorted_idx ==
 * NULL (then rgb_b == NULL, Sf = 0): the identity -- the coarse map, and the final map of a caster with a separate fine network,
 * whose S + Sf samples arrive sorted in rgb_a.  bits_a / bits_b (each nullable: every row written): a sample whose in-volume word
 * is 0 has no colour row, is NOT read and contributes nothing.  A sample of weight 0 contributes +0 and is not read either.
 * ray_list / ray_count (optional, together; as danbo_composite_merged_fwd): only the listed rays are written -- the rows of the
 * rays of constants were set to +0 by danbo_flat_rays, which is their map, all their weights being +0.
 * Summation order, fixed: lane l of the wavefront adds the products of positions l, l + 64, ... in that order (product and sum
 * rounded separately), then the 64 partial sums go through one fixed tree: the same bits on every call, no atomics.
 * Limits: S <= 256 and Sf <= 64 as the unfused composites (identity form: S <= 320); anything else, or only one of ray_list /
 * ray_count, is DANBO_EINVAL before any launch. */
int danbo_composite_colors_fwd(const float* rgb_a /*[R,S,3]*/, const float* rgb_b /*[R,Sf,3] or NULL*/, const uint32_t* bits_a,
                               const uint32_t* bits_b, const int32_t* sorted_idx /*[R,S+Sf] or NULL*/,
                               const float* weights /*[R,S+Sf]*/, int R, int S, int Sf, const int32_t* ray_list,
                               const int32_t* ray_count, float* rgb_map /*[R,3]*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
