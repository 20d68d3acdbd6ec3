/*
 * libdanbo_hip.so -- C ABI of K1a over the listed rays of a frame: depths, in-volume words and the compacted row list for the rays
 * danbo_flat_rays lists and for no other ray (csrc/k_cull_rays.hip), in place of danbo_coarse_samples + danbo_bone_cull over every
 * ray.  danbo_render_frame and DanboEngine.render use it when the frame has rays of constants and one pose.
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, the kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entry is additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  It stands in a header of its own, like the rasteriser's (danbo_raster.h), the part
 * maps' (danbo_partmap.h) and the metrics' (danbo_metrics.h), because danbo_hip.h is the pinned statement of the entry points it
 * has (tests/test_abi_binding.py counts them).  This header declares no struct and no constant.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_cull.h").
 */
#ifndef DANBO_CULL_H
#define DANBO_CULL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* danbo_bone_cull_rays: what danbo_coarse_samples + danbo_bone_cull make, for the rays of a list and for
 * no other ray.  For a frame whose rays of constants have their outputs from danbo_flat_rays: nothing downstream reads the depths
 * or the in-volume words of those rays (danbo_view_consts, the `_rays` composites and the resampling walk the same list; K2 and K3
 * reach samples through the row list made here), so none are made.  One pose (G == 1; anything else is DANBO_EINVAL).
 *   ray_list [n], ray_count [1] (device): the rays, as danbo_flat_rays lists them; n = *ray_count clamped to [0, R], every entry
 *   clamped to [0, R - 1].  ray_mask / t_lo / t_hi: danbo_ray_bone_mask's result for these rays, required; as in danbo_bone_cull a
 *   depth outside its ray's interval is tested against every bone, so the words never depend on the mask.
 *   near / far (both or neither): given, this is the COARSE pass -- the depths near (1 - t) + far t of danbo_coarse_samples
 *   (t_rand = NULL) are made here and STORED to z [R,S] for the listed rays; NULL, z [R,S] is READ (the importance depths).
 *   valid_bits [R*S]: written for every sample of a listed ray, bit for bit danbo_bone_cull's word for the same depth.
 *   list [R*S], count [1] (zeroed by the caller): the samples with a non-zero word are appended; the rows a workgroup appends are
 *   ray-major with ascending sample index, order across workgroups unspecified.  One atomic per workgroup that has a row.
 *   rays_per_wg: list entries per workgroup, 0 = the library's choice for the pass (at most 384, and at most 16384 / S; S <= 16384).
 *   Nothing is read or written for a ray that is not listed; *ray_count == 0 writes nothing at all. */
int danbo_bone_cull_rays(const int32_t* ray_list, const int32_t* ray_count, const uint32_t* ray_mask /*[R]*/,
                         const float* t_lo /*[R]*/, const float* t_hi /*[R]*/, const float* rays_o, const float* rays_d,
                         int R, int S, int G, const float* skts /*[1,24,4,4]*/, const float* align /*[24,4,4]*/,
                         const float* axis_scale /*[24,3]*/, const float* near /*[R] or NULL*/, const float* far /*[R] or NULL*/,
                         float* z /*[R,S]: out (coarse) or in*/, int rays_per_wg, uint32_t* valid_bits /*[R*S]*/,
                         int32_t* list /*[R*S]*/, int32_t* count /*[1]*/, void* stream);

#ifdef __cplusplus
}
#endif

#endif
