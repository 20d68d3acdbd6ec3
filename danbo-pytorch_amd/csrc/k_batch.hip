// The training batch on the device (danbo_batch.h): rays, targets and per-ray pose rows of the images and pixels the host drew, from
// tables uploaded once -- what core/load_data.py PoseImageDataset.sample_batch builds in numpy and copies over per step.  Every
// formula, the clamps and the copy loops are batch_math.hpp's; this file only spreads them over a grid.
#include "common.hpp"
#include "batch_math.hpp"
#include "../../include/danbo_batch.h"

namespace danbo {

static_assert(BATCH_SKT_ROW % 4 == 0 && BATCH_KP_ROW % 4 == 0 && BATCH_BONE_ROW % 4 == 0, "pose rows are whole 16-byte tuples");

// One launch, two kinds of workgroup.  The first `ray_groups` take BATCH_BLOCK rays each, one per lane: a gather of 3 + 1 + 3 floats
// and the ray's arithmetic.  Every later one streams the pose rows (533 floats a ray) of BATCH_RAYS_PER_GROUP consecutive rays:
// lanes run along a row, so a wavefront's stores cover consecutive addresses, 16 bytes a lane where V is a 4-float tuple.  The
// source rows are few (one per pick) and come from the caches after their first read.
// DANBO_NO_PK_F32 (common.hpp): the three directions' products invite packed fp32 multiplies, and this kernel may run beside the
// previous step's MFMA wavefronts.
template <class V>
__global__ __launch_bounds__(BATCH_BLOCK) DANBO_NO_PK_F32 void k_batch_gather(BatchTables t, BatchDraw d, BatchOut out, int ray_groups) {
    const long R = (long)d.G * d.per;
    if ((int)blockIdx.x < ray_groups) {
        const long r = (long)blockIdx.x * BATCH_BLOCK + threadIdx.x;
        if (r < R) batch_ray_values(t, d, out, r);
        return;
    }
    const long r0 = (long)(blockIdx.x - ray_groups) * BATCH_RAYS_PER_GROUP;
    const long r1 = r0 + BATCH_RAYS_PER_GROUP < R ? r0 + BATCH_RAYS_PER_GROUP : R;
    batch_pose_rows<V>(t, d, out, r0, r1, threadIdx.x, BATCH_BLOCK);
}

}  // namespace danbo

using namespace danbo;

extern "C" int danbo_batch_gather(const float* imgs, const float* fgs, const float* bgs, const int32_t* bg_idxs, const int32_t* cam_idxs,
                                  const float* c2ws, const float* focals, const float* centers, const float* kp3d, const float* bones,
                                  const float* skts, const float* cyls, int n_images, int n_bgs, int height, int width,
                                  const int32_t* picks, const int32_t* pixels, const float* noise, int n_picks, int per, int mask_image,
                                  float* out_rays_o, float* out_rays_d, float* out_target, float* out_fgs, float* out_bgs,
                                  float* out_kp3d, float* out_bones, float* out_skts, float* out_cyls, long long* out_cam_idxs,
                                  long long* out_kp_idx, void* stream) {
    const BatchTables t = {imgs, fgs, bgs, bg_idxs, cam_idxs, c2ws, focals, centers, kp3d, bones, skts, cyls, n_images, n_bgs, height, width};
    const BatchDraw d = {picks, pixels, noise, n_picks, per, mask_image};
    const BatchOut out = {out_rays_o, out_rays_d, out_target, out_fgs, out_bgs, out_kp3d, out_bones, out_skts, out_cyls, out_cam_idxs, out_kp_idx};
    DANBO_CHECK_ARG(batch_args_ok(t, d, out));
    if (n_picks == 0) return 0;
    const long R = (long)n_picks * per;
    const int ray_groups = ceil_div(R, BATCH_BLOCK), pose_groups = ceil_div(R, BATCH_RAYS_PER_GROUP);      // (both < 2^29: R < 2^31)
    // every pose row is a whole number of 16-byte tuples; the tables and outputs are moved as such when all six start on one
    const bool wide = (((uintptr_t)skts | (uintptr_t)kp3d | (uintptr_t)bones | (uintptr_t)out_skts | (uintptr_t)out_kp3d |
                        (uintptr_t)out_bones) & 15) == 0;
    hipLaunchKernelGGL(wide ? k_batch_gather<f32x4> : k_batch_gather<float>, dim3((unsigned)(ray_groups + pose_groups)), dim3(BATCH_BLOCK),
                       0, (hipStream_t)stream, t, d, out, ray_groups);
    DANBO_LAUNCH_RET();
}
