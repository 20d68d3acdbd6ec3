/*
 * libdanbo_hip.so -- C ABI of the triangle rasteriser for the extracted meshes (turntable normal maps).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument.  The entries are additive in ABI 9
 * (danbo_abi_version() of danbo_hip.h stays 9).  They stand in a header of their own because danbo_hip.h is the pinned statement
 * of the render and training path (tests/test_abi_binding.py counts its entry points and constants).
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/_hip.py parses it on import and binds it as header("danbo_raster.h");
 * tests/test_abi_binding.py checks what the parser derived against the host compiler's view of this file.
 */
#ifndef DANBO_RASTER_H
#define DANBO_RASTER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Triangle rasteriser for the extracted meshes.  Replaces the GL pass of the reference's separate
 * render_mesh.py: an orthographic camera (render/camera.py:186-188, ortho(+-w r / 2, +-h r / 2)), the colour 0.5 * normal + 0.5 per
 * vertex, background 1, depth-tested, not culled, one sample per pixel.
 *   verts [V,3], tris [T,3] (int32 indices), views [n_views][12]: model -> view matrices, 3x4 row-major; view space has x right, y
 *   up, z towards the viewer.  Per vertex p = M (v, 1); x_pix = (p.x / (2 half_extent_x) + 0.5) * width, y_pix = 0.5 * height -
 *   p.y * (width / (2 half_extent_x)) (square pixels, row 0 at the top), snapped to 1/256 pixel; depth = p.z, the larger the nearer.
 *   A pixel is covered iff its centre lies inside the triangle, a centre on an edge belonging to exactly one of the two triangles
 *   that share it (a tie rule in exact integers: a closed mesh has no cracks and no double hits); both windings are drawn.
 *   Depth and colour are interpolated with fp32 barycentrics; the largest depth wins, at equal depth the lowest triangle index.
 *   A triangle with an index outside [0, V), a vertex whose p is not finite or lies 2^20 pixels outside, or no area draws nothing.
 *   (csrc/raster_math.hpp states every rounding; the kernels equal its serial restatement bit for bit, and two runs give the same
 *   bits: visibility is one integer maximum per pixel, nothing depends on the order of arrival.)
 *   attr_mode: DANBO_RASTER_COLOR -- attr [V,3] is interpolated as it is; DANBO_RASTER_NORMAL -- attr holds vertex normals, the
 *   colour 0.5 n' + 0.5 of n' = normalise(M3x3 n) (0 where the length is 0 or not finite) is interpolated; DANBO_RASTER_FLAT --
 *   attr is not read (NULL): per triangle 0.5 n + 0.5 of the unit normal of the view-space triangle, cross(B - A, C - A).
 * Writes, per view, rgb [H,W,3], depth [H,W] and tri_id [H,W] -- whichever is not NULL; a pixel no triangle covers gets
 * background[3], -INFINITY and -1.  The views are rendered one after the other on the stream and share `workspace`
 * (danbo_raster_workspace_bytes: 8 B per pixel + 28 B per vertex; 0 for sizes outside the limits).  n_tris = 0: background only.
 * DANBO_EINVAL before any launch: height or width outside 1 .. 4096, n_verts < 0, n_tris < 0, n_views < 1, an unknown attr_mode,
 * attr == NULL with a mode other than FLAT, half_extent_x not finite or <= 0, a null (views, background, workspace; verts / tris
 * unless their count is 0) or misaligned pointer, rgb, depth and tri_id all NULL.
 * ------------------------------------------------------------------------------------- */
#define DANBO_RASTER_COLOR 0
#define DANBO_RASTER_NORMAL 1
#define DANBO_RASTER_FLAT 2
size_t danbo_raster_workspace_bytes(int n_verts, int height, int width);
int danbo_raster_mesh(const float* verts, int n_verts, const int* tris, int n_tris, const float* attr /*[V,3] or NULL*/, int attr_mode,
                      const float* views /*device [n_views][12]*/, int n_views, float half_extent_x, int height, int width,
                      const float* background /*device [3]*/, void* workspace, float* rgb /*[n_views,H,W,3] or NULL*/,
                      float* depth /*[n_views,H,W] or NULL*/, int* tri_id /*[n_views,H,W] or NULL*/, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* DANBO_RASTER_H */
