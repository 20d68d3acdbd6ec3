/*
 * libdanbo_hip.so -- C ABI of the mesh scores: area-weighted surface samples of a triangle mesh, the exact nearest neighbour
 * between two point sets, and the one-directional sums behind Chamfer distance, F-score and normal consistency
 * (csrc/k_mesh_score.hip; csrc/mesh_score_math.hpp states every definition once, for the kernels and for the serial restatement
 * mesh_face_areas_host / mesh_sample_host / points_nearest_host / points_score_host that the tests compare the kernels with bit for
 * bit).
 *
 * A companion of danbo_hip.h with the same conventions: every pointer is a DEVICE pointer, no function retains a pointer past the
 * call, every kernel is enqueued on `stream` (a hipStream_t passed as void*), nothing allocates or synchronises; the return value
 * is 0, a hipError_t, or DANBO_EINVAL (-22, danbo_hip.h) for a rejected argument, before any launch and with no output touched.
 * The entries are additive in ABI 9 (danbo_abi_version() of danbo_hip.h stays 9).  This header declares no struct.
 *
 * THIS FILE IS READ BY A PROGRAM, like danbo_hip.h and in the same subset of C (stated at the top of danbo_hip.h):
 * danbo-pytorch_amd/core/mesh_score.py parses it with _hip.bind_headers beside the headers of _hip.HEADERS and sets the types of
 * its entries on the library.
 *
 * Every result is a function of the inputs alone: fp32 operations in an order mesh_score_math.hpp fixes, an integer minimum for
 * the nearest point, float64 sums in a fixed order; no floating-point atomics; two calls give the same bits.  Every input is
 * finite.  Every size (V, F, M, Nq, Nr, N) lies in 1 .. 2^24.
 */
#ifndef DANBO_MESH_SCORE_H
#define DANBO_MESH_SCORE_H

#include <stddef.h>
#include <stdint.h>

#define DANBO_POINTS_TILE 1024                 /* reference points per LDS tile of danbo_points_nearest */
#define DANBO_POINTS_MAX_TAU 8                 /* thresholds of one danbo_points_score call */
#define DANBO_POINTS_SCORE_WORKSPACE_BYTES 5888 /* the workspace of danbo_points_score: 11 x 64 doubles + 256 */

#ifdef __cplusplus
extern "C" {
#endif

/* areas[f] = half the length of the cross product of the two edges of face f, in fp32.  A face with a corner index outside [0, V)
 * is not loaded from: its area is +0 and *bad_face (one int32 the caller zeroed) is set to 1.  One launch, one thread per face.
 * DANBO_EINVAL: a null pointer; V or F outside 1 .. 2^24. */
int danbo_mesh_face_areas(const float* verts /*[V,3]*/, int V, const int32_t* faces /*[F,3]*/, int F, float* areas /*[F]*/,
                          int32_t* bad_face /*[1]*/, void* stream);

/* M surface samples.  cdf [F]: the non-decreasing inclusive prefix of the face areas (an input: however it was summed); u [M,3] in
 * [0, 1).  Sample m lies on the first face f with cdf[f] > u0 cdf[F - 1] (binary search; F - 1 when there is none; a face of area
 * zero is never chosen) at the barycentric weights b0 = 1 - sqrt(u1), b1 = sqrt(u1) (1 - u2), b2 = sqrt(u1) u2.
 * pts [M,3] the point, nrm [M,3] the face's unit normal (the zero vector on a degenerate face), face [M] the face's index.  A
 * chosen face with a corner index outside [0, V) is not loaded from: the sample's point and normal are +0 and *bad_face (one
 * int32 the caller zeroed) is set to 1.  One launch, one thread per sample.
 * DANBO_EINVAL: a null pointer; V, F or M outside 1 .. 2^24. */
int danbo_mesh_sample(const float* verts /*[V,3]*/, int V, const int32_t* faces /*[F,3]*/, int F, const float* cdf /*[F]*/,
                      const float* u /*[M,3]*/, int M, float* pts /*[M,3]*/, float* nrm /*[M,3]*/, int32_t* face /*[M]*/,
                      int32_t* bad_face /*[1]*/, void* stream);

/* Bytes of the workspace of danbo_points_nearest (never 0 for accepted sizes); 0: Nq or Nr outside 1 .. 2^24. */
size_t danbo_points_nearest_workspace_bytes(int Nq, int Nr);

/* For every query q_i: d2[i] = min_j d2(i, j), d2(i, j) = fma(dz, dz, fma(dy, dy, dx dx)) with d = q_i - r_j in fp32, and idx[i]
 * the smallest j that attains it -- an exact sweep over all Nq Nr pairs.  Tiles of DANBO_POINTS_TILE reference points are staged
 * in LDS; when Nq alone gives too few workgroups the reference range is split over workgroups that combine through a 64-bit
 * integer minimum of (bits(d2) << 32) | j in the workspace, so the result does not depend on the split.
 * DANBO_EINVAL: q, r, d2, idx or workspace null; Nq or Nr outside 1 .. 2^24. */
int danbo_points_nearest(const float* q /*[Nq,3]*/, int Nq, const float* r /*[Nr,3]*/, int Nr, float* d2 /*[Nq]*/, int32_t* idx /*[Nq]*/,
                         void* workspace, void* stream);

/* The sums of one direction over N queries: out[0] = sum sqrt(d2) (float64, correctly rounded root), out[1] = sum d2, out[2] = sum
 * |n_i . m_idx[i]| (an fp32 fma chain; +0 without normals), out[3] = N, out[4 + t] = the number of queries with sqrt(d2) <= tau[t].
 * nq [N,3] and nr [Nr,3] are the normals of the queries and of the reference set: both or neither (then Nr is not read); idx is
 * read clamped to 0 .. Nr - 1.  tau [T] distances on the device, 0 <= T <= DANBO_POINTS_MAX_TAU.  workspace:
 * DANBO_POINTS_SCORE_WORKSPACE_BYTES bytes.  Two launches, a fixed summation order.
 * DANBO_EINVAL: d2, idx, out or workspace null; tau null with T > 0; only one of nq / nr; N (or Nr with normals) outside
 * 1 .. 2^24; T outside 0 .. 8. */
int danbo_points_score(const float* d2 /*[N]*/, const int32_t* idx /*[N]*/, const float* nq /*[N,3] or NULL*/,
                       const float* nr /*[Nr,3] or NULL*/, int Nr, int N, const float* tau /*[T]*/, int T, void* out /*[4 + T] float64*/,
                       void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif
