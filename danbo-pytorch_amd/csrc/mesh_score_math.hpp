// Scoring of triangle meshes (include/danbo_mesh_score.h, k_mesh_score.hip): area-weighted surface samples, the exact nearest
// neighbour between two point sets, and the one-directional sums behind Chamfer distance, F-score and normal consistency.
//
// Like depth_math.hpp and skel_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels and compiled by g++ for
// the serial restatement at the end of this file (the *_host functions), which the CPU tests check against tests/mesh_score_ref.py
// (numpy float64) and the GPU tests compare the kernels with, bit for bit.  Built with -ffp-contract=off; every product, sum,
// difference and quotient below is a separately rounded fp32 operation (mul_rn / add_rn / sub_rn / div_rn) except where fmaf is
// written; sqrtf and the float64 sqrt are the correctly rounded ones on both sides.  EVERY INPUT IS FINITE (no NaN, no infinity):
// the order of the nearest-point key relies on it.
//
// FACE f with corners A, B, C = verts[faces[3 f + 0 .. 2]]; e1 = B - A, e2 = C - A per component;
//   c = e1 x e2, each component mul - mul;  len = sqrtf(fmaf(c_z, c_z, fmaf(c_y, c_y, c_x c_x)))
//   area[f] = 0.5 len;  normal = c / len per component when 0 < len < inf, else the zero vector (a degenerate face).
//   A face with a corner index outside [0, V) is never loaded from: its area is +0, a sample that chooses it is all +0, and the
//   call's flag word is set to 1.
// SURFACE SAMPLE m from u = (u0, u1, u2) in [0, 1) and cdf [F], the non-decreasing inclusive prefix of the areas (an INPUT: the
//   kernel and the restatement read the same array):
//   face  = the first f with cdf[f] > u0 cdf[F - 1] (the product rounded), by binary search, F - 1 when there is none: a face of
//           area zero (cdf[f] == cdf[f - 1]) is never the first.
//   r = sqrtf(u1);  b0 = 1 - r;  b1 = r (1 - u2);  b2 = r u2
//   point = fmaf(b2, C, fmaf(b1, B, b0 A)) per component; normal = the face's.
// NEAREST POINT of query q_i among r_0 .. r_{Nr-1}: d = q - r per component,
//   d2(i, j) = fmaf(d_z, d_z, fmaf(d_y, d_y, d_x d_x))                       (>= +0, never -0, never NaN for finite inputs)
//   key(i, j) = (bits(d2) << 32) | j as an unsigned 64-bit integer: for d2 >= +0 the bit pattern orders like the value, so the
//   smallest key is the smallest d2 and among equal d2 the smallest j.  Result: d2 and j of min_j key(i, j) -- an integer minimum,
//   independent of the order in which the j are visited and of how the range of j is split.
// ONE-DIRECTIONAL SUMS over i = 0 .. N - 1 from d2 [N], idx [N], optionally unit normals n [N,3] of the queries and m [Nr,3] of the
//   reference set (idx read clamped to 0 .. Nr - 1), and T <= 8 thresholds tau_t (distances):
//   out[0] = sum sqrt((double) d2_i)      out[1] = sum (double) d2_i
//   out[2] = sum (double) |fmaf(n_z, m_z, fmaf(n_y, m_y, n_x m_x))| with m = m[idx_i]; +0 without normals
//   out[3] = N      out[4 + t] = the number of i with sqrt((double) d2_i) <= (double) tau_t  (an exact integer in a double)
//   ORDER: chain c (0 .. SCORE_CHAINS - 1) starts from +0 and adds the terms of items c, c + SCORE_CHAINS, ... in that order; the
//   SCORE_BLOCK chains c = SCORE_BLOCK b + l of block b go through score_tree (for s = n / 2 .. 1: u[i] = u[i] + u[i + s], i < s),
//   and the SCORE_BLOCKS block sums through the same tree.  float64 additions, each rounded once; no atomics.
#pragma once
#include <stddef.h>
#include "sample_math.hpp"

namespace danbo {

constexpr int MESH_SCORE_MAX = 1 << 24;           // V, F, M, Nq, Nr, N: 1 .. 2^24
constexpr int MESH_SCORE_EINVAL = -22;            // DANBO_EINVAL of danbo_hip.h
constexpr int POINTS_TILE = 1024;                 // reference points per LDS tile (DANBO_POINTS_TILE)
constexpr int POINTS_QBLOCK = 1024;               // queries per workgroup: 256 lanes x 4
constexpr int POINTS_TARGET_BLOCKS = 512;         // the reference range is split until about this many workgroups exist
constexpr int SCORE_MAX_TAU = 8;
constexpr int SCORE_BLOCK = 256, SCORE_BLOCKS = 64, SCORE_CHAINS = SCORE_BLOCK * SCORE_BLOCKS;
constexpr int SCORE_MAX_Q = 3 + SCORE_MAX_TAU;    // summed quantities: three sums and the counts
constexpr size_t SCORE_WORKSPACE_BYTES = (size_t)SCORE_MAX_Q * SCORE_BLOCKS * sizeof(double) + 256;

DANBO_HD bool mesh_score_size_ok(long n) { return n >= 1 && n <= MESH_SCORE_MAX; }

// ---- argument rules (the entry points and the restatement reject the same) ----
DANBO_HD bool mesh_areas_ok(const void* verts, int V, const void* faces, int F, const void* areas, const void* flag) {
    return verts && faces && areas && flag && mesh_score_size_ok(V) && mesh_score_size_ok(F);
}
DANBO_HD bool mesh_sample_ok(const void* verts, int V, const void* faces, int F, const void* cdf, const void* u, int M, const void* pts,
                             const void* nrm, const void* face, const void* flag) {
    return verts && faces && cdf && u && pts && nrm && face && flag && mesh_score_size_ok(V) && mesh_score_size_ok(F) &&
           mesh_score_size_ok(M);
}
DANBO_HD bool points_nearest_ok(const void* q, int Nq, const void* r, int Nr, const void* d2, const void* idx) {
    return q && r && d2 && idx && mesh_score_size_ok(Nq) && mesh_score_size_ok(Nr);
}
DANBO_HD bool points_score_ok(const void* d2, const void* idx, const void* nq, const void* nr, int Nr, int N, const void* tau, int T,
                              const void* out) {
    return d2 && idx && out && mesh_score_size_ok(N) && T >= 0 && T <= SCORE_MAX_TAU && (T == 0 || tau) &&
           ((nq == nullptr) == (nr == nullptr)) && (nq == nullptr || mesh_score_size_ok(Nr));
}

// ---- how danbo_points_nearest divides its work (a function of the sizes alone; the result does not depend on it) ----
DANBO_HD int points_tiles(int Nr) { return (Nr + POINTS_TILE - 1) / POINTS_TILE; }
DANBO_HD int points_qblocks(int Nq) { return (Nq + POINTS_QBLOCK - 1) / POINTS_QBLOCK; }
// tiles of the reference set per workgroup row
DANBO_HD int points_tiles_per_split(int Nq, int Nr) {
    const int tiles = points_tiles(Nr), qb = points_qblocks(Nq);
    int want = (POINTS_TARGET_BLOCKS + qb - 1) / qb;
    if (want > tiles) want = tiles;
    return (tiles + want - 1) / want;
}
DANBO_HD int points_splits(int Nq, int Nr) {
    const int tps = points_tiles_per_split(Nq, Nr);
    return (points_tiles(Nr) + tps - 1) / tps;
}
// bytes of danbo_points_nearest's workspace: one 64-bit key per query when the reference range is split; 0 for a rejected size
DANBO_HD size_t points_nearest_workspace_size(int Nq, int Nr) {
    if (!mesh_score_size_ok(Nq) || !mesh_score_size_ok(Nr)) return 0;
    return 256 + (points_splits(Nq, Nr) > 1 ? (size_t)Nq * sizeof(uint64_t) : 0);
}

// ---- faces ----
struct ScoreVec {
    float x, y, z;
};
DANBO_HD ScoreVec score_load3(const float* p, long i) { return ScoreVec{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
DANBO_HD float score_fma_len(ScoreVec c) { return sqrtf(fmaf(c.z, c.z, fmaf(c.y, c.y, mul_rn(c.x, c.x)))); }
DANBO_HD float score_fma_dot(ScoreVec a, ScoreVec b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, mul_rn(a.x, b.x))); }
// the three corner indices of face f -> false: one lies outside [0, V) (nothing may be loaded through them)
DANBO_HD bool mesh_face_corners(const int32_t* faces, long f, int V, int* a, int* b, int* c) {
    *a = faces[3 * f], *b = faces[3 * f + 1], *c = faces[3 * f + 2];
    return *a >= 0 && *a < V && *b >= 0 && *b < V && *c >= 0 && *c < V;
}
DANBO_HD ScoreVec mesh_face_cross(ScoreVec A, ScoreVec B, ScoreVec C) {
    const ScoreVec e1{sub_rn(B.x, A.x), sub_rn(B.y, A.y), sub_rn(B.z, A.z)}, e2{sub_rn(C.x, A.x), sub_rn(C.y, A.y), sub_rn(C.z, A.z)};
    return ScoreVec{sub_rn(mul_rn(e1.y, e2.z), mul_rn(e1.z, e2.y)), sub_rn(mul_rn(e1.z, e2.x), mul_rn(e1.x, e2.z)),
                    sub_rn(mul_rn(e1.x, e2.y), mul_rn(e1.y, e2.x))};
}
// area of face f; *bad set when a corner index is out of range (area +0)
DANBO_HD float mesh_face_area(const float* verts, int V, const int32_t* faces, long f, bool* bad) {
    int a, b, c;
    if (!mesh_face_corners(faces, f, V, &a, &b, &c)) {
        *bad = true;
        return 0.f;
    }
    return mul_rn(0.5f, score_fma_len(mesh_face_cross(score_load3(verts, a), score_load3(verts, b), score_load3(verts, c))));
}

// ---- surface samples ----
// the first f with cdf[f] > target, F - 1 when there is none
DANBO_HD int mesh_pick_face(const float* cdf, int F, float u0) {
    const float target = mul_rn(u0, cdf[F - 1]);
    int lo = 0, hi = F;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    return lo < F ? lo : F - 1;
}
DANBO_HD void mesh_bary(float u1, float u2, float* b0, float* b1, float* b2) {
    const float r = sqrtf(u1);
    *b0 = sub_rn(1.f, r);
    *b1 = mul_rn(r, sub_rn(1.f, u2));
    *b2 = mul_rn(r, u2);
}
DANBO_HD float mesh_bary_mix(float b0, float b1, float b2, float A, float B, float C) { return fmaf(b2, C, fmaf(b1, B, mul_rn(b0, A))); }
// sample m: pts[3 m ..], nrm[3 m ..], face[m] -> false: the chosen face has a corner out of range (the outputs are +0, the face's index)
DANBO_HD bool mesh_sample_one(const float* verts, int V, const int32_t* faces, int F, const float* cdf, const float* u, long m, float* pts,
                              float* nrm, int32_t* face) {
    const int f = mesh_pick_face(cdf, F, u[3 * m]);
    face[m] = f;
    int a, b, c;
    if (!mesh_face_corners(faces, f, V, &a, &b, &c)) {
        pts[3 * m] = pts[3 * m + 1] = pts[3 * m + 2] = 0.f;
        nrm[3 * m] = nrm[3 * m + 1] = nrm[3 * m + 2] = 0.f;
        return false;
    }
    const ScoreVec A = score_load3(verts, a), B = score_load3(verts, b), C = score_load3(verts, c);
    float b0, b1, b2;
    mesh_bary(u[3 * m + 1], u[3 * m + 2], &b0, &b1, &b2);
    pts[3 * m] = mesh_bary_mix(b0, b1, b2, A.x, B.x, C.x);
    pts[3 * m + 1] = mesh_bary_mix(b0, b1, b2, A.y, B.y, C.y);
    pts[3 * m + 2] = mesh_bary_mix(b0, b1, b2, A.z, B.z, C.z);
    const ScoreVec cr = mesh_face_cross(A, B, C);
    const float len = score_fma_len(cr);
    const bool ok = len > 0.f && len < INFINITY;
    nrm[3 * m] = ok ? div_rn(cr.x, len) : 0.f;
    nrm[3 * m + 1] = ok ? div_rn(cr.y, len) : 0.f;
    nrm[3 * m + 2] = ok ? div_rn(cr.z, len) : 0.f;
    return true;
}

// ---- nearest point ----
DANBO_HD float points_d2(float qx, float qy, float qz, float rx, float ry, float rz) {
    const float dx = sub_rn(qx, rx), dy = sub_rn(qy, ry), dz = sub_rn(qz, rz);
    return fmaf(dz, dz, fmaf(dy, dy, mul_rn(dx, dx)));
}
DANBO_HD uint32_t points_bits(float d2) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = d2;
    return v.u;
}
DANBO_HD float points_unbits(uint32_t b) {
    union {
        float f;
        uint32_t u;
    } v;
    v.u = b;
    return v.f;
}
DANBO_HD uint64_t points_key(float d2, int j) { return ((uint64_t)points_bits(d2) << 32) | (uint32_t)j; }
constexpr uint64_t POINTS_KEY_NONE = ~(uint64_t)0;      // above every key of a finite input

// ---- one-directional sums ----
// the 3 + T terms of item i into v[]: sqrt(d2), d2, |n . m|, and 1 or 0 per threshold
DANBO_HD void score_terms(const float* d2, const int32_t* idx, const float* nq, const float* nr, int Nr, long i, const float* tau, int T,
                          double* v) {
    const double dd = (double)d2[i];
#if defined(__HIP_DEVICE_COMPILE__)
    const double d = __dsqrt_rn(dd);
#else
    const double d = sqrt(dd);
#endif
    v[0] = d, v[1] = dd, v[2] = 0.0;
    if (nq) {
        int j = idx[i];
        j = j < 0 ? 0 : (j < Nr ? j : Nr - 1);
        v[2] = (double)fabsf(score_fma_dot(score_load3(nq, i), score_load3(nr, j)));
    }
    for (int t = 0; t < SCORE_MAX_TAU; ++t)      // (a constant trip count: v[] stays in registers on the device)
        if (t < T) v[3 + t] = d <= (double)tau[t] ? 1.0 : 0.0;
}
// THE tree, for nq arrays of n = 2^k leaves `qstride` doubles apart, walked by `nthreads` cooperating threads (serial: tid 0 of 1,
// sync a no-op); the sum of array q ends in u[q * qstride]
template <class Sync>
DANBO_HD void score_tree(double* u, int n, int nq, int qstride, int tid, int nthreads, Sync sync) {
    int ls = 0;
    while ((2 << ls) <= n) ++ls;
    for (--ls; ls >= 0; --ls) {
        const int s = 1 << ls;
        for (int k = tid; k < nq * s; k += nthreads) {
            double* p = u + (k >> ls) * qstride + (k & (s - 1));
            p[0] = dadd_rn(p[0], p[s]);
        }
        sync();
    }
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial restatement (host): the four calls of danbo_mesh_score.h on host memory without the stream and the workspaces, one item
// after the other.  Each returns 0, or -22 for a rejected argument (no output touched).

inline int mesh_face_areas_host(const float* verts, int V, const int32_t* faces, int F, float* areas, int32_t* flag) {
    if (!mesh_areas_ok(verts, V, faces, F, areas, flag)) return MESH_SCORE_EINVAL;
    for (long f = 0; f < F; ++f) {
        bool bad = false;
        areas[f] = mesh_face_area(verts, V, faces, f, &bad);
        if (bad) *flag = 1;
    }
    return 0;
}

inline int mesh_sample_host(const float* verts, int V, const int32_t* faces, int F, const float* cdf, const float* u, int M, float* pts,
                            float* nrm, int32_t* face, int32_t* flag) {
    if (!mesh_sample_ok(verts, V, faces, F, cdf, u, M, pts, nrm, face, flag)) return MESH_SCORE_EINVAL;
    for (long m = 0; m < M; ++m)
        if (!mesh_sample_one(verts, V, faces, F, cdf, u, m, pts, nrm, face)) *flag = 1;
    return 0;
}

inline int points_nearest_host(const float* q, int Nq, const float* r, int Nr, float* d2, int32_t* idx) {
    if (!points_nearest_ok(q, Nq, r, Nr, d2, idx)) return MESH_SCORE_EINVAL;
    for (long i = 0; i < Nq; ++i) {
        uint64_t best = POINTS_KEY_NONE;
        for (int j = 0; j < Nr; ++j) {
            const uint64_t k = points_key(points_d2(q[3 * i], q[3 * i + 1], q[3 * i + 2], r[3 * (long)j], r[3 * (long)j + 1], r[3 * (long)j + 2]), j);
            if (k < best) best = k;
        }
        d2[i] = points_unbits((uint32_t)(best >> 32));
        idx[i] = (int32_t)(uint32_t)best;
    }
    return 0;
}

inline int points_score_host(const float* d2, const int32_t* idx, const float* nq, const float* nr, int Nr, int N, const float* tau, int T,
                             double* out) {
    if (!points_score_ok(d2, idx, nq, nr, Nr, N, tau, T, out)) return MESH_SCORE_EINVAL;
    const int Q = 3 + T;
    const auto no_sync = [] {};
    double part[SCORE_MAX_Q * SCORE_BLOCKS];
    for (int b = 0; b < SCORE_BLOCKS; ++b) {
        double leaf[SCORE_MAX_Q * SCORE_BLOCK];
        for (int l = 0; l < SCORE_BLOCK; ++l) {
            double acc[SCORE_MAX_Q], v[SCORE_MAX_Q];
            for (int k = 0; k < Q; ++k) acc[k] = 0.0;
            for (long i = (long)b * SCORE_BLOCK + l; i < N; i += SCORE_CHAINS) {
                score_terms(d2, idx, nq, nr, Nr, i, tau, T, v);
                for (int k = 0; k < Q; ++k) acc[k] = dadd_rn(acc[k], v[k]);
            }
            for (int k = 0; k < Q; ++k) leaf[k * SCORE_BLOCK + l] = acc[k];
        }
        score_tree(leaf, SCORE_BLOCK, Q, SCORE_BLOCK, 0, 1, no_sync);
        for (int k = 0; k < Q; ++k) part[k * SCORE_BLOCKS + b] = leaf[k * SCORE_BLOCK];
    }
    score_tree(part, SCORE_BLOCKS, Q, SCORE_BLOCKS, 0, 1, no_sync);
    out[0] = part[0], out[1] = part[SCORE_BLOCKS], out[2] = part[2 * SCORE_BLOCKS], out[3] = (double)N;
    for (int t = 0; t < T; ++t) out[4 + t] = part[(3 + t) * SCORE_BLOCKS];
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
