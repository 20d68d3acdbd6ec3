// The skeleton overlay: the posed 24-joint skeleton projected into a frame and drawn over it (reference run_render.py:1332-1346 ->
// draw_skeletons_3d, core/utils/skeleton_utils.py:478-491, 1454-1472, 1577-1612) -- include/danbo_skel.h, k_skel.hip.
//
// Like grid_cc_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels and compiled by g++ for the serial
// restatement at the end of this file (skel_project_host / skel_draw_host), which the CPU tests check against tests/skel_ref.py
// (numpy float32 and Python integers) and the GPU tests compare the kernels with, bit for bit.  Built with -ffp-contract=off: a
// fused multiply-add appears only where the source says fmaf, and this file says it nowhere.
//
// PROJECTION (float32; world_to_cam of the reference with its diagonal intrinsic matrix multiplied out), per frame n and joint j:
// p = kps[n, j], E = w2c[n] (3 x 4, row-major), focals fx, fy, offset (ox, oy) = centers[n], or (0.5 W, 0.5 H) without centres:
//     x = ((E00 px + E01 py) + E02 pz) + E03         (y, z likewise from rows 1, 2)
//     zz = z + 1e-8f
//     u = (fx x) / zz + ox,   v = (fy y) / zz + oy   (a quotient equal to +inf becomes 0 before the offset is added, as the
//                                                     reference's `cam_pts[cam_pts == np.inf] = 0.`)
// SEGMENT ENDS (int32).  Bone j runs from joint j to its parent skel_parent(j), formed as draw_skeleton2d forms them:
//     a = rint(u_j, v_j),   b = rint(u_j + (u_par - u_j), v_j + (v_par - v_j))
// in float32 as written, rounding to nearest-even (Python's round).  A coordinate that is NaN or -inf marks the bone as SKIPPED
// (ends = {SKEL_SKIP, 0, 0, 0}; the reference raises there); every other coordinate is clamped to [-2^30, 2^30].  The root's
// parent is the root: its bone is the degenerate segment a = b, a disc.
// COVERAGE (exact, in integers; a rule of this project's own -- cv2.line's is not stated anywhere but in its source).  Pixel
// p = (x, y) is covered by the segment (a, b) at width w (1 .. 64) iff its centre lies within w / 2 of the segment:
//     d = b - a, r = p - a, L = d.d, t = r.d
//     t <= 0 :  r.r <= floor(w^2 / 4)
//     t >= L :  (p - b).(p - b) <= floor(w^2 / 4)
//     else   :  (2 |rx dy - ry dx|)^2 <= w^2 L                    (128-bit products: skel_mul128)
// With |coordinate| <= 2^30 and 0 <= x, y < 4096: |d| <= 2^31, so L <= 2^63 (held unsigned); |r| < 2^30 + 2^12, so |t| and
// |rx dy - ry dx| < 2^62 + 2^45 and twice the latter fits 64 unsigned bits; r.r < 2^61.  Ends that come from a caller, not from the
// projection, are clamped to the same range when they are read (skel_segment), so the bounds hold for any input.
// A pixel outside the segment's bounding box grown by ceil(w / 2) cannot be covered: the cheap reject, which changes no result.
// PAINT ORDER: bones 0 .. 23 in order, a later bone overwrites an earlier one: the pixel takes the colour of the largest
// covering j.  The 24 x 3 colour table is the caller's (the reference's rule on the joints' names is Python's).
// UNCOVERED PIXELS hold the source frame: a uint8 source is copied, a float32 source quantised as the reference's
// (rgb * 255).astype(uint8), made total -- NaN -> 0, clamped to [0, 255], truncated (skel_quant); numpy's result on [0, 1].
#pragma once
#include "sample_math.hpp"
#if !defined(__HIPCC__)
#include <string.h>
#endif

namespace danbo {

constexpr int SKEL_MAX_WIDTH = 64, SKEL_MAX_DIM = 4096, SKEL_MAX_FRAMES = 1 << 20;
constexpr int32_t SKEL_SKIP = -2147483647 - 1;      // INT32_MIN in ends[.][0]: the bone is not drawn
constexpr int32_t SKEL_LIMIT = 1 << 30;             // |coordinate| of an end
constexpr int SKEL_PIX = 4;                         // consecutive pixels of a row that one thread of the draw kernel owns

// the parent of every joint (SMPLSkeleton.joint_trees; tests/test_skel_host.py holds the table to it)
DANBO_HD int skel_parent(int j) {
    constexpr int8_t parent[J] = {0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
    return parent[j];
}

DANBO_HD bool skel_dims_ok(int N, int H, int W) {
    return N >= 1 && N <= SKEL_MAX_FRAMES && H >= 1 && H <= SKEL_MAX_DIM && W >= 1 && W <= SKEL_MAX_DIM;
}
// two byte ranges that share no address
DANBO_HD bool skel_disjoint(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
}

// ---- projection ----
DANBO_HD float skel_cam(const float* e, const float* p) {
    return add_rn(add_rn(add_rn(mul_rn(e[0], p[0]), mul_rn(e[1], p[1])), mul_rn(e[2], p[2])), e[3]);
}
DANBO_HD float skel_image(float f, float c, float zz, float offset) {
    float q = div_rn(mul_rn(f, c), zz);
    if (q == INFINITY) q = 0.f;
    return add_rn(q, offset);
}
// (u, v) of the point p seen through E [3,4]
DANBO_HD void skel_uv(const float* p, const float* E, float fx, float fy, float ox, float oy, float* u, float* v) {
    const float x = skel_cam(E, p), y = skel_cam(E + 4, p), z = skel_cam(E + 8, p);
    const float zz = add_rn(z, 1e-8f);
    *u = skel_image(fx, x, zz, ox);
    *v = skel_image(fy, y, zz, oy);
}
// focals and offset of frame n
DANBO_HD void skel_camera(const float* focals, int focal_stride, const float* centers, int n, int H, int W, float* fx, float* fy,
                          float* ox, float* oy) {
    *fx = focals[(long)n * focal_stride];
    *fy = focals[(long)n * focal_stride + (focal_stride - 1)];
    *ox = centers ? centers[2 * (long)n] : mul_rn(0.5f, (float)W);
    *oy = centers ? centers[2 * (long)n + 1] : mul_rn(0.5f, (float)H);
}

// ---- segment ends ----
DANBO_HD bool skel_unusable(float c) { return c != c || c == -INFINITY; }
DANBO_HD int32_t skel_clamp(int32_t c) { return c < -SKEL_LIMIT ? -SKEL_LIMIT : (c > SKEL_LIMIT ? SKEL_LIMIT : c); }
DANBO_HD int32_t skel_round(float c) {
    const float r = rintf(c);
    return r <= -(float)SKEL_LIMIT ? -SKEL_LIMIT : (r >= (float)SKEL_LIMIT ? SKEL_LIMIT : (int32_t)r);
}
// the ends {ax, ay, bx, by} of a bone from the unrounded image points of its joint and of the joint's parent
DANBO_HD void skel_ends(float uj, float vj, float up, float vp, int32_t* e) {
    const float bu = add_rn(uj, sub_rn(up, uj)), bv = add_rn(vj, sub_rn(vp, vj));
    if (skel_unusable(uj) || skel_unusable(vj) || skel_unusable(bu) || skel_unusable(bv)) {
        e[0] = SKEL_SKIP; e[1] = 0; e[2] = 0; e[3] = 0;
        return;
    }
    e[0] = skel_round(uj); e[1] = skel_round(vj); e[2] = skel_round(bu); e[3] = skel_round(bv);
}
// bone j of one frame: kps [24,3] of the frame, E [3,4]
DANBO_HD void skel_bone(const float* kps, const float* E, float fx, float fy, float ox, float oy, int j, int32_t* e) {
    float uj, vj, up, vp;
    skel_uv(kps + 3 * j, E, fx, fy, ox, oy, &uj, &vj);
    skel_uv(kps + 3 * skel_parent(j), E, fx, fy, ox, oy, &up, &vp);
    skel_ends(uj, vj, up, vp, e);
}

// ---- coverage ----
// a segment as the draw reads it: the clamped ends and the bounding box grown by ceil(w / 2), empty (x0 > x1) for a skipped bone
struct SkelSegment {
    int32_t ax, ay, bx, by, x0, x1, y0, y1;
};
DANBO_HD SkelSegment skel_segment(const int32_t* e, int width) {
    SkelSegment s;
    if (e[0] == SKEL_SKIP) {
        s.ax = s.ay = s.bx = s.by = 0;
        s.x0 = s.y0 = 1; s.x1 = s.y1 = 0;
        return s;
    }
    const int grow = (width + 1) / 2;
    s.ax = skel_clamp(e[0]); s.ay = skel_clamp(e[1]); s.bx = skel_clamp(e[2]); s.by = skel_clamp(e[3]);
    s.x0 = (s.ax < s.bx ? s.ax : s.bx) - grow; s.x1 = (s.ax < s.bx ? s.bx : s.ax) + grow;
    s.y0 = (s.ay < s.by ? s.ay : s.by) - grow; s.y1 = (s.ay < s.by ? s.by : s.ay) + grow;
    return s;
}
DANBO_HD bool skel_in_box(const SkelSegment& s, int x, int y) { return x >= s.x0 && x <= s.x1 && y >= s.y0 && y <= s.y1; }

// the one 128-bit product of the device and the host build
struct SkelU128 {
    uint64_t hi, lo;
};
DANBO_HD SkelU128 skel_mul128(uint64_t a, uint64_t b) {
    const unsigned __int128 p = (unsigned __int128)a * b;
    return SkelU128{(uint64_t)(p >> 64), (uint64_t)p};
}
DANBO_HD bool skel_le128(SkelU128 a, SkelU128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo <= b.lo); }

// the rule (the bounds of every term: the head of this file)
DANBO_HD bool skel_covers(const SkelSegment& s, int x, int y, int width) {
    const int64_t dx = (int64_t)s.bx - s.ax, dy = (int64_t)s.by - s.ay, rx = (int64_t)x - s.ax, ry = (int64_t)y - s.ay;
    const int64_t quarter = (int64_t)((width * width) >> 2);
    const uint64_t L = (uint64_t)(dx * dx) + (uint64_t)(dy * dy);
    const int64_t t = rx * dx + ry * dy;
    if (t <= 0) return rx * rx + ry * ry <= quarter;
    if ((uint64_t)t >= L) {
        const int64_t qx = (int64_t)x - s.bx, qy = (int64_t)y - s.by;
        return qx * qx + qy * qy <= quarter;
    }
    const int64_t cross = rx * dy - ry * dx;
    const uint64_t twice = 2u * (uint64_t)(cross < 0 ? -cross : cross);
    return skel_le128(skel_mul128(twice, twice), skel_mul128((uint64_t)(width * width), L));
}

// ---- the source frame ----
DANBO_HD uint32_t skel_quant(float c) {
    const float s = mul_rn(c, 255.f);
    if (!(s > 0.f)) return 0u;      // NaN, zero and everything below
    return s >= 255.f ? 255u : (uint32_t)(int)s;
}
// a pixel as r | g << 8 | b << 16
DANBO_HD uint32_t skel_pack(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// the pixel (x, y) of the overlay: `rgb` (the packed source pixel) or the colour of the largest covering bone
DANBO_HD uint32_t skel_paint(const SkelSegment* segs, const uint32_t* colours, int width, int x, int y, uint32_t rgb) {
    for (int j = 0; j < J; ++j)
        if (skel_in_box(segs[j], x, y) && skel_covers(segs[j], x, y, width)) rgb = colours[j];
    return rgb;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial restatement (host): the same two calls as danbo_skel_project / danbo_skel_draw without the stream, the same definitions,
// one bone and one pixel after the other.  Returns 0, or -22 for a rejected argument.
inline int skel_project_host(const float* kps, const float* w2c, const float* focals, int focal_stride, const float* centers, int N,
                             int H, int W, int32_t* ends) {
    if (!kps || !w2c || !focals || !ends || (focal_stride != 1 && focal_stride != 2) || !skel_dims_ok(N, H, W)) return -22;
    for (int n = 0; n < N; ++n) {
        float fx, fy, ox, oy;
        skel_camera(focals, focal_stride, centers, n, H, W, &fx, &fy, &ox, &oy);
        for (int j = 0; j < J; ++j)
            skel_bone(kps + (long)n * J * 3, w2c + (long)n * 12, fx, fy, ox, oy, j, ends + ((long)n * J + j) * 4);
    }
    return 0;
}

inline int skel_draw_host(const void* src, int src_is_float, const int32_t* ends, const uint8_t* colours, int width, int N, int H,
                          int W, uint8_t* dst) {
    if (!src || !ends || !colours || !dst || (src_is_float != 0 && src_is_float != 1) || width < 1 || width > SKEL_MAX_WIDTH ||
        !skel_dims_ok(N, H, W))
        return -22;
    const size_t n_values = (size_t)N * H * W * 3;
    if (!skel_disjoint(src, n_values * (src_is_float ? 4 : 1), dst, n_values)) return -22;
    uint32_t table[J];
    for (int j = 0; j < J; ++j) table[j] = skel_pack(colours[3 * j], colours[3 * j + 1], colours[3 * j + 2]);
    for (int n = 0; n < N; ++n) {
        SkelSegment segs[J];
        for (int j = 0; j < J; ++j) segs[j] = skel_segment(ends + ((long)n * J + j) * 4, width);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long at = (((long)n * H + y) * W + x) * 3;
                uint32_t rgb;
                if (src_is_float) {
                    float c[3];
                    memcpy(c, static_cast<const float*>(src) + at, 12);
                    rgb = skel_pack(skel_quant(c[0]), skel_quant(c[1]), skel_quant(c[2]));
                } else {
                    const uint8_t* c = static_cast<const uint8_t*>(src) + at;
                    rgb = skel_pack(c[0], c[1], c[2]);
                }
                rgb = skel_paint(segs, table, width, x, y, rgb);
                dst[at] = (uint8_t)rgb; dst[at + 1] = (uint8_t)(rgb >> 8); dst[at + 2] = (uint8_t)(rgb >> 16);
            }
    }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
