// Depth and normal maps of the volume renderer (include/danbo_depth.h, k_depth.hip): the expected and the level depth of every ray
// from the weights and sorted depths the final composite already made, and the normal map of an assembled depth frame.  The only
// reference fact is the definition depth_map = sum(weights * z_vals) of raw2outputs (reference core/networks/nerf.py:337).
//
// Like skel_math.hpp: plain scalar C++ marked DANBO_HD, inlined into the gfx950 kernels and compiled by g++ for the serial
// restatement at the end of this file (depth_composite_host / depth_normals_host), which the CPU tests check against
// tests/depth_ref.py (numpy float64) and the GPU tests compare the kernels with, bit for bit.  Built with -ffp-contract=off; every
// product, sum, difference and quotient below is a separately rounded fp32 operation (mul_rn / add_rn / sub_rn / div_rn), sqrtf
// is the correctly rounded one on both sides.
//
// PER RAY: n = S + Sf positions (1 .. 320) of the sorted order with weights w_k and depths z_k.
//   term_k = w_k == 0 ? +0 : w_k z_k                     (a position of weight 0 contributes +0 whatever its depth holds)
//   EXPECTED DEPTH  depth = sum_k term_k in the order of danbo_composite_colors_fwd: lane l (0 .. 63) starts from +0 and adds the
//     terms of positions l, l + 64, l + 128, ... in that order; the 64 partial sums then go through the wavefront's scan tree
//     (depth_wave_scan below) and the result is the tree's value at lane 63.
//   LEVEL DEPTH  depth_level = z_{k*}, k* the first position whose inclusive prefix sum of w is >= level (0 < level <= 1), +0 when
//     no position reaches it.  The prefix of position k = 64 s + l (strip s, lane l) is
//         prefix_k = carry_s + scan_s[l]
//     where scan_s = depth_wave_scan of the strip's 64 weights (positions at or beyond n read as +0) and the carries are added in
//     order: carry_0 = +0, carry_{s+1} = prefix_{64 s + 63}.  "First" is the smallest k with prefix_k >= level: strips in order,
//     lanes in order inside a strip (the rounded prefixes need not be monotonic; the rule does not ask them to be).
//   THE SCAN TREE (depth_wave_scan: common.hpp's wave_scan_add -- the DPP scan of a wavefront -- written out).  Six steps on the
//     64 values x[0 .. 63], each step x[l] = x[l] + t[l] for ALL lanes at once, t read before any lane of the step is written:
//       steps 1-4, d = 1, 2, 4, 8:  t[l] = (l mod 16 >= d) ? x[l - d] : +0        (Hillis-Steele inside each row of 16 lanes)
//       step 5:                      t[l] = (l div 16 is 1 or 3) ? x[16 (l div 16) - 1] : +0   (the row before: rows 0->1, 2->3)
//       step 6:                      t[l] = (l >= 32) ? x[31] : +0                              (the lower half into the upper)
//     After it x[l] is the inclusive prefix of lanes 0 .. l and x[63] the total.  The additions of +0 are made (they matter for
//     a -0 only) so that the restatement is the instruction sequence, not a simplification of it.
//
// PER PIXEL of an assembled frame: depth, acc [N,H,W] (0 outside the cast box), cast [N,H,W] uint8 or none (none: every pixel
// was cast), per frame c2w [3,4] row-major and intr = (fx, fy, cx, cy).
//   D = depth / acc.  USABLE iff cast, acc >= acc_min and D > 0.
//   P = (D (x - cx) / fx, -(D (y - cy) / fy), -D): the camera-space point (x right, y up, z towards the camera; get_rays directions
//     have camera z = -1, so a ray's z is the planar depth and the pixel back-projects as o + z d).  Product first, then quotient.
//   A NEIGHBOUR (x +- 1 in the row, y +- 1 in the column) counts iff it lies inside the frame, is usable, and -- only when
//     jump > 0 -- |D_nb - D| <= jump.
//   dPx = P(x+1) - P(x-1) with both neighbours, else P(x+1) - P or P - P(x-1) with one, else the pixel has no normal; dPy the same
//     over rows (y+1, y-1).
//   c = cross(dPx, dPy) (each component mul - mul), len = sqrt((cx^2 + cy^2) + cz^2).  No normal unless 0 < len < inf.
//   n = c / len, negated when n . P > 0 (so that n . (-P) > 0: the normal faces the camera).
//   space 1: n := R n with R = c2w[:3, :3], row i as (R_i0 n_x + R_i1 n_y) + R_i2 n_z: world space, the mesh turntable's.
//   colour = 0.5 n + 0.5; a pixel without a normal (unusable ones included) gets `background` in all three channels.
#pragma once
#include "sample_math.hpp"

namespace danbo {

constexpr int DEPTH_MAX_N = 320, DEPTH_MAX_DIM = 4096, DEPTH_MAX_FRAMES = 1 << 20;
constexpr int DEPTH_EINVAL = -22;      // DANBO_EINVAL of danbo_hip.h

// ---- argument rules (the entry points and the restatement reject the same) ----
DANBO_HD bool depth_level_ok(float level) { return level > 0.f && level <= 1.f; }      // (false for NaN)
DANBO_HD bool depth_composite_ok(const void* w, const void* z, int R, int n, float level, const void* ray_list, const void* ray_count,
                                 const void* depth, const void* depth_level) {
    return w && z && depth && depth_level && R >= 0 && n >= 1 && n <= DEPTH_MAX_N && depth_level_ok(level) &&
           ((ray_list == nullptr) == (ray_count == nullptr));
}
DANBO_HD bool depth_normals_ok(const void* depth, const void* acc, const void* c2w, const void* intr, int N, int H, int W, float jump,
                               int space, const void* out_rgb) {
    return depth && acc && c2w && intr && out_rgb && N >= 1 && N <= DEPTH_MAX_FRAMES && H >= 1 && H <= DEPTH_MAX_DIM && W >= 1 &&
           W <= DEPTH_MAX_DIM && jump >= 0.f && (space == 0 || space == 1);
}

// ---- per ray ----
DANBO_HD float depth_term(float w, float z) { return w == 0.f ? 0.f : mul_rn(w, z); }
// the prefix of a position from its strip's carry and the scan's value at its lane
DANBO_HD float depth_prefix(float carry, float scanned) { return add_rn(carry, scanned); }
DANBO_HD bool depth_reached(float prefix, float level) { return prefix >= level; }

// ---- per pixel ----
struct DepthVec {
    float x, y, z;
};
// the usable test of pixel `at`; *D its depth when usable
DANBO_HD bool depth_usable(const float* depth, const float* acc, const uint8_t* cast, long at, float acc_min, float* D) {
    if (cast && !cast[at]) return false;
    const float a = acc[at];
    if (!(a >= acc_min)) return false;
    *D = div_rn(depth[at], a);
    return *D > 0.f;
}
DANBO_HD DepthVec depth_point(float D, int x, int y, const float* intr) {
    DepthVec p;
    p.x = div_rn(mul_rn(D, sub_rn((float)x, intr[2])), intr[0]);
    p.y = -div_rn(mul_rn(D, sub_rn((float)y, intr[3])), intr[1]);
    p.z = -D;
    return p;
}
DANBO_HD DepthVec depth_sub(DepthVec a, DepthVec b) { return DepthVec{sub_rn(a.x, b.x), sub_rn(a.y, b.y), sub_rn(a.z, b.z)}; }
DANBO_HD float depth_dot(float a0, float a1, float a2, DepthVec b) {
    return add_rn(add_rn(mul_rn(a0, b.x), mul_rn(a1, b.y)), mul_rn(a2, b.z));
}
// the neighbour (xn, yn) of a pixel of depth D: counted or not; *p its point when counted
DANBO_HD bool depth_neighbour(const float* depth, const float* acc, const uint8_t* cast, long frame, int H, int W, int xn, int yn,
                              float acc_min, float jump, float D, const float* intr, DepthVec* p) {
    if (xn < 0 || xn >= W || yn < 0 || yn >= H) return false;
    float Dn;
    if (!depth_usable(depth, acc, cast, frame + (long)yn * W + xn, acc_min, &Dn)) return false;
    if (jump > 0.f && fabsf(sub_rn(Dn, D)) > jump) return false;
    *p = depth_point(Dn, xn, yn, intr);
    return true;
}
// the difference along one axis from the two neighbours (before: -1, after: +1) -> false: none
DANBO_HD bool depth_diff(bool has_b, DepthVec b, bool has_a, DepthVec a, DepthVec p, DepthVec* d) {
    if (has_a && has_b) *d = depth_sub(a, b);
    else if (has_a) *d = depth_sub(a, p);
    else if (has_b) *d = depth_sub(p, b);
    else return false;
    return true;
}
// pixel (x, y) of frame n: its colour into rgb[3] -> 1 with a normal, 0 without (rgb = background)
DANBO_HD int depth_normal_pixel(const float* depth, const float* acc, const uint8_t* cast, const float* c2w, const float* intr4, int n,
                                int H, int W, int x, int y, float acc_min, float jump, int space, float background, float* rgb) {
    rgb[0] = rgb[1] = rgb[2] = background;
    const long frame = (long)n * H * W;
    const float* intr = intr4 + 4 * (long)n;
    float D;
    if (!depth_usable(depth, acc, cast, frame + (long)y * W + x, acc_min, &D)) return 0;
    const DepthVec p = depth_point(D, x, y, intr);
    DepthVec pb = p, pa = p, dx, dy;
    bool hb = depth_neighbour(depth, acc, cast, frame, H, W, x - 1, y, acc_min, jump, D, intr, &pb);
    bool ha = depth_neighbour(depth, acc, cast, frame, H, W, x + 1, y, acc_min, jump, D, intr, &pa);
    if (!depth_diff(hb, pb, ha, pa, p, &dx)) return 0;
    pb = p, pa = p;
    hb = depth_neighbour(depth, acc, cast, frame, H, W, x, y - 1, acc_min, jump, D, intr, &pb);
    ha = depth_neighbour(depth, acc, cast, frame, H, W, x, y + 1, acc_min, jump, D, intr, &pa);
    if (!depth_diff(hb, pb, ha, pa, p, &dy)) return 0;
    DepthVec c;
    c.x = sub_rn(mul_rn(dx.y, dy.z), mul_rn(dx.z, dy.y));
    c.y = sub_rn(mul_rn(dx.z, dy.x), mul_rn(dx.x, dy.z));
    c.z = sub_rn(mul_rn(dx.x, dy.y), mul_rn(dx.y, dy.x));
    const float len = sqrtf(add_rn(add_rn(mul_rn(c.x, c.x), mul_rn(c.y, c.y)), mul_rn(c.z, c.z)));
    if (!(len > 0.f && len < INFINITY)) return 0;
    DepthVec v{div_rn(c.x, len), div_rn(c.y, len), div_rn(c.z, len)};
    if (depth_dot(v.x, v.y, v.z, p) > 0.f) v = DepthVec{-v.x, -v.y, -v.z};
    if (space == 1) {
        const float* R = c2w + 12 * (long)n;
        v = DepthVec{depth_dot(R[0], R[1], R[2], v), depth_dot(R[4], R[5], R[6], v), depth_dot(R[8], R[9], R[10], v)};
    }
    rgb[0] = add_rn(mul_rn(0.5f, v.x), 0.5f);
    rgb[1] = add_rn(mul_rn(0.5f, v.y), 0.5f);
    rgb[2] = add_rn(mul_rn(0.5f, v.z), 0.5f);
    return 1;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------------------
// Serial restatement (host): the same two calls as danbo_depth_composite_fwd / danbo_depth_normals without the stream, one ray
// and one pixel after the other.  Returns 0, or -22 for a rejected argument.

// THE SCAN TREE of the head of this file, on 64 values in place
inline void depth_wave_scan(float* x) {
    float t[64];
    for (int d = 1; d <= 8; d <<= 1) {
        for (int l = 0; l < 64; ++l) t[l] = (l % 16 >= d) ? x[l - d] : 0.f;
        for (int l = 0; l < 64; ++l) x[l] = add_rn(x[l], t[l]);
    }
    for (int l = 0; l < 64; ++l) t[l] = ((l / 16) & 1) ? x[16 * (l / 16) - 1] : 0.f;
    for (int l = 0; l < 64; ++l) x[l] = add_rn(x[l], t[l]);
    for (int l = 0; l < 64; ++l) t[l] = (l >= 32) ? x[31] : 0.f;
    for (int l = 0; l < 64; ++l) x[l] = add_rn(x[l], t[l]);
}

inline void depth_ray_host(const float* w, const float* z, int n, float level, float* depth, float* depth_level) {
    float part[64];
    for (int l = 0; l < 64; ++l) {
        part[l] = 0.f;
        for (int k = l; k < n; k += 64) part[l] = add_rn(part[l], depth_term(w[k], z[k]));
    }
    depth_wave_scan(part);
    *depth = part[63];
    float carry = 0.f;
    *depth_level = 0.f;
    for (int base = 0; base < n; base += 64) {
        float s[64];
        for (int l = 0; l < 64; ++l) s[l] = base + l < n ? w[base + l] : 0.f;
        depth_wave_scan(s);
        for (int l = 0; l < 64 && base + l < n; ++l)
            if (depth_reached(depth_prefix(carry, s[l]), level)) {
                *depth_level = z[base + l];
                return;
            }
        carry = depth_prefix(carry, s[63]);
    }
}

inline int depth_composite_host(const float* weights, const float* z_sorted, int R, int n, float level, const int32_t* ray_list,
                                const int32_t* ray_count, float* depth, float* depth_level) {
    if (!depth_composite_ok(weights, z_sorted, R, n, level, ray_list, ray_count, depth, depth_level)) return DEPTH_EINVAL;
    int count = R;
    if (ray_list) count = *ray_count < 0 ? 0 : (*ray_count < R ? *ray_count : R);
    for (int i = 0; i < count; ++i) {
        int r = i;
        if (ray_list) r = ray_list[i] < 0 ? 0 : (ray_list[i] < R ? ray_list[i] : R - 1);
        depth_ray_host(weights + (size_t)r * n, z_sorted + (size_t)r * n, n, level, depth + r, depth_level + r);
    }
    return 0;
}

inline int depth_normals_host(const float* depth, const float* acc, const uint8_t* cast, const float* c2w, const float* intr, int N, int H,
                              int W, float acc_min, float jump, int space, float background, float* out_rgb, uint8_t* out_valid) {
    if (!depth_normals_ok(depth, acc, c2w, intr, N, H, W, jump, space, out_rgb)) return DEPTH_EINVAL;
    for (int n = 0; n < N; ++n)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long at = ((long)n * H + y) * W + x;
                const int ok = depth_normal_pixel(depth, acc, cast, c2w, intr, n, H, W, x, y, acc_min, jump, space, background,
                                                  out_rgb + 3 * at);
                if (out_valid) out_valid[at] = (uint8_t)ok;
            }
    return 0;
}
#endif  // !__HIPCC__

}  // namespace danbo
