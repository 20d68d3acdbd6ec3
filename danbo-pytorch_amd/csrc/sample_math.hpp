// Per-item arithmetic of the sampling / transform / gather / composite stages.
//
// Everything here is plain scalar C++ marked DANBO_HD so that the very same code is
//   * inlined into the gfx950 kernels (hipcc), and
//   * compiled for the host by g++ (tests/host_emu.cpp) so the CPU test-suite can check the
//     kernel bodies against the numpy oracle without a GPU.
// Operation order is part of the contract: the transform chain and the in-volume test use
// separately rounded fp32 mul/add (never FMA) so that GPU, host build and
// oracle/danbo_oracle.py agree bit-for-bit on the in-volume mask.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DANBO_HD __host__ __device__ __forceinline__
#else
#define DANBO_HD inline
#endif

namespace danbo {

constexpr int J = 24;
constexpr int FEAT = 15;
constexpr int VOXF = 5;
constexpr int VRES = 16;
constexpr int VOL = 240;

// ---- exactly-rounded, never-contracted fp32 primitives --------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
DANBO_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
DANBO_HD float add_rn(float a, float b) { return __fadd_rn(a, b); }
DANBO_HD float sub_rn(float a, float b) { return __fsub_rn(a, b); }
DANBO_HD float div_rn(float a, float b) { return __fdiv_rn(a, b); }
DANBO_HD double dmul_rn(double a, double b) { return __dmul_rn(a, b); }
DANBO_HD double dadd_rn(double a, double b) { return __dadd_rn(a, b); }
#else
// host build is compiled with -ffp-contract=off
DANBO_HD float mul_rn(float a, float b) { volatile float r = a * b; return r; }
DANBO_HD float add_rn(float a, float b) { volatile float r = a + b; return r; }
DANBO_HD float sub_rn(float a, float b) { volatile float r = a - b; return r; }
DANBO_HD float div_rn(float a, float b) { volatile float r = a / b; return r; }
DANBO_HD double dmul_rn(double a, double b) { volatile double r = a * b; return r; }
DANBO_HD double dadd_rn(double a, double b) { volatile double r = a + b; return r; }
#endif

// torch.norm(x, dim=-1) of a 2- / 3-vector: the reduction's step is acc + x*x CONTRACTED to one fma (ATen NormTwoOps; pinned on
// the reference's tensors in the build container: sqrt(fma(z,z,fma(y,y,x*x))) equals torch's result on every one of 98 304 rows,
// the separately rounded sum on 95 % of them) -- the only place of this file where an FMA is part of the contract
DANBO_HD float norm3_torch(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, mul_rn(x, x)))); }
DANBO_HD float norm2_torch(float x, float y) { return sqrtf(fmaf(y, y, mul_rn(x, x))); }

// torch.linspace(0,1,n)[i] in fp32 (symmetric evaluation around the midpoint)
DANBO_HD float linspace01(int i, int n) {
    if (n <= 1) return 0.f;
    const float step = div_rn(1.0f, (float)(n - 1));
    return (i < n / 2) ? mul_rn((float)i, step) : sub_rn(1.0f, mul_rn((float)(n - 1 - i), step));
}

// sample_from_lineseg, perturb = 0:  near*(1-t) + far*t
DANBO_HD float coarse_z(float nr, float fr, int s, int S) {
    const float t = linspace01(s, S);
    return add_rn(mul_rn(nr, sub_rn(1.0f, t)), mul_rn(fr, t));
}

// coarse depth s of a ray: coarse_z, or (t_rand: one uniform per sample, read at [m]) the stratified jitter between the mid-points
// to its neighbours (ray_utils.py:233-248).  One definition for k_coarse_samples* (k_sample.hip) and k_cull_rays (k_cull_rays.hip)
DANBO_HD float coarse_sample(float n_, float f_, int s, int S, const float* __restrict__ t_rand, long m) {
    float v = coarse_z(n_, f_, s, S);
    if (t_rand) {  // stratified jitter (ray_utils.py:233-248)
        const float zp = s > 0 ? coarse_z(n_, f_, s - 1, S) : v;
        const float zn = s + 1 < S ? coarse_z(n_, f_, s + 1, S) : v;
        const float lower = s > 0 ? mul_rn(0.5f, add_rn(v, zp)) : v;
        const float upper = s + 1 < S ? mul_rn(0.5f, add_rn(zn, v)) : v;
        v = add_rn(lower, mul_rn(sub_rn(upper, lower), t_rand[m]));
    }
    return v;
}

// pts = o + d*z (two roundings), core/raycasters.py:463
DANBO_HD void sample_point(const float* o, const float* d, float z, float* p) {
    p[0] = add_rn(o[0], mul_rn(d[0], z));
    p[1] = add_rn(o[1], mul_rn(d[1], z));
    p[2] = add_rn(o[2], mul_rn(d[2], z));
}

// pose of sample m of an [R, S] batch that holds G poses, spp = (R / G) * S samples each (clamped like the rays' r / (R / G))
DANBO_HD int pose_of_sample(long m, long spp, int G) { return (int)(m / spp < (long)G - 1 ? m / spp : (long)G - 1); }
// the point of sample m: pts[m] where the caller brings points, o + d z of ray m / S otherwise
DANBO_HD void point_of_sample(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ z,
                              const float* __restrict__ pts, long m, int S, float* p) {
    if (pts != nullptr) {
        p[0] = pts[3 * m]; p[1] = pts[3 * m + 1]; p[2] = pts[3 * m + 2];
    } else {
        const int r = (int)(m / S);
        const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
        const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
        sample_point(o, d, z[m], p);
    }
}

// (m0*x + m1*y) + m2*z for the three rows of a row-major 4x4: the rotation alone, what a DIRECTION takes (torch.matmul's
// sequential-k order).  q must not alias d.
DANBO_HD void rotate_unfused(const float* M, const float* d, float* q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* r = M + 4 * k;
        q[k] = add_rn(add_rn(mul_rn(r[0], d[0]), mul_rn(r[1], d[1])), mul_rn(r[2], d[2]));
    }
}
// ((m0*x + m1*y) + m2*z) + m3: rotate_unfused's sum plus the translation column (only rows 0..2 read).  Restated, not a call
// of rotate_unfused: that form moved the assembly of the cull / gather / assignment kernels (profiles/one_definition_measured.txt)
DANBO_HD void affine_unfused(const float* M, const float* p, float* q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* r = M + 4 * k;
        float s = add_rn(mul_rn(r[0], p[0]), mul_rn(r[1], p[1]));
        s = add_rn(s, mul_rn(r[2], p[2]));
        q[k] = add_rn(s, r[3]);
    }
}
// F.normalize(d, p = 2, eps = 1e-12) of a 3-vector, in place: d / max(|d|, 1e-12)
DANBO_HD void normalize3(float* d) {
    const float den = fmaxf(norm3_torch(d[0], d[1], d[2]), 1e-12f);
    d[0] = div_rn(d[0], den); d[1] = div_rn(d[1], den); d[2] = div_rn(d[2], den);
}

// world -> bone-local -> bone-aligned  (core/encoders.py:288-303,442-444)
DANBO_HD void bone_local(const float* skt, const float* align, const float* p, float* pt) {
    float pl[3];
    affine_unfused(skt, p, pl);
    affine_unfused(align, pl, pt);
}

// !invalid of gnn_backbone.py:808 in the division-free form  |p_k| <= |scale_k|
DANBO_HD bool in_volume(const float* pt, const float* abs_scale) {
    return !(fabsf(pt[0]) > abs_scale[0] || fabsf(pt[1]) > abs_scale[1] || fabsf(pt[2]) > abs_scale[2]);
}

// window = exp(-2 * sum x^6), gnn_backbone.py:803-804
DANBO_HD float coord_window(const float* x) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x2 = mul_rn(x[k], x[k]);
        acc = add_rn(acc, mul_rn(mul_rn(x2, x2), x2));
    }
    return expf(mul_rn(-2.0f, acc));
}

// one bone's 15 windowed features from its 240-float factorised volume
// layout vol[f*48 + r*3 + axis]; out[f*3 + axis]   (misc.py:331-351, gnn_backbone.py:810-826)
template <typename VolPtr>
DANBO_HD void gather_bone_features(VolPtr vol, const float* pt, const float* abs_scale, float* out) {
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = div_rn(pt[k], abs_scale[k]);
    const float win = coord_window(x);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float iy = div_rn(sub_rn(mul_rn(add_rn(x[k], 1.0f), (float)VRES), 1.0f), 2.0f);
        const float fl = floorf(iy);
        const float w1 = sub_rn(iy, fl);
        const float w0 = sub_rn(1.0f, w1);
        // clamp before the int conversion: far-away samples have |iy| ~ 1e3..1e6
        const float flc = fminf(fmaxf(fl, -2.0f), (float)VRES + 1.0f);
        const int y0 = (int)flc;
        const int y1 = y0 + 1;
        const bool ok0 = (y0 >= 0) && (y0 < VRES);
        const bool ok1 = (y1 >= 0) && (y1 < VRES);
        const int c0 = ok0 ? y0 : 0;
        const int c1 = ok1 ? y1 : 0;
#pragma unroll
        for (int f = 0; f < VOXF; ++f) {
            const float v0 = ok0 ? vol[f * (VRES * 3) + c0 * 3 + k] : 0.f;
            const float v1 = ok1 ? vol[f * (VRES * 3) + c1 * 3 + k] : 0.f;
            const float s = add_rn(mul_rn(v0, w0), mul_rn(v1, w1));
            out[f * 3 + k] = mul_rn(s, win);
        }
    }
}

DANBO_HD float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// What the reference makes of a sigmoid s, a sample's colour (core/networks/nerf.py:281-347) and a bone's assignment probability
// alike: s * 1.002 - 0.001, two roundings.  _bwd: the gradient `up` of that taken to the logit, ((up * 1.002) * s) * (1 - s)
constexpr float SIGMOID_GAIN = 1.002f, SIGMOID_SHIFT = 0.001f;
DANBO_HD float sigmoid_affine(float s) { return sub_rn(mul_rn(s, SIGMOID_GAIN), SIGMOID_SHIFT); }
DANBO_HD float sigmoid_affine_bwd(float up, float s) { return up * SIGMOID_GAIN * s * (1.0f - s); }
DANBO_HD float rgb_of_logit(float x) { return sigmoid_affine(sigmoidf_(x)); }
// disparity of a ray from its weighted depth and accumulated weight: 1 / max(1e-10, depth / (acc + 1e-10)), 0 where
// torch.isclose(acc, 0): |acc| <= 1e-8 + 1e-5 * 0
DANBO_HD float disp_of(float depth, float acc) {
    const float dsp = div_rn(1.0f, fmaxf(1e-10f, div_rn(depth, add_rn(acc, 1e-10f))));
    return fabsf(acc) <= 1e-8f ? 0.f : dsp;
}

// ---- density activation (get_density_fn, core/raycasters.py:192-200): relu(x) or softplus(x - shift) ----
// A compile-time parameter of every composite (DA); the shift is a run-time float that the relu forms never read.
constexpr int DENSITY_RELU = 0;
constexpr int DENSITY_SOFTPLUS = 1;
// log(1 + e^t) for t <= 20 (clamped: the caller's select drops the other side, and no inf or NaN is formed on the way).
// Device: log(u) e / (u - 1) with u = fl(1 + e) -- the rounding of 1 + e cancels in the quotient (e itself where u == 1), a few
// ulp like log1p.  Not the device library's log1pf: it sums its two-float result with a v_pk_add_f32 ... op_sel:[0,1], the packed
// operand selection that is wrong on gfx950 beside MFMA wavefronts (common.hpp, DANBO_NO_PK_F32), and a kernel template cannot
// carry that attribute for one of its instantiations only.
DANBO_HD float log1p_exp(float t) {
    const float e = expf(fminf(t, 20.f));
#if defined(__HIP_DEVICE_COMPILE__)
    const float u = add_rn(1.0f, e);
    return u == 1.0f ? e : mul_rn(logf(u), div_rn(e, sub_rn(u, 1.0f)));
#else
    return log1pf(e);
#endif
}
// F.softplus(x - shift, beta=1) with torch's threshold 20.  A NaN logit stays NaN, as in torch (the clamp inside log1p_exp would
// drop it; relu's fmaxf makes it 0, as before)
template <int DA>
DANBO_HD float density_act(float x, float shift) {
    if constexpr (DA == DENSITY_SOFTPLUS) {
        const float t = sub_rn(x, shift);
        return (t > 20.f || t != t) ? t : log1p_exp(t);
    } else {
        return fmaxf(x, 0.f);
    }
}
// d density_act / d x: [x > 0] for relu; sigmoid(x - shift) (1 beyond the threshold) for softplus
template <int DA>
DANBO_HD float density_act_grad(float x, float shift) {
    if constexpr (DA == DENSITY_SOFTPLUS) {
        const float t = sub_rn(x, shift);
        return t > 20.f ? 1.0f : sigmoidf_(t);
    } else {
        return x > 0.f ? 1.0f : 0.f;
    }
}

// ---- get_near_far_in_cylinder, one ray, before the NaN back-fill ----------------------
// core/utils/ray_utils.py:294-329.  Returns false when the ray misses the cylinder.
DANBO_HD bool cylinder_bounds(const float* o, const float* d, const float* cyl, float near0, float far0,
                              float* nr, float* fr) {
    const float nx = add_rn(o[0], mul_rn(d[0], near0)), nz = add_rn(o[2], mul_rn(d[2], near0));
    const float fx = add_rn(o[0], mul_rn(d[0], far0)), fz = add_rn(o[2], mul_rn(d[2], far0));
    const float ncx = sub_rn(cyl[0], nx), ncz = sub_rn(cyl[1], nz);
    const float nfx = sub_rn(fx, nx), nfz = sub_rn(fz, nz);
    const float nf_norm = norm2_torch(nfx, nfz);
    const float scale = norm2_torch(d[0], d[2]);
    const float cross = sub_rn(mul_rn(ncx, nfz), mul_rn(ncz, nfx));
    const float dist = div_rn(fabsf(cross), nf_norm);
    const float rad = cyl[2];
    const float q2 = sub_rn(mul_rn(rad, rad), mul_rn(dist, dist));
    const float Q = sqrtf(q2);  // NaN when the ray misses
    const float K = div_rn(add_rn(mul_rn(ncx, nfx), mul_rn(ncz, nfz)), nf_norm);
    const float mask = (Q < K) ? 1.0f : 0.0f;
    *nr = add_rn(near0, div_rn(mul_rn(mask, sub_rn(K, Q)), scale));
    *fr = add_rn(near0, div_rn(add_rn(K, Q), scale));
    return !(Q != Q);
}

// ---- per-bone box near/far (fast configs), one ray x one bone --------------------------
// core/raycasters.py:659-697 + core/utils/ray_utils.py:383-417.  Returns true when exactly
// two of the six plane hits are inside the (bound + eps) box; *smin/*smax = their steps.
DANBO_HD bool bone_box_steps(const float* skt, const float* align, const float* abs_scale,
                             const float* o, const float* d, float* smin, float* smax) {
    const float bound = 1.3f, eps = 1e-4f;
    float ol[3], ot[3], dl[3], dt[3];
    // origin: full affine (affine_unfused); direction: rotation only (rotate_unfused).  Restated: either call moved k_box_bounds'
    // registers (profiles/one_definition_measured.txt)
    for (int k = 0; k < 3; ++k) {
        const float* r = skt + 4 * k;
        ol[k] = add_rn(add_rn(add_rn(mul_rn(r[0], o[0]), mul_rn(r[1], o[1])), mul_rn(r[2], o[2])), r[3]);
        dl[k] = add_rn(add_rn(mul_rn(r[0], d[0]), mul_rn(r[1], d[1])), mul_rn(r[2], d[2]));
    }
    for (int k = 0; k < 3; ++k) {
        const float* r = align + 4 * k;
        ot[k] = add_rn(add_rn(add_rn(mul_rn(r[0], ol[0]), mul_rn(r[1], ol[1])), mul_rn(r[2], ol[2])), r[3]);
        dt[k] = add_rn(add_rn(mul_rn(r[0], dl[0]), mul_rn(r[1], dl[1])), mul_rn(r[2], dl[2]));
    }
    float os[3], ds[3];
    for (int k = 0; k < 3; ++k) { os[k] = div_rn(ot[k], abs_scale[k]); ds[k] = div_rn(dt[k], abs_scale[k]); }
    const float dnorm = norm3_torch(dt[0], dt[1], dt[2]);
    int hits = 0;
    float lo = INFINITY, hi = -INFINITY;
    const float lim = bound + eps;
    for (int side = 0; side < 2; ++side) {
        for (int ax = 0; ax < 3; ++ax) {
            const double b = side ? (double)bound : -(double)bound;
            const double t = (b - (double)os[ax]) / (double)ds[ax];
            float p[3];
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                p[k] = (float)dadd_rn(dmul_rn(t, (double)ds[k]), (double)os[k]);   // torch: t * d + o as two float64 ops
                ok = ok && (p[k] <= lim) && (p[k] >= -lim);
            }
            if (ok) {
                ++hits;
                float df[3];
                for (int k = 0; k < 3; ++k) df[k] = sub_rn(mul_rn(p[k], abs_scale[k]), ot[k]);
                const float step = div_rn(norm3_torch(df[0], df[1], df[2]), dnorm);
                lo = fminf(lo, step);
                hi = fmaxf(hi, step);
            }
        }
    }
    *smin = lo;
    *smax = hi;
    return hits == 2;
}

// ---- pdf weight of importance bin i (core/utils/ray_utils.py:271-279 + sample_pdf's + 1e-5) ------------------------
// TWO = false (one network, is_only):  0.5 (max(w_i, w_i+1) + max(w_i+1, w_i+2)) + 0.01 + 1e-5
// TWO = true  (separate fine network):  w_i+1 + 1e-5
// A compile-time choice: the single-network instantiations are the code they were before the two-network form existed.
template <bool TWO>
DANBO_HD float pdf_weight(float w0, float w1, float w2) {
    if (TWO) return add_rn(w1, 1e-5f);
    return add_rn(add_rn(mul_rn(0.5f, add_rn(fmaxf(w0, w1), fmaxf(w1, w2))), 0.01f), 1e-5f);
}

// ---- inverse CDF of one draw (sample_pdf, core/utils/ray_utils.py:159-203) ----
// lo = searchsorted(cdf, u, right=True) over the ncdf bin edges; the edges on either side of the draw, clamped to the table
DANBO_HD int cdf_below(int lo) { return lo - 1 > 0 ? lo - 1 : 0; }
DANBO_HD int cdf_above(int lo, int ncdf) { return lo < ncdf - 1 ? lo : ncdf - 1; }
// the depth of draw uk between the bin mid-points b0, b1 whose cdf values are c0, c1 (a bin narrower than 1e-5 counts as 1)
DANBO_HD float inverse_cdf_point(float uk, float c0, float c1, float b0, float b1) {
    float denom = sub_rn(c1, c0);
    if (denom < 1e-5f) denom = 1.0f;
    const float t = div_rn(sub_rn(uk, c0), denom);
    return add_rn(b0, mul_rn(t, sub_rn(b1, b0)));
}

// rank rule of the merged order inside ONE of the two sequences: (za, ia) comes before (zb, ib) in a stable sort by depth
DANBO_HD bool sorts_before(float za, int ia, float zb, int ib) { return (za < zb) || (za == zb && ia < ib); }

// ---- importance sampling of one ray (pdf + inverse CDF + stable merge) --------------------
// core/utils/ray_utils.py:159-203,257-291.  z, w: [S]; u: [Sf] or NULL (linspace);
// scratch cdf: [S-1] floats... caller provides `cdf` with room for S floats.
// TWO: the pdf of the two-network mode (pdf_weight).
template <bool TWO = false>
DANBO_HD void importance_ray(const float* z, const float* w, int S, int Sf, const float* u, float* cdf,
                             float* z_fine, float* z_sorted, int32_t* sorted_idx) {
    const int nb = S - 2;  // number of pdf bins; bin edges are the S-1 midpoints
    float sum = 0.f;
    for (int i = 0; i < nb; ++i) {
        const float dw = pdf_weight<TWO>(w[i], w[i + 1], w[i + 2]);
        cdf[i + 1] = dw;
        sum = add_rn(sum, dw);
    }
    cdf[0] = 0.f;
    float run = 0.f;
    for (int i = 0; i < nb; ++i) {
        run = add_rn(run, div_rn(cdf[i + 1], sum));
        cdf[i + 1] = run;
    }
    const int ncdf = nb + 1;  // == S-1 == number of bin edges
    for (int k = 0; k < Sf; ++k) {
        const float uk = u ? u[k] : linspace01(k, Sf);
        // searchsorted(cdf, u, right=True): first index with cdf[idx] > u
        int lo_i = 0, hi_i = ncdf;
        while (lo_i < hi_i) {
            const int mid = (lo_i + hi_i) >> 1;
            if (cdf[mid] > uk) hi_i = mid; else lo_i = mid + 1;
        }
        const int below = cdf_below(lo_i), above = cdf_above(lo_i, ncdf);
        const float b0 = mul_rn(0.5f, add_rn(z[below + 1], z[below]));
        const float b1 = mul_rn(0.5f, add_rn(z[above + 1], z[above]));
        z_fine[k] = inverse_cdf_point(uk, cdf[below], cdf[above], b0, b1);
    }
    // stable merge, coarse first on ties (torch.sort of cat([z, z_fine]))
    int a = 0, b = 0;
    for (int i = 0; i < S + Sf; ++i) {
        const bool take_a = (b >= Sf) || (a < S && z[a] <= z_fine[b]);
        if (take_a) { z_sorted[i] = z[a]; sorted_idx[i] = a; ++a; }
        else { z_sorted[i] = z_fine[b]; sorted_idx[i] = S + b; ++b; }
    }
}

// ---- alpha compositing of one ray, sequential form (core/networks/nerf.py:281-347) -----
// DA / shift: the density activation (density_act above); the default is relu, which never reads the shift
template <int DA = DENSITY_RELU>
DANBO_HD void composite_ray(const float* raw, const float* z, const float* d, int S, float B, const float* noise,
                            float* rgb_map, float* disp, float* acc_out, float* weights, float* alpha_out, float shift = 0.f) {
    const float dn = norm3_torch(d[0], d[1], d[2]);
    float T = 1.0f, r = 0.f, g = 0.f, b = 0.f, depth = 0.f, acc = 0.f;
    for (int s = 0; s < S; ++s) {
        const float dz = (s + 1 < S) ? sub_rn(z[s + 1], z[s]) : 1e10f;
        const float dist = mul_rn(dz, dn);
        float sg = div_rn(raw[4 * s + 3], B);
        if (noise) sg = add_rn(sg, noise[s]);
        sg = density_act<DA>(sg, shift);
        const float al = sub_rn(1.0f, expf(-mul_rn(sg, dist)));
        const float w = mul_rn(al, T);
        T = mul_rn(T, add_rn(sub_rn(1.0f, al), 1e-10f));
        const float cr = rgb_of_logit(raw[4 * s + 0]);
        const float cg = rgb_of_logit(raw[4 * s + 1]);
        const float cb = rgb_of_logit(raw[4 * s + 2]);
        r = add_rn(r, mul_rn(w, cr));
        g = add_rn(g, mul_rn(w, cg));
        b = add_rn(b, mul_rn(w, cb));
        depth = add_rn(depth, mul_rn(w, z[s]));
        acc = add_rn(acc, w);
        if (weights) weights[s] = w;
        if (alpha_out) alpha_out[s] = al;
    }
    rgb_map[0] = r; rgb_map[1] = g; rgb_map[2] = b;
    *disp = disp_of(depth, acc);
    *acc_out = fminf(acc, 1.0f);
}

}  // namespace danbo
