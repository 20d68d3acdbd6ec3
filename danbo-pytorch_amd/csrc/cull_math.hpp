// Device code of the in-volume test (K1a) that more than one translation unit inlines: the packed-fp32 transform chain, the slack
// of the candidate-bone interval and the per-pair bone loop.  k_bone_cull (k_sample.hip) and k_cull_rays (k_cull_rays.hip) call
// these very functions, so their in-volume words agree bit for bit for the same depths.  gfx950 device code only.
#pragma once
#include "common.hpp"

namespace danbo {

typedef float v2f __attribute__((ext_vector_type(2)));

// li / S with inv_S = 1 / (float)S, exact for li < 2^22: the ray of a workgroup's local sample index without an integer division
__device__ __forceinline__ int ray_of_local(int li, int S, float inv_S) {
    int q = (int)((float)li * inv_S);
    q -= (q * S > li) ? 1 : 0;
    q += ((q + 1) * S <= li) ? 1 : 0;
    return q;
}

// ((m0*x + m1*y) + m2*z) + m3 for two points at once; every packed op rounds each half like the
// scalar __fmul_rn / __fadd_rn chain of affine_unfused() (contraction disabled).
// The matrix entries are BROADCAST over the pair.  Left to the compiler that is v_pk_mul_f32 x, m op_sel:[0,1] for the odd entries --
// the low half from SRC1's high dword: the one operand selection that is wrong on gfx950 beside MFMA wavefronts (common.hpp,
// DANBO_NO_PK_F32; without packed instructions this kernel takes 102 instead of 55 us).  Written out with the matrix pair as SRC0, whose
// high-dword selection is exact (tools/probe/cview_probe.hip: 0 of 2.7e10), the products and sums are the same IEEE operations.
template <int HI>
__device__ __forceinline__ v2f pk_mul_bcast(v2f m, v2f x) {     // m[HI] * x
    v2f d;
    if (HI) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(d) : "v"(m), "v"(x));
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(d) : "v"(m), "v"(x));
    return d;
}
__device__ __forceinline__ v2f pk_add(v2f a, v2f b) {
    v2f d;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ v2f pk_add_bcast_hi(v2f m, v2f a) {  // m[1] + a
    v2f d;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(d) : "v"(m), "v"(a));
    return d;
}
__device__ __forceinline__ void affine_pk(const float* M, v2f x, v2f y, v2f z, v2f* q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 r = *reinterpret_cast<const float4*>(M + 4 * k);
        const v2f m01 = {r.x, r.y}, m23 = {r.z, r.w};
        v2f s = pk_add(pk_mul_bcast<0>(m01, x), pk_mul_bcast<1>(m01, y));
        s = pk_add(s, pk_mul_bcast<0>(m23, z));
        q[k] = pk_add_bcast_hi(m23, s);
    }
}

// Slack of the interval a ray's bone mask holds for: a depth within [t_lo - slack, t_hi + slack] takes the mask's candidates, any
// other depth all bones (half of segment_misses_bone's pad)
__device__ __forceinline__ float mask_slack(float lo, float hi) { return 5e-5f * fmaxf(fabsf(lo), fabsf(hi)); }

// In-volume words of two points (x, y lanes of px / py / pz) against the bones of `need` (wave-uniform): world -> bone-local ->
// bone-aligned by two affine_pk, then |p_k| <= |scale_k| (in_volume of sample_math.hpp).  sk: the pose's [24][16] matrices,
// s_align [24][16], s_scale [24][4], all in LDS.  Bits outside `need` stay as they were.
__device__ __forceinline__ void in_volume_pk(const float* sk, const float* s_align, const float* s_scale, uint32_t need,
                                             v2f px, v2f py, v2f pz, uint32_t& ba, uint32_t& bb) {
    while (need) {
        const int j = __builtin_ctz(need);
        need &= need - 1u;
        v2f l[3], t[3];
        affine_pk(sk + 16 * j, px, py, pz, l);
        affine_pk(s_align + 16 * j, l[0], l[1], l[2], t);
        const float* sc = s_scale + 4 * j;
        const bool ina = !(fabsf(t[0].x) > sc[0] || fabsf(t[1].x) > sc[1] || fabsf(t[2].x) > sc[2]);
        const bool inb = !(fabsf(t[0].y) > sc[0] || fabsf(t[1].y) > sc[1] || fabsf(t[2].y) > sc[2]);
        ba |= (ina ? 1u : 0u) << j;
        bb |= (inb ? 1u : 0u) << j;
    }
}

}  // namespace danbo
