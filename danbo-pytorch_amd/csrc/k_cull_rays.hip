// K1a over the LISTED rays of a frame (danbo_flat_rays' list): depths, in-volume words and the compacted row list of those rays
// only.  A frame whose rays of constants got their outputs from k_flat_rays reads neither depths nor in-volume words of those rays
// ("Rays"), so nothing is made, tested or stored for them here: k_coarse_samples4 + k_bone_cull walk all
// R x S samples, this walks n x S.  The per-sample arithmetic is k_bone_cull's own (cull_math.hpp, sample_math.hpp): the same
// words for the same depths.  gfx950 only.
#include "common.hpp"
#include "../../include/danbo_cull.h"
#include "cull_math.hpp"

namespace danbo {

constexpr int CR_BLOCK = 256;
constexpr int CR_PAIR = 2 * CR_BLOCK;        // samples of one turn of a workgroup: two per thread, CR_BLOCK apart (affine_pk's pair)
constexpr int CR_MAX_RPW = 384;              // rays a workgroup may take (its per-ray records live in LDS)
constexpr int CR_MAX_SAMPLES = 16384;        // samples a workgroup may take: one 64-bit ballot per 64 of them
constexpr int CR_MAX_BALLOTS = CR_MAX_SAMPLES / 64;

// Workgroup b takes the entries [b * rpw, (b + 1) * rpw) of ray_list (clamped as the composites clamp them) and ALL samples of
// those rays: local sample li = i * S + s is sample s of the workgroup's i-th ray.  Three steps:
//   1. every pair of samples: depth (COARSE: made here with coarse_sample and stored to z; otherwise read from z), candidate
//      bones from the ray's mask, the in-volume test, the word to valid_bits, the wavefront's ballot of non-zero words to LDS;
//   2. one wavefront scans the ballots' counts, ONE atomicAdd(count, run) draws the workgroup's rows (none if it has no row);
//   3. every sample with a non-zero word writes its index to its row: the rows of a workgroup are ordered by li -- ray-major,
//      ascending sample index inside a ray, as K2's bone skipping and K3's per-ray loads want them.
// No workgroup waits for another.  Unlisted rays: nothing read, nothing written.
template <bool COARSE>
__global__ __launch_bounds__(CR_BLOCK) void k_cull_rays(const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count,
                                                        const uint32_t* __restrict__ ray_mask, const float* __restrict__ t_lo,
                                                        const float* __restrict__ t_hi, const float* __restrict__ rays_o,
                                                        const float* __restrict__ rays_d, const float* __restrict__ skts,
                                                        const float* __restrict__ align, const float* __restrict__ axis_scale,
                                                        const float* __restrict__ near, const float* __restrict__ far,
                                                        float* __restrict__ z /* COARSE: out; otherwise in */, int R, int S, int rpw,
                                                        uint32_t* __restrict__ valid_bits, int32_t* __restrict__ list,
                                                        int32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) float s_align[J * 16];
    __shared__ __attribute__((aligned(16))) float s_scale[J * 4];
    __shared__ __attribute__((aligned(16))) float s_skt[J * 16];
    __shared__ float4 s_o[CR_MAX_RPW];       // origin, near
    __shared__ float4 s_d[CR_MAX_RPW];       // direction, far
    __shared__ float4 s_m[CR_MAX_RPW];       // t_lo - slack, t_hi + slack, mask, ray (the last two as bit patterns)
    __shared__ unsigned long long s_ball[CR_MAX_BALLOTS];
    __shared__ int s_off[CR_MAX_BALLOTS];
    __shared__ int s_base;

    const int n = min(max(*ray_count, 0), R);
    const int i0 = blockIdx.x * rpw;
    if (i0 >= n) return;                     // (the grid is sized from R: *ray_count is known on the device only)
    const int nr = min(rpw, n - i0);
    const int T = nr * S;                    // <= CR_MAX_SAMPLES by the launch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int i = tid; i < nr; i += CR_BLOCK) {
        const int r = min(max(ray_list[i0 + i], 0), R - 1);
        const float lo = t_lo[r], hi = t_hi[r];
        const float slack = mask_slack(lo, hi);
        s_o[i] = make_float4(rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2], COARSE ? near[r] : 0.f);
        s_d[i] = make_float4(rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2], COARSE ? far[r] : 0.f);
        s_m[i] = make_float4(lo - slack, hi + slack, __builtin_bit_cast(float, ray_mask[r]), __builtin_bit_cast(float, r));
    }
    // stage_bone_tables (common.hpp, pad 0) restated: the pose's transforms ride in the align loop; apart, both instantiations moved
    for (int i = tid; i < J * 16; i += CR_BLOCK) { s_align[i] = align[i]; s_skt[i] = skts[i]; }
    for (int i = tid; i < J * 4; i += CR_BLOCK) s_scale[i] = (i & 3) < 3 ? fabsf(axis_scale[(i >> 2) * 3 + (i & 3)]) : 0.f;
    __syncthreads();

    const float inv_S = 1.0f / (float)S;
    const int nturns = (T + CR_PAIR - 1) / CR_PAIR;

    // ---- 1. depths, words, ballots
    for (int c = 0; c < nturns; ++c) {
        const int la = c * CR_PAIR + tid, lb = la + CR_BLOCK;
        const int lac = min(la, T - 1), lbc = min(lb, T - 1);            // (a tail sample repeats the last one and stores nothing)
        const int ia = ray_of_local(lac, S, inv_S), ib = ray_of_local(lbc, S, inv_S);
        const int sa = lac - ia * S, sb = lbc - ib * S;
        const float4 oa = s_o[ia], da = s_d[ia], qa = s_m[ia];
        const float4 ob = s_o[ib], db = s_d[ib], qb = s_m[ib];
        const size_t ma = (size_t)__builtin_bit_cast(int, qa.w) * S + sa, mb = (size_t)__builtin_bit_cast(int, qb.w) * S + sb;
        float za, zb;
        if (COARSE) {
            za = coarse_sample(oa.w, da.w, sa, S, nullptr, 0);
            zb = coarse_sample(ob.w, db.w, sb, S, nullptr, 0);
            if (la < T) z[ma] = za;
            if (lb < T) z[mb] = zb;
        } else {
            za = z[ma];
            zb = z[mb];
        }
        // candidate bones: the ray's mask for a depth inside the interval it was made for, every bone otherwise
        const uint32_t pre_a = (za >= qa.x && za <= qa.y) ? __builtin_bit_cast(uint32_t, qa.z) : (1u << J) - 1u;
        const uint32_t pre_b = (zb >= qb.x && zb <= qb.y) ? __builtin_bit_cast(uint32_t, qb.z) : (1u << J) - 1u;
        const float o_a[3] = {oa.x, oa.y, oa.z}, d_a[3] = {da.x, da.y, da.z};
        const float o_b[3] = {ob.x, ob.y, ob.z}, d_b[3] = {db.x, db.y, db.z};
        float pa[3], pb[3];
        sample_point(o_a, d_a, za, pa);
        sample_point(o_b, d_b, zb, pb);
        const v2f px = {pa[0], pb[0]}, py = {pa[1], pb[1]}, pz = {pa[2], pb[2]};
        uint32_t ba = 0, bb = 0;
        in_volume_pk(s_skt, s_align, s_scale, wave_or(pre_a | pre_b), px, py, pz, ba, bb);
        if (la >= T) ba = 0u;
        if (lb >= T) bb = 0u;
        if (la < T) valid_bits[ma] = ba;
        if (lb < T) valid_bits[mb] = bb;
        const unsigned long long ball_a = __ballot(ba != 0u), ball_b = __ballot(bb != 0u);
        if (lane == 0) {
            s_ball[c * 8 + wave] = ball_a;           // local samples [64 k, 64 k + 64) of ballot k
            s_ball[c * 8 + 4 + wave] = ball_b;
        }
    }
    __syncthreads();

    // ---- 2. first row of every ballot, one draw on the counter
    const int nball = nturns * 8;
    if (wave == 0) {
        int run = 0;
        for (int k0 = 0; k0 < nball; k0 += 64) {
            const int k = k0 + lane;
            const int cnt = k < nball ? (int)__popcll(s_ball[k]) : 0;
            int incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            if (k < nball) s_off[k] = run + incl - cnt;
            run += __builtin_amdgcn_readlane(incl, 63);
        }
        if (lane == 0) s_base = run > 0 ? atomicAdd(count, run) : 0;
    }
    __syncthreads();

    // ---- 3. the rows
    const int base = s_base;
    for (int c = 0; c < nturns; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = c * 8 + 4 * h + wave;
            const unsigned long long ball = s_ball[k];
            if ((ball >> lane) & 1ull) {             // (set only for local samples < T)
                const int li = c * CR_PAIR + h * CR_BLOCK + tid;
                const int i = ray_of_local(li, S, inv_S);
                const int r = __builtin_bit_cast(int, s_m[i].w);
                list[base + s_off[k] + (int)__popcll(ball & ((1ull << lane) - 1ull))] = (int32_t)(r * S + (li - i * S));
            }
        }
    }
}

}  // namespace danbo

using namespace danbo;

// rays per workgroup where the caller leaves the choice (rays_per_wg = 0): about a thousand draws on the counter for the listed
// rays of a 512 x 512 frame, in both passes (profiles/cull_rays_measured.txt has the timings of the alternatives)
static int default_rays_per_wg(bool coarse) { return coarse ? 64 : 96; }

extern "C" int danbo_bone_cull_rays(const int32_t* ray_list, const int32_t* ray_count, const uint32_t* ray_mask, const float* t_lo,
                                    const float* t_hi, const float* rays_o, const float* rays_d, int R, int S, int G, const float* skts,
                                    const float* align, const float* axis_scale, const float* near, const float* far, float* z,
                                    int rays_per_wg, uint32_t* valid_bits, int32_t* list, int32_t* count, void* stream) {
    DANBO_CHECK_ARG(ray_list && ray_count && ray_mask && t_lo && t_hi && rays_o && rays_d && skts && align && axis_scale);
    DANBO_CHECK_ARG(z && valid_bits && list && count);
    DANBO_CHECK_ARG((near == nullptr) == (far == nullptr));
    DANBO_CHECK_ARG(G == 1);                                                // one pose: the frame's case (danbo_bone_cull has the others)
    DANBO_CHECK_ARG(R > 0 && S > 0 && S <= CR_MAX_SAMPLES && (long)R * S <= 0x7fffffffL);
    DANBO_CHECK_ARG(rays_per_wg >= 0);
    const bool coarse = near != nullptr;
    int rpw = rays_per_wg > 0 ? rays_per_wg : default_rays_per_wg(coarse);
    rpw = std::min(rpw, std::min(CR_MAX_RPW, CR_MAX_SAMPLES / S));           // >= 1
    const int grid = ceil_div(R, rpw);
    if (coarse)
        hipLaunchKernelGGL(k_cull_rays<true>, dim3(grid), dim3(CR_BLOCK), 0, (hipStream_t)stream, ray_list, ray_count, ray_mask, t_lo,
                           t_hi, rays_o, rays_d, skts, align, axis_scale, near, far, z, R, S, rpw, valid_bits, list, count);
    else
        hipLaunchKernelGGL(k_cull_rays<false>, dim3(grid), dim3(CR_BLOCK), 0, (hipStream_t)stream, ray_list, ray_count, ray_mask, t_lo,
                           t_hi, rays_o, rays_d, skts, align, axis_scale, near, far, z, R, S, rpw, valid_bits, list, count);
    DANBO_LAUNCH_RET();
}
