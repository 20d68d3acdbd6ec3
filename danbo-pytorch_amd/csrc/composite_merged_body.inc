// Body of k_composite_merged / k_composite_merged_softplus (k_sample.hip), included into each of them with
//   constexpr int DA (the density activation, sample_math.hpp) and float shift
// in scope.  Not a kernel template and not an inlined function: this kernel spills SGPRs under its waves_per_eu bound, and either
// form moved the register allocation of the relu kernel (as a template instantiation: seven more moves and one more VGPR around the
// same arithmetic).  Included into a plain kernel, the relu form compiles to the instruction sequence it had before the activation
// became a parameter.
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int St = S + Sf;
    if (St <= 64) {
        // one chunk per ray, software-pipelined over the wavefront's rays: a ray is the chain sorted_idx -> in-volume word -> raw;
        // the index of ray r + 2 and the word of ray r + 1 are in flight while ray r is composited
        const bool act = lane < St;
        struct Idx { int src; float zs, z1, dn; float4 re; };
        auto fetch_idx = [&](int r) {
            Idx in;
            const size_t m = (size_t)r * St + (act ? lane : St - 1);
            in.src = min(max(sorted_idx[m], 0), St - 1);     // NaN depths must not become an out-of-bounds read
            in.zs = z[m];
            in.z1 = (lane + 1 < St) ? z[m + 1] : 0.f;
            in.dn = ray_norm(rays_d, r);
            in.re = raw_empty ? raw_empty[r] : float4{0.f, 0.f, 0.f, 0.f};
            return in;
        };
        auto fetch_word = [&](int r, int src) -> uint32_t {
            if (src < S) return bits_a ? bits_a[(size_t)r * S + src] : 1u;
            return bits_b ? bits_b[(size_t)r * Sf + (src - S)] : 1u;
        };
        // item i of the launch: the i-th listed ray, or (no list) ray scattered_ray(i); the index of item i + 2 and the word of
        // item i + 1 are in flight while item i is composited
        const int n = ray_list ? min(max(*ray_count, 0), R) : R;
        auto ray_at = [&](int i) { return i < n ? (ray_list ? min(max(ray_list[i], 0), R - 1) : scattered_ray(i, scatter, R)) : -1; };
        int r = ray_at(wave), r_nxt = ray_at(wave + nwaves);
        if (r < 0) return;
        Idx cur = fetch_idx(r), nxt = fetch_idx(r_nxt >= 0 ? r_nxt : r);
        uint32_t cur_word = fetch_word(r, cur.src);
        for (int i = wave; i < n; i += nwaves) {
            CompositeState st = {1.0f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const size_t m = (size_t)r * St + (act ? lane : St - 1);
            float4 rw = cur.re;
            if (cur_word != 0u) rw = cur.src < S ? raw_a[(size_t)r * S + cur.src] : raw_b[(size_t)r * Sf + (cur.src - S)];
            const int r_n = r_nxt >= 0 ? r_nxt : r;
            const uint32_t nxt_word = fetch_word(r_n, nxt.src);
            const int r_nn = ray_at(i + 2 * nwaves);
            const Idx nn = fetch_idx(r_nn >= 0 ? r_nn : r_n);
            const float gap = (lane + 1 < St) ? sub_rn(cur.z1, cur.zs) : 1e10f;
            float al, w;
            // a ray without an in-volume sample in either pass: constants, as in k_composite_importance below (bit for bit)
            // -- relu only: softplus is positive everywhere, the condition can never hold and the path is compiled out
            const float dist = mul_rn(gap, cur.dn);
            const float rgb_sum = add_rn(add_rn(cur.re.x, cur.re.y), cur.re.z);
            const bool flat = DA == DENSITY_RELU && raw_empty != nullptr && bits_a != nullptr && bits_b != nullptr && noise == nullptr &&
                              !(div_rn(cur.re.w, B) > 0.f) && sub_rn(rgb_sum, rgb_sum) == 0.f &&
                              __all(cur_word == 0u && sub_rn(dist, dist) == 0.f);
            if (flat) {
                al = 0.f;
                w = 0.f;
            } else {
                w = composite_chunk<DA>(st, rw, cur.zs, gap, cur.dn, B, noise != nullptr, noise ? noise[m] : 0.f, act, lane, al, shift);
            }
            if (act) {
                if (weights) weights[m] = w;
                if (alpha_out) alpha_out[m] = al;
                if (raw_sorted) raw_sorted[m] = rw;
            }
            if (lane == 0) composite_finish(st, r, rgb_map, disp, acc_out);
            cur = nxt; cur_word = nxt_word; nxt = nn; r = r_n; r_nxt = r_nn;
        }
        return;
    }
    const int n_all = ray_list ? min(max(*ray_count, 0), R) : R;
    for (int i = wave; i < n_all; i += nwaves) {
        const int r = ray_list ? min(max(ray_list[i], 0), R - 1) : i;
        const float dn = ray_norm(rays_d, r);
        CompositeState st = {1.0f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < St; c0 += 64) {
            const int s = c0 + lane;
            const bool act = s < St;
            const size_t m = (size_t)r * St + (act ? s : St - 1);
            const int src = min(max(sorted_idx[m], 0), St - 1);   // NaN depths must not become an out-of-bounds read
            float4 rw;
            if (src < S) {
                const size_t q = (size_t)r * S + src;
                rw = (bits_a && bits_a[q] == 0u) ? raw_empty[r] : raw_a[q];
            } else {
                const size_t q = (size_t)r * Sf + (src - S);
                rw = (bits_b && bits_b[q] == 0u) ? raw_empty[r] : raw_b[q];
            }
            const float zs = z[m];
            const float gap = (s + 1 < St) ? sub_rn(z[m + 1], zs) : 1e10f;
            float al;
            const float w = composite_chunk<DA>(st, rw, zs, gap, dn, B, noise != nullptr, noise ? noise[m] : 0.f, act, lane, al, shift);
            if (act) {
                if (weights) weights[m] = w;
                if (alpha_out) alpha_out[m] = al;
                if (raw_sorted) raw_sorted[m] = rw;
            }
        }
        if (lane == 0) composite_finish(st, r, rgb_map, disp, acc_out);
    }
