// Connected components of a density grid's inside set and the filter that drops unwanted ones (include/danbo_grid_cc.h), where the
// grid of RayCaster.render_mesh_density lies: in device memory, before marching cubes.  Every definition is grid_cc_math.hpp's,
// whose serial restatement the tests compare these kernels with bit for bit.
//
// A lock-free union-find over the logical linear index p.  `labels` is the parent array while the label call runs: parent[p] = -1
// outside, else an index <= p of p's component; a root has parent[r] = r.  INVARIANT: parent[p] <= p -- set by k_cc_init, and kept
// because a parent is afterwards only lowered (atomicMin in k_cc_union, the root itself in k_cc_flatten).  So a tree's root is its
// smallest index, and once every neighbouring pair is joined the root of a point IS its label.
//   k_cc_init     one thread per point: inside-ness, and the run of inside points along k that the point belongs to INSIDE its
//                 wavefront, found from two ballots (as k_mesh_classify ranks): parent[p] = the first point of the run.  sizes = 0.
//   k_cc_union    joins p with its +i and +j neighbours, and with p - 1 where a run goes on across a wavefront boundary.  A pair
//                 (p, q) whose predecessors (p - 1, q - 1) are both inside is skipped: p ~ p - 1, q ~ q - 1 and (p - 1, q - 1) is
//                 some thread's pair, so only the pairs at the ends of runs cost an atomic.
//   k_cc_flatten  parent[p] = root(p); sizes[root] += 1, added up per distinct root inside the wavefront first and carried in
//                 registers across the wavefront's chunks while the root stays the same (one body: a few atomics per wavefront,
//                 not one per point); the numbers of inside points and of roots.
//   k_cc_best     the maximum of cc_size_key over sizes: one 64-bit integer atomicMax per wavefront.
//   k_cc_stats    one thread: stats[4] from the three counters.
//   k_cc_keep     (danbo_grid_cc_keep) one thread per point: the keep rule on sizes[labels[p]] and stats[3], the copied or filled word.
//
// WHY NOTHING HERE CAN HANG.  No kernel waits for another workgroup: no spin loop, no flag, no grid-wide barrier, no assumption of
// co-residency; phases that need each other's results are separate launches on the stream.  Every loop ends by construction:
//   * cc_root walks x -> parent[x] only while the value read is smaller than x: x strictly decreases and is >= 0;
//   * cc_union holds a pair (a, b), a + b >= 0.  A pass takes both roots (neither grows), returns if they are equal, and hooks the
//     larger, a, below the smaller with atomicMin.  If the atomic returns a, a was a root and the pair is joined: return.  Otherwise
//     it returns old < a: the pass goes on with (old, b), so a + b has strictly decreased.  No retry counter, no "until nothing
//     changed";
//   * the loop over the distinct roots of a wavefront clears at least its leader's bit of the mask in every pass.
// WHY STALE READS ARE HARMLESS.  The eight XCDs have private L2s.  A word another workgroup may write in the same launch (parent[])
// is read with a relaxed agent-scope atomic load or through an atomic's return value, never with a plain load; and correctness does
// not need the value to be fresh.  Every value parent[x] ever held is an index of x's component, <= x.  When atomicMin replaces the
// link a -> old by a -> b, the thread that did it goes on to join (old, b), so everything that was ever linked, and every pair
// asked for, is joined when the launch ends: a walk over a stale link only starts its union from a point further from the root --
// extra steps, the same result.  The atomic's return value is the truth the decision "a was a root" is taken on.
// Bounds: a neighbour index is formed only where i + 1 < nx / j + 1 < ny / k > 0 says it exists; lanes past the last point of the
// last chunk load and store nothing.  No allocation, no synchronisation.  gfx950, wave64.
#include "common.hpp"
#include "grid_cc_math.hpp"
#include "../../include/danbo_grid_cc.h"

namespace danbo {

struct CcDims {
    int nx, ny, nz;
    uint32_t n_pts;
    int n_chunks;
};

// the counters at the head of the workspace (CC_HEAD_BYTES)
struct CcHead {
    unsigned long long best;
    int inside, comps;
};
static_assert(sizeof(CcHead) <= CC_HEAD_BYTES, "the counters fit the head of the workspace");

__device__ __forceinline__ void cc_ijk(const CcDims& d, uint32_t n, int* i, int* j, int* k) {
    const uint32_t r = n / (uint32_t)d.nz;
    *k = (int)(n - r * (uint32_t)d.nz);
    *i = (int)(r / (uint32_t)d.ny);
    *j = (int)(r - (uint32_t)*i * (uint32_t)d.ny);
}

// parent[x] as it is now or as it was: never a plain load (another workgroup may be lowering it)
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of the inside point x.  Ends: x goes on only to a value below it (the unsigned comparison also stops at a negative word).
__device__ __forceinline__ int cc_root(const int* parent, int x) {
    for (;;) {
        const int q = cc_load(parent + x);
        if ((uint32_t)q >= (uint32_t)x) return x;
        x = q;
    }
}

// Joins the components of the inside points a and b.  Ends: see the head of this file (a + b strictly decreases from pass to pass).
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_root(parent, a);
        b = cc_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;       // a was a root and hangs below b now
        a = old;                    // a had been hooked meanwhile (old < a): parent[a] = min(old, b), and (old, b) is still to be joined
    }
}

__global__ __launch_bounds__(CC_CHUNK) void k_cc_init(const float* __restrict__ sigma, long sx, long sy, float floor, float iso, CcDims d,
                                                      int* __restrict__ parent, int* __restrict__ sizes, CcHead* __restrict__ head) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) { head->best = 0ull; head->inside = 0; head->comps = 0; }
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
        const uint32_t p = (uint32_t)chunk * CC_CHUNK + threadIdx.x;
        const bool live = p < d.n_pts;
        int i = 0, j = 0, k = 0;
        bool in = false;
        if (live) {
            cc_ijk(d, p, &i, &j, &k);
            in = cc_inside(sigma[i * sx + j * sy + k], floor, iso);
        }
        const uint64_t inb = __ballot(in);
        // a run starts at an inside lane that is the first of its wavefront or of its row, or that follows a lane outside
        const bool start = in && (lane == 0 || k == 0 || !((inb >> (lane - 1)) & 1ull));
        const uint64_t sb = __ballot(start);
        if (live) {
            int v = -1;
            if (in) {
                const uint64_t upto = sb & (~0ull >> (63 - lane));      // the starts at or below this lane: at least its own run's
                v = (int)(p - (uint32_t)(lane - (63 - __clzll((long long)upto))));
            }
            parent[p] = v;
            sizes[p] = 0;
        }
    }
}

__global__ __launch_bounds__(CC_CHUNK) void k_cc_union(CcDims d, int* parent) {
    const int lane = threadIdx.x & 63;
    const uint32_t step_j = (uint32_t)d.nz, step_i = (uint32_t)d.ny * (uint32_t)d.nz;
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
        const uint32_t p = (uint32_t)chunk * CC_CHUNK + threadIdx.x;
        const bool live = p < d.n_pts;
        int i = 0, j = 0, k = 0, bits = 0;       // bit 0: p inside, bit 1: its +i neighbour, bit 2: its +j neighbour
        bool hi = false, hj = false;
        if (live) {
            cc_ijk(d, p, &i, &j, &k);
            hi = i + 1 < d.nx; hj = j + 1 < d.ny;
            bits = (cc_load(parent + p) >= 0 ? 1 : 0) | (hi && cc_load(parent + p + step_i) >= 0 ? 2 : 0) |
                   (hj && cc_load(parent + p + step_j) >= 0 ? 4 : 0);
        }
        // the same of the point p - 1 = (i, j, k - 1): the lane below's (k > 0: the same row), the first lane of a wavefront loads it
        int prev = __shfl_up(bits, 1, WAVE);
        if (lane == 0 && live && k > 0)
            prev = (cc_load(parent + p - 1) >= 0 ? 1 : 0) | (hi && cc_load(parent + p + step_i - 1) >= 0 ? 2 : 0) |
                   (hj && cc_load(parent + p + step_j - 1) >= 0 ? 4 : 0);
        if (k == 0) prev = 0;
        if (bits & 1) {
            if (lane == 0 && (prev & 1)) cc_union(parent, (int)p, (int)(p - 1));               // a run across two wavefronts
            if ((bits & 2) && (prev & 3) != 3) cc_union(parent, (int)p, (int)(p + step_i));
            if ((bits & 4) && (prev & 5) != 5) cc_union(parent, (int)p, (int)(p + step_j));
        }
    }
}

__global__ __launch_bounds__(CC_CHUNK) void k_cc_flatten(CcDims d, int* parent, int* sizes, CcHead* head) {
    const int lane = threadIdx.x & 63;
    int cur = -1, cur_n = 0, n_in = 0, n_roots = 0;      // the same in every lane of the wavefront
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
        const uint32_t p = (uint32_t)chunk * CC_CHUNK + threadIdx.x;
        int r = -1;
        if (p < d.n_pts && cc_load(parent + p) >= 0) {
            r = cc_root(parent, (int)p);
            // (a walker of another workgroup reads the old parent or the root: both are links of the same tree)
            __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const bool in = r >= 0;
        uint64_t todo = __ballot(in);
        n_in += __popcll(todo);
        n_roots += __popcll(__ballot(in && r == (int)p));
        while (todo) {      // one pass per distinct root of the wavefront: every pass clears at least the leader's bit
            const int leader = __ffsll((long long)todo) - 1;
            const int rl = __shfl(r, leader, WAVE);
            const uint64_t same = __ballot(in && r == rl);
            const int n = __popcll(same);
            if (rl == cur) {
                cur_n += n;
            } else {
                if (cur_n > 0 && lane == 0) atomicAdd(sizes + cur, cur_n);
                cur = rl;
                cur_n = n;
            }
            todo &= ~same;
        }
    }
    if (lane == 0) {
        if (cur_n > 0) atomicAdd(sizes + cur, cur_n);
        if (n_in > 0) atomicAdd(&head->inside, n_in);
        if (n_roots > 0) atomicAdd(&head->comps, n_roots);
    }
}

__global__ __launch_bounds__(CC_CHUNK) void k_cc_best(uint32_t n_pts, const int* __restrict__ sizes, CcHead* __restrict__ head) {
    unsigned long long best = 0ull;
    const uint32_t stride = gridDim.x * CC_CHUNK;
    for (uint32_t p = blockIdx.x * CC_CHUNK + threadIdx.x; p < n_pts; p += stride) {       // (p + stride < 2^32: n_pts < 2^31)
        const int s = sizes[p];
        if (s > 0) {
            const unsigned long long key = cc_size_key(s, (int)p);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, WAVE);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&head->best, best);
}

__global__ __launch_bounds__(WAVE) void k_cc_stats(const CcHead* __restrict__ head, int* __restrict__ stats) {
    if (threadIdx.x != 0) return;
    const unsigned long long best = head->best;
    stats[0] = head->inside;
    stats[1] = head->comps;
    stats[2] = cc_key_size(best);
    stats[3] = cc_key_label(best);
}

struct CcKeepArgs {
    const uint32_t* sigma;
    long sx, sy;
    const int *labels, *sizes, *stats;
    int keep_largest, min_points;
    uint32_t fill_bits;
    uint32_t* out;
    long osx, osy;
    int* kept;
};

// in place (out == sigma, equal strides): a thread reads its own point's word before it writes it and reads no other point's
__global__ __launch_bounds__(CC_CHUNK) void k_cc_keep(CcDims d, CcKeepArgs a) {
    const int largest = a.stats[3];
    int n_comps = 0, n_points = 0;
    for (int chunk = blockIdx.x; chunk < d.n_chunks; chunk += gridDim.x) {
        const uint32_t p = (uint32_t)chunk * CC_CHUNK + threadIdx.x;
        bool keep = false, root = false;
        if (p < d.n_pts) {
            int i, j, k;
            cc_ijk(d, p, &i, &j, &k);
            const int label = a.labels[p];
            const bool inside = cc_label_inside(label, (long)d.n_pts);
            keep = inside && cc_keep(a.sizes[label], label, a.keep_largest, a.min_points, largest);
            root = keep && label == (int)p;
            a.out[i * a.osx + j * a.osy + k] = cc_out_word(a.sigma[i * a.sx + j * a.sy + k], inside, keep, a.fill_bits);
        }
        n_points += __popcll(__ballot(keep));
        n_comps += __popcll(__ballot(root));
    }
    if (a.kept && (threadIdx.x & 63) == 0) {
        if (n_comps > 0) atomicAdd(a.kept, n_comps);
        if (n_points > 0) atomicAdd(a.kept + 1, n_points);
    }
}

static inline CcDims cc_dims(int nx, int ny, int nz) {
    const long n = (long)nx * ny * nz;
    return CcDims{nx, ny, nz, (uint32_t)n, (int)((n + CC_CHUNK - 1) / CC_CHUNK)};
}
static inline bool cc_aligned(const void* p, uintptr_t to) { return (uintptr_t)p % to == 0; }

}  // namespace danbo

using namespace danbo;

// the counters, then one int per point: the sizes of a call that does not want them
extern "C" size_t danbo_grid_cc_workspace_bytes(int nx, int ny, int nz) {
    if (!cc_dims_ok(nx, ny, nz, 0, 0, 0.f, 0.f)) return 0;
    return CC_HEAD_BYTES + (size_t)nx * ny * nz * sizeof(int);
}

extern "C" int danbo_grid_cc_label(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                                   void* workspace, int32_t* labels, int32_t* sizes, int32_t* stats, void* stream) {
    DANBO_CHECK_ARG(sigma && workspace && labels && stats && cc_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso));
    DANBO_CHECK_ARG(cc_aligned(sigma, 4) && cc_aligned(workspace, 8) && cc_aligned(labels, 4) && cc_aligned(sizes, 4) && cc_aligned(stats, 4));
    const CcDims d = cc_dims(nx, ny, nz);
    CcHead* head = static_cast<CcHead*>(workspace);
    int* sz = sizes ? sizes : reinterpret_cast<int*>(static_cast<char*>(workspace) + CC_HEAD_BYTES);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(stream_grid((long)d.n_chunks * CC_CHUNK, CC_CHUNK)), block(CC_CHUNK);
    hipLaunchKernelGGL(k_cc_init, grid, block, 0, st, sigma, stride_x, stride_y, floor, iso, d, labels, sz, head);
    hipLaunchKernelGGL(k_cc_union, grid, block, 0, st, d, labels);
    hipLaunchKernelGGL(k_cc_flatten, grid, block, 0, st, d, labels, sz, head);
    hipLaunchKernelGGL(k_cc_best, grid, block, 0, st, d.n_pts, sz, head);
    hipLaunchKernelGGL(k_cc_stats, dim3(1), dim3(WAVE), 0, st, head, stats);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_grid_cc_keep(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                                  const int32_t* labels, const int32_t* sizes, const int32_t* stats, int keep_largest, int min_points,
                                  float fill, float* out, long out_stride_x, long out_stride_y, int32_t* kept, void* stream) {
    DANBO_CHECK_ARG(sigma && labels && sizes && stats && out && cc_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso));
    DANBO_CHECK_ARG(cc_aligned(sigma, 4) && cc_aligned(labels, 4) && cc_aligned(sizes, 4) && cc_aligned(stats, 4) && cc_aligned(out, 4) &&
                    cc_aligned(kept, 4));
    DANBO_CHECK_ARG(min_points >= 0 && cc_fill_ok(fill, floor, iso) && cc_out_layout_ok(nx, ny, nz, out_stride_x, out_stride_y) &&
                    cc_overlap_ok(sigma, stride_x, stride_y, out, out_stride_x, out_stride_y, nx, ny, nz));
    const CcDims d = cc_dims(nx, ny, nz);
    const hipStream_t st = (hipStream_t)stream;
    if (kept) zero_words(kept, 2, nullptr, 0, st);
    const CcKeepArgs a = {reinterpret_cast<const uint32_t*>(sigma), stride_x, stride_y, labels, sizes, stats, keep_largest, min_points,
                          __builtin_bit_cast(uint32_t, fill), reinterpret_cast<uint32_t*>(out), out_stride_x, out_stride_y, kept};
    hipLaunchKernelGGL(k_cc_keep, dim3(stream_grid((long)d.n_chunks * CC_CHUNK, CC_CHUNK)), dim3(CC_CHUNK), 0, st, d, a);
    DANBO_LAUNCH_RET();
}
