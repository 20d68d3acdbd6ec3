// Isosurface extraction (marching cubes) on the density grid of RayCaster.render_mesh_density, where it lies: in device memory.
// Replaces the host step of the reference's render_mesh (run_render.py:1265-1281: mcubes.marching_cubes(np.maximum(raw, 0), threshold));
// the definitions -- inside-ness, vertex ownership, order, orientation -- are those of mesh_math.hpp, whose serial extractor the tests
// compare these kernels with bit for bit.
//
// The grid is cut into chunks of MESH_CHUNK = 256 consecutive points of the LOGICAL linear index ((i * ny + j) * nz + k); a chunk is
// one workgroup's work, so "ascending by linear index" is "ascending by chunk, then by rank inside the chunk" and no atomic orders
// anything:
//   k_mesh_classify   one thread per point: 4 loads (the rows (i, j), (i+1, j), (i, j+1), (i+1, j+1) at its k, coalesced along k),
//                     the four at k + 1 come from the next lane (the last lane of a wavefront loads its own).  Per point the mask of
//                     owned crossing edges and the case of its cell; ranks inside the chunk by ballot + mbcnt; one 4-byte word per
//                     point (mesh_word) and the chunk's two totals.  A chunk without a crossing writes its totals only.
//   k_mesh_scan       one workgroup: exclusive scan of the chunk totals in place (64-bit carry, saturating at INT_MAX), V and T.
//   k_mesh_vertices   one thread per point with an owned crossing edge: t, the output transform, float[V][3].
//   k_mesh_triangles  one thread per cell with triangles: a welded vertex index is voff[chunk of the owning point] + the rank in
//                     that point's word + the owned edges below the axis -- read from the words, not from a 3 N index array.
//   k_mesh_normals    (danbo_mesh_normals) one thread per point with an owned crossing edge, the walk of k_mesh_vertices: the
//                     normalised negative gradient of the floored grid at every vertex, float[V][3] (mesh_math.hpp).
// Workspace: 4 B per grid point + 8 B per chunk (danbo_mesh_workspace_bytes).  No allocation, no synchronisation.  gfx950, wave64.
#include "common.hpp"
#include "mesh_math.hpp"

namespace danbo {

static __device__ const uint64_t MC_CASE_DEV[256] = {
#include "mc_table.inc"
};

struct MeshGridArgs {
    const float* sigma;
    int nx, ny, nz;
    long sx, sy;
    float floor, iso;
    uint32_t n_pts;
    int n_chunks;
};

__device__ __forceinline__ int lanes_below(uint64_t ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

__device__ __forceinline__ void mesh_ijk(const MeshGridArgs& a, uint32_t n, int* i, int* j, int* k) {
    const uint32_t r = n / (uint32_t)a.nz;
    *k = (int)(n - r * (uint32_t)a.nz);
    *i = (int)(r / (uint32_t)a.ny);
    *j = (int)(r - (uint32_t)*i * (uint32_t)a.ny);
}

__global__ __launch_bounds__(MESH_CHUNK) void k_mesh_classify(MeshGridArgs a, uint32_t* __restrict__ words, int* __restrict__ vcnt,
                                                              int* __restrict__ tcnt) {
    __shared__ uint8_t s_ntri[256];
    __shared__ int s_v[MESH_CHUNK / WAVE], s_t[MESH_CHUNK / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_ntri[tid] = (uint8_t)mc_ntri(MC_CASE_DEV[tid]);
    __syncthreads();
    auto in = [&](const float* p) { return mesh_inside(mesh_value(*p, a.floor), a.iso) ? 1 : 0; };
    for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const uint32_t n = (uint32_t)chunk * MESH_CHUNK + tid;
        const bool live = n < a.n_pts;
        int i = 0, j = 0, k = 0, b4 = 0;
        bool hx = false, hy = false, hz = false;
        const float* p = a.sigma;
        if (live) {
            mesh_ijk(a, n, &i, &j, &k);
            hx = i + 1 < a.nx; hy = j + 1 < a.ny; hz = k + 1 < a.nz;
            p += i * a.sx + j * a.sy + k;
            b4 = in(p) | (hx ? in(p + a.sx) << 1 : 0) | (hy ? in(p + a.sy) << 2 : 0) | (hx && hy ? in(p + a.sx + a.sy) << 3 : 0);
        }
        // the point n + 1 = (i, j, k + 1) is the next lane's (same i, j: same hx, hy)
        int nb = __shfl_down(b4, 1, WAVE);
        if (lane == WAVE - 1 && hz)
            nb = in(p + 1) | (hx ? in(p + a.sx + 1) << 1 : 0) | (hy ? in(p + a.sy + 1) << 2 : 0) | (hx && hy ? in(p + a.sx + a.sy + 1) << 3 : 0);
        const int emask = (hx ? ((b4 >> 1) ^ b4) & 1 : 0) | (hy ? (((b4 >> 2) ^ b4) & 1) << 1 : 0) | (hz ? ((nb ^ b4) & 1) << 2 : 0);
        const int cell_case = hx && hy && hz ? (b4 | (nb << 4)) : 0;
        const int nt = s_ntri[cell_case];
        const uint64_t e0 = __ballot(emask & 1), e1 = __ballot(emask & 2), e2 = __ballot(emask & 4);
        const uint64_t t0 = __ballot(nt & 1), t1 = __ballot(nt & 2), t2 = __ballot(nt & 4);
        int vrank = lanes_below(e0) + lanes_below(e1) + lanes_below(e2);
        int trank = lanes_below(t0) + 2 * lanes_below(t1) + 4 * lanes_below(t2);
        if (lane == 0) {
            s_v[wave] = __popcll(e0) + __popcll(e1) + __popcll(e2);
            s_t[wave] = __popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2);
        }
        __syncthreads();
        int vtot = 0, ttot = 0;
#pragma unroll
        for (int w = 0; w < MESH_CHUNK / WAVE; ++w) {
            if (w < wave) { vrank += s_v[w]; trank += s_t[w]; }
            vtot += s_v[w]; ttot += s_t[w];
        }
        if (live && (vtot | ttot)) words[n] = mesh_word(emask, cell_case, vrank, trank);
        if (tid == 0) { vcnt[chunk] = vtot; tcnt[chunk] = ttot; }
        __syncthreads();
    }
}

__device__ __forceinline__ int mesh_sat(long v) { return v < 0x7fffffffL ? (int)v : 0x7fffffff; }

// exclusive scan in place over cnt[0 .. n_chunks), the total into cnt[n_chunks] and counts[]; one workgroup of 1024
__global__ __launch_bounds__(1024) void k_mesh_scan(int* __restrict__ vcnt, int* __restrict__ tcnt, int n_chunks, int* __restrict__ counts) {
    __shared__ int s_v[16], s_t[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long cv = 0, ct = 0;
    for (int base = 0; base < n_chunks; base += 1024) {
        const int idx = base + tid;
        const int v = idx < n_chunks ? vcnt[idx] : 0, t = idx < n_chunks ? tcnt[idx] : 0;
        int iv = v, it = t;       // a tile's sum is at most 1024 * 5 * 255: an int
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int pv = __shfl_up(iv, off, WAVE), pt = __shfl_up(it, off, WAVE);
            if (lane >= off) { iv += pv; it += pt; }
        }
        if (lane == WAVE - 1) { s_v[wave] = iv; s_t[wave] = it; }
        __syncthreads();
        int pv = 0, pt = 0, tv = 0, tt = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) { pv += s_v[w]; pt += s_t[w]; }
            tv += s_v[w]; tt += s_t[w];
        }
        if (idx < n_chunks) {
            vcnt[idx] = mesh_sat(cv + pv + iv - v);
            tcnt[idx] = mesh_sat(ct + pt + it - t);
        }
        cv += tv; ct += tt;
        __syncthreads();
    }
    if (tid == 0) {
        vcnt[n_chunks] = counts[0] = mesh_sat(cv);
        tcnt[n_chunks] = counts[1] = mesh_sat(ct);
    }
}

__global__ __launch_bounds__(MESH_CHUNK) void k_mesh_vertices(MeshGridArgs a, const uint32_t* __restrict__ words, const int* __restrict__ voff,
                                                              float scale, float ox, float oy, float oz, float* __restrict__ verts, int cap_v) {
    for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const int v0 = voff[chunk];
        if (voff[chunk + 1] == v0 || v0 >= cap_v) continue;       // no vertex here, or none below the capacity
        const uint32_t n = (uint32_t)chunk * MESH_CHUNK + threadIdx.x;
        if (n >= a.n_pts) continue;
        const uint32_t w = words[n];
        const int emask = mesh_word_emask(w);
        if (!emask) continue;
        int i, j, k;
        mesh_ijk(a, n, &i, &j, &k);
        const float* p = a.sigma + i * a.sx + j * a.sy + k;
        const float s0 = mesh_value(*p, a.floor);
        long v = (long)v0 + mesh_word_vrank(w);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((emask >> ax) & 1)) continue;
            if (v < cap_v) {
                const float t = mesh_edge_t(s0, mesh_value(p[ax == 0 ? a.sx : (ax == 1 ? a.sy : 1L)], a.floor), a.iso);
                verts[3 * v + 0] = mesh_coord(i, ax == 0 ? t : 0.f, scale, ox);
                verts[3 * v + 1] = mesh_coord(j, ax == 1 ? t : 0.f, scale, oy);
                verts[3 * v + 2] = mesh_coord(k, ax == 2 ? t : 0.f, scale, oz);
            }
            ++v;
        }
    }
}

// The normals of the vertices k_mesh_vertices writes, by the same walk: the gradient at the point (up to 6 loads) is shared by its
// owned edges, each adds the gradient at its upper end; every load is at a fixed offset of the thread's own point, so a wavefront's
// are coalesced along k like those of k_mesh_classify.
__global__ __launch_bounds__(MESH_CHUNK) void k_mesh_normals(MeshGridArgs a, const uint32_t* __restrict__ words, const int* __restrict__ voff,
                                                             float* __restrict__ normals, int cap_v) {
    const MeshReader at{a.sigma, a.sx, a.sy, a.floor};
    for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const int v0 = voff[chunk];
        if (voff[chunk + 1] == v0 || v0 >= cap_v) continue;       // no vertex here, or none below the capacity
        const uint32_t n = (uint32_t)chunk * MESH_CHUNK + threadIdx.x;
        if (n >= a.n_pts) continue;
        const uint32_t w = words[n];
        const int emask = mesh_word_emask(w);
        if (!emask) continue;
        int i, j, k;
        mesh_ijk(a, n, &i, &j, &k);
        float g0[3];
        mesh_gradient(at, a.nx, a.ny, a.nz, i, j, k, g0);
        long v = (long)v0 + mesh_word_vrank(w);
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!((emask >> ax) & 1)) continue;
            if (v < cap_v) {
                float nrm[3];
                mesh_vertex_normal(at, a.nx, a.ny, a.nz, i, j, k, ax, a.iso, g0, nrm);
                normals[3 * v + 0] = nrm[0];
                normals[3 * v + 1] = nrm[1];
                normals[3 * v + 2] = nrm[2];
            }
            ++v;
        }
    }
}

__global__ __launch_bounds__(MESH_CHUNK) void k_mesh_triangles(MeshGridArgs a, const uint32_t* __restrict__ words, const int* __restrict__ voff,
                                                               const int* __restrict__ toff, int* __restrict__ tris, int cap_t) {
    __shared__ uint64_t s_case[256];
    s_case[threadIdx.x] = MC_CASE_DEV[threadIdx.x];
    __syncthreads();
    for (int chunk = blockIdx.x; chunk < a.n_chunks; chunk += gridDim.x) {
        const int t0 = toff[chunk];
        if (toff[chunk + 1] == t0 || t0 >= cap_t) continue;
        const uint32_t n = (uint32_t)chunk * MESH_CHUNK + threadIdx.x;
        if (n >= a.n_pts) continue;
        const uint32_t w = words[n];
        const uint64_t entry = s_case[mesh_word_case(w)];
        const int nt = mc_ntri(entry);
        if (!nt) continue;
        const long t = (long)t0 + mesh_word_trank(w);
        for (int c = 0; c < 3 * nt; ++c) {
            int di, dj, dk, ax;
            mc_edge_owner(mc_edge(entry, c), &di, &dj, &dk, &ax);
            const uint32_t q = n + (uint32_t)((di * a.ny + dj) * a.nz + dk);     // inside the grid: the cell exists
            const uint32_t wq = words[q];
            const uint32_t idx = (uint32_t)voff[q / MESH_CHUNK] + (uint32_t)mesh_word_vrank(wq) +
                                 (uint32_t)mesh_popc3(mesh_word_emask(wq) & ((1 << ax) - 1));
            const long tt = t + c / 3;
            if (tt < cap_t) tris[3 * tt + c % 3] = (int)idx;
        }
    }
}

static inline long mesh_chunks(long n_pts) { return (n_pts + MESH_CHUNK - 1) / MESH_CHUNK; }
static inline size_t mesh_words_bytes(long n_pts) { return ((size_t)n_pts * 4 + 15) & ~(size_t)15; }

static inline bool finite_f(float x) { return x - x == 0.f; }

}  // namespace danbo

using namespace danbo;

extern "C" size_t danbo_mesh_workspace_bytes(int nx, int ny, int nz) {
    if (!mesh_dims_ok(nx, ny, nz, 0, 0, 0.f, 0.f)) return 0;
    const long n = (long)nx * ny * nz;
    return mesh_words_bytes(n) + 2 * (size_t)(mesh_chunks(n) + 1) * sizeof(int);
}

static MeshGridArgs mesh_args(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso) {
    const long n = (long)nx * ny * nz;
    return MeshGridArgs{sigma, nx, ny, nz, sx, sy, floor, iso, (uint32_t)n, (int)mesh_chunks(n)};
}

extern "C" int danbo_mesh_count(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                                void* workspace, int* counts, void* stream) {
    DANBO_CHECK_ARG(sigma && workspace && counts && mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso));
    DANBO_CHECK_ARG((uintptr_t)sigma % 4 == 0 && (uintptr_t)workspace % 4 == 0 && (uintptr_t)counts % 4 == 0);
    const MeshGridArgs a = mesh_args(sigma, nx, ny, nz, stride_x, stride_y, floor, iso);
    uint32_t* words = static_cast<uint32_t*>(workspace);
    int* vcnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + mesh_words_bytes(a.n_pts));
    int* tcnt = vcnt + a.n_chunks + 1;
    hipLaunchKernelGGL(k_mesh_classify, dim3(stream_grid((long)a.n_chunks * MESH_CHUNK, MESH_CHUNK)), dim3(MESH_CHUNK), 0,
                       (hipStream_t)stream, a, words, vcnt, tcnt);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, vcnt, tcnt, a.n_chunks, counts);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_mesh_extract(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                                  const void* workspace, float scale, float off_x, float off_y, float off_z, float* verts, int cap_v,
                                  int* tris, int cap_t, void* stream) {
    DANBO_CHECK_ARG(sigma && workspace && mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso));
    DANBO_CHECK_ARG((uintptr_t)sigma % 4 == 0 && (uintptr_t)workspace % 4 == 0);
    DANBO_CHECK_ARG(cap_v >= 0 && cap_t >= 0 && (verts || !cap_v) && (tris || !cap_t));
    DANBO_CHECK_ARG((uintptr_t)verts % 4 == 0 && (uintptr_t)tris % 4 == 0);
    DANBO_CHECK_ARG(finite_f(scale) && finite_f(off_x) && finite_f(off_y) && finite_f(off_z));
    const MeshGridArgs a = mesh_args(sigma, nx, ny, nz, stride_x, stride_y, floor, iso);
    const uint32_t* words = static_cast<const uint32_t*>(workspace);
    const int* voff = reinterpret_cast<const int*>(static_cast<const char*>(workspace) + mesh_words_bytes(a.n_pts));
    const int* toff = voff + a.n_chunks + 1;
    const int grid = stream_grid((long)a.n_chunks * MESH_CHUNK, MESH_CHUNK);
    if (cap_v > 0)
        hipLaunchKernelGGL(k_mesh_vertices, dim3(grid), dim3(MESH_CHUNK), 0, (hipStream_t)stream, a, words, voff, scale, off_x, off_y,
                           off_z, verts, cap_v);
    if (cap_t > 0)
        hipLaunchKernelGGL(k_mesh_triangles, dim3(grid), dim3(MESH_CHUNK), 0, (hipStream_t)stream, a, words, voff, toff, tris, cap_t);
    DANBO_LAUNCH_RET();
}

extern "C" int danbo_mesh_normals(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso,
                                  const void* workspace, float* normals, int cap_v, void* stream) {
    DANBO_CHECK_ARG(sigma && workspace && normals && mesh_dims_ok(nx, ny, nz, stride_x, stride_y, floor, iso) && cap_v >= 0);
    DANBO_CHECK_ARG((uintptr_t)sigma % 4 == 0 && (uintptr_t)workspace % 4 == 0 && (uintptr_t)normals % 4 == 0);
    const MeshGridArgs a = mesh_args(sigma, nx, ny, nz, stride_x, stride_y, floor, iso);
    const uint32_t* words = static_cast<const uint32_t*>(workspace);
    const int* voff = reinterpret_cast<const int*>(static_cast<const char*>(workspace) + mesh_words_bytes(a.n_pts));
    if (cap_v > 0)
        hipLaunchKernelGGL(k_mesh_normals, dim3(stream_grid((long)a.n_chunks * MESH_CHUNK, MESH_CHUNK)), dim3(MESH_CHUNK), 0,
                           (hipStream_t)stream, a, words, voff, normals, cap_v);
    DANBO_LAUNCH_RET();
}
