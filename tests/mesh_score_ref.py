"""Mesh scores (include/danbo_mesh_score.h): what the tests of csrc/mesh_score_math.hpp and csrc/k_mesh_score.hip share.

  * the host build of the header's serial restatement (tests/hostlib.py), called through ctypes: host_areas / host_sample /
    host_bary / host_nearest / host_score;
  * an independent statement of the same definitions in numpy float64 -- d2_64, nearest64, areas64, sample64, score64 -- written
    from the definitions with a brute-force argmin, sharing no code and no evaluation order with the header;
  * the cases both test files use, made once per process.

Bounds (u = 2^-24, the unit round-off of fp32; every input is an fp32 number, so the float64 statement reads exactly what the fp32
code reads; the float64 statement's own error, ~2^-53, is ignored beside them):
  nearest, d2      the issue's count: three squared differences, each a rounded subtraction squared, and two additions -- the
                   product d_x d_x and the two fma are the three roundings of the sum, each <= u relative to a partial sum of
                   non-negative terms, hence <= u of the whole: |d2_32 - d2_64| <= 3 u d2_64 (D2_REL = 3 u).  (The rounding of each
                   difference enters squared, (1 + e)^2 with |e| <= u, and is not counted by the issue; a strict first-order bound
                   that counts it is 5 u.  The test holds the issue's 3 u.)
  nearest, idx     the index the fp32 code picks is one whose float64 d2 lies within D2_REL of the float64 minimum: an acceptance
                   set, near-ties need no exclusion.
  sample point     b0 A, then two fma: three roundings on the path of the first term, two and one on the others:
                   |p_32 - p_64| <= ((1 + u)^3 - 1) (|b0 A| + |b1 B| + |b2 C|) with the fp32 weights b read exactly.
  weights          b0 = 1 - r has one rounding (<= u since b0 <= 1), b1 two (<= 2 u b1), b2 one (<= u b2) and r cancels exactly
                   in 1 - r + r (1 - u2) + r u2: |b0 + b1 + b2 - 1| <= 4 u (the issue's bound; 2 u by this count).
  normal           |n| = 1 within 4 u: len carries (3 u) / 2 from its three roundings under the root plus u of the root, each
                   quotient u more: 3.5 u.
  sums             N float64 additions on the longest path is a gross over-count (a chain of N / 16384 items and 14 tree steps),
                   so N 2^-53 relative to the sum of absolute terms covers the summation; the dot product of two unit normals
                   is an fp32 chain of three roundings: 3 u per term (|n . m| <= 1 + 8 u).
"""
import ctypes
import functools
import os

import numpy as np

import hostlib
from helpers import ROOT

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
D2_REL = 3 * U
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
EINVAL = -22
MAX_TAU = 8
SENTINEL = F32(-777.25)

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_face_areas(const float* verts, int V, const int32_t* faces, int F, float* areas, int32_t* flag) {
    return mesh_face_areas_host(verts, V, faces, F, areas, flag);
}
int ref_sample(const float* verts, int V, const int32_t* faces, int F, const float* cdf, const float* u, int M, float* pts, float* nrm,
               int32_t* face, int32_t* flag) {
    return mesh_sample_host(verts, V, faces, F, cdf, u, M, pts, nrm, face, flag);
}
void ref_bary(const float* u, int M, float* b) {
    for (long m = 0; m < M; ++m) mesh_bary(u[3 * m + 1], u[3 * m + 2], b + 3 * m, b + 3 * m + 1, b + 3 * m + 2);
}
int ref_nearest(const float* q, int Nq, const float* r, int Nr, float* d2, int32_t* idx) { return points_nearest_host(q, Nq, r, Nr, d2, idx); }
int ref_score(const float* d2, const int32_t* idx, const float* nq, const float* nr, int Nr, int N, const float* tau, int T, double* out) {
    return points_score_host(d2, idx, nq, nr, Nr, N, tau, T, out);
}
size_t ref_nearest_workspace(int Nq, int Nr) { return points_nearest_workspace_size(Nq, Nr); }
int ref_splits(int Nq, int Nr) { return points_splits(Nq, Nr); }
unsigned long long ref_key(float d2, int j) { return points_key(d2, j); }
int ref_tile() { return POINTS_TILE; }
}
'''
_P, _I = ctypes.c_void_p, ctypes.c_int


@functools.lru_cache(maxsize=None)
def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/mesh_score_math.hpp)"""
    lib = hostlib.build("mesh_score_ref", _WRAPPER % os.path.join(CSRC, "mesh_score_math.hpp"))
    lib.ref_face_areas.argtypes = [_P, _I, _P, _I, _P, _P]
    lib.ref_sample.argtypes = [_P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P]
    lib.ref_bary.argtypes, lib.ref_bary.restype = [_P, _I, _P], None
    lib.ref_nearest.argtypes = [_P, _I, _P, _I, _P, _P]
    lib.ref_score.argtypes = [_P, _P, _P, _P, _I, _I, _P, _I, _P]
    lib.ref_nearest_workspace.argtypes, lib.ref_nearest_workspace.restype = [_I, _I], ctypes.c_size_t
    lib.ref_splits.argtypes = [_I, _I]
    lib.ref_key.argtypes, lib.ref_key.restype = [ctypes.c_float, _I], ctypes.c_ulonglong
    return lib


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _a(x, dt):
    return np.ascontiguousarray(x, dt)


def _p(x):
    return None if x is None else x.ctypes.data


# ----------------------------------------------------------------------------- the header's restatement, called
def host_areas(verts, faces):
    """-> (areas [F] float32, flag) of the restatement"""
    verts, faces = _a(verts, F32), _a(faces, np.int32)
    areas, flag = np.full(len(faces), SENTINEL, F32), np.zeros(1, np.int32)
    rc = host_lib().ref_face_areas(_p(verts), len(verts), _p(faces), len(faces), _p(areas), _p(flag))
    assert rc == 0, rc
    return areas, int(flag[0])


def host_sample(verts, faces, cdf, u):
    """-> (pts [M,3], nrm [M,3], face [M], flag) of the restatement"""
    verts, faces, cdf, u = _a(verts, F32), _a(faces, np.int32), _a(cdf, F32), _a(u, F32)
    M = len(u)
    pts, nrm, face, flag = np.full((M, 3), SENTINEL, F32), np.full((M, 3), SENTINEL, F32), np.full(M, -7, np.int32), np.zeros(1, np.int32)
    rc = host_lib().ref_sample(_p(verts), len(verts), _p(faces), len(faces), _p(cdf), _p(u), M, _p(pts), _p(nrm), _p(face), _p(flag))
    assert rc == 0, rc
    return pts, nrm, face, int(flag[0])


def host_bary(u):
    """-> b [M,3] float32: the header's barycentric weights of u[:, 1:]"""
    u = _a(u, F32)
    b = np.empty((len(u), 3), F32)
    host_lib().ref_bary(_p(u), len(u), _p(b))
    return b


def host_nearest(q, r):
    """-> (d2 [Nq] float32, idx [Nq] int32) of the restatement"""
    q, r = _a(q, F32), _a(r, F32)
    d2, idx = np.full(len(q), SENTINEL, F32), np.full(len(q), -7, np.int32)
    rc = host_lib().ref_nearest(_p(q), len(q), _p(r), len(r), _p(d2), _p(idx))
    assert rc == 0, rc
    return d2, idx


def host_score(d2, idx, nq, nr, tau):
    """-> out [4 + T] float64 of the restatement"""
    d2, idx, tau = _a(d2, F32), _a(idx, np.int32), _a(tau, F32)
    nq, nr = (None, None) if nq is None else (_a(nq, F32), _a(nr, F32))
    out = np.full(4 + len(tau), np.nan, F64)
    rc = host_lib().ref_score(_p(d2), _p(idx), _p(nq), _p(nr), 0 if nr is None else len(nr), len(d2), _p(tau) if len(tau) else None,
                              len(tau), _p(out))
    assert rc == 0, rc
    return out


def host_chain(mesh_a, cdf_a, u_a, mesh_b, cdf_b, u_b, thresholds):
    """the restatement chained as score_meshes chains the kernels, on given cdf and u -> (sums a->b, sums b->a), float64 [4 + T]"""
    pa, na = host_sample(*mesh_a, cdf_a, u_a)[:2]
    pb, nb = host_sample(*mesh_b, cdf_b, u_b)[:2]
    tau = np.asarray(thresholds, F32)
    d_ab, i_ab = host_nearest(pa, pb)
    d_ba, i_ba = host_nearest(pb, pa)
    return host_score(d_ab, i_ab, na, nb, tau), host_score(d_ba, i_ba, nb, na, tau), (pa, na, pb, nb)


# ----------------------------------------------------------------------------- float64, from the definitions
def d2_64(q, r):
    """[Nq, Nr] float64: every squared distance (brute force)"""
    q, r = np.asarray(q, F64), np.asarray(r, F64)
    return sum((q[:, None, k] - r[None, :, k]) ** 2 for k in range(3))


def nearest64(q, r):
    """-> (min_j d2 [Nq], argmin [Nq], the whole table) in float64"""
    d = d2_64(q, r)
    j = d.argmin(1)
    return d[np.arange(len(d)), j], j, d


def nearest_rejects(got_d2, got_idx, q, r):
    """the queries at which (got_d2, got_idx) break the two bounds of the docstring -> (list, worst d2 error / d2, worst excess of
    the chosen index's float64 d2 over the minimum / minimum)"""
    dmin, _, table = nearest64(q, r)
    got_idx = np.asarray(got_idx)
    ok_idx = (got_idx >= 0) & (got_idx < len(r))
    own = table[np.arange(len(table)), np.where(ok_idx, got_idx, 0)]
    err = np.abs(np.asarray(got_d2, F64) - own)
    bad = ~ok_idx | (err > D2_REL * own) | (own - dmin > D2_REL * dmin)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(own > 0, err / own, 0.0).max()
        exc = np.where(dmin > 0, (own - dmin) / dmin, 0.0).max()
    return np.flatnonzero(bad).tolist(), float(rel), float(exc)


def areas64(verts, faces):
    v = np.asarray(verts, F64)[np.asarray(faces)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=-1)


def pick64(cdf, u0):
    """the face of every sample from the definition: the first f with cdf[f] > fp32(u0 cdf[F - 1]), F - 1 when there is none"""
    cdf = np.asarray(cdf, F32)
    target = (np.asarray(u0, F32) * cdf[-1]).astype(F32)
    return np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1).astype(np.int32)


def sample64(verts, faces, face, b):
    """-> (points [M,3], bound [M,3], unit normals [M,3] (zero on a degenerate face)) in float64 from the chosen faces and the fp32
    weights b [M,3] read exactly"""
    v = np.asarray(verts, F64)[np.asarray(faces)[np.asarray(face)]]                  # [M, 3 corners, 3]
    b = np.asarray(b, F64)
    pts = (b[:, :, None] * v).sum(1)
    bound = ((1 + U) ** 3 - 1) * (np.abs(b[:, :, None] * v)).sum(1)
    c = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    length = np.linalg.norm(c, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(length > 0, c / length, 0.0)
    return pts, bound, n


def score64(d2, idx, nq, nr, tau):
    """-> (out [4 + T] float64, bound [4 + T]) from the definitions: plain numpy sums; the counts are exact (bound 0)"""
    d2 = np.asarray(d2, F64)
    N, d = len(d2), np.sqrt(np.asarray(d2, F64))
    out, bound = np.zeros(4 + len(tau)), np.zeros(4 + len(tau))
    out[0], out[1], out[3] = d.sum(), d2.sum(), N
    bound[0], bound[1] = N * 2.0 ** -53 * d.sum(), N * 2.0 ** -53 * d2.sum()
    if nq is not None:
        dots = np.abs((np.asarray(nq, F64) * np.asarray(nr, F64)[np.asarray(idx)]).sum(-1))
        out[2] = dots.sum()
        bound[2] = N * 2.0 ** -53 * dots.sum() + 3 * U * (np.abs(np.asarray(nq, F64) * np.asarray(nr, F64)[np.asarray(idx)])).sum()
    for t, x in enumerate(tau):
        out[4 + t] = np.count_nonzero(d <= F64(F32(x)))
    return out, bound


def metrics64(ab, ba, thresholds):
    """the dict of score_points from two directions' sums, restated"""
    na, nb = ab[3], ba[3]
    out = dict(chamfer_l1=0.5 * (ab[0] / na + ba[0] / nb), chamfer_l2=ab[1] / na + ba[1] / nb,
               normal_consistency=0.5 * (ab[2] / na + ba[2] / nb), precision={}, recall={}, fscore={})
    for t, tau in enumerate(thresholds):
        p, r = ab[4 + t] / na, ba[4 + t] / nb
        out["precision"][tau], out["recall"][tau], out["fscore"][tau] = p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


# ----------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def icosphere(level=2, radius=1.0):
    """a subdivided icosahedron, every vertex pushed onto the sphere of `radius` -> (verts [V,3] float32, faces [F,3] int32);
    level 2: 162 vertices, 320 faces"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, F64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts, faces = (np.asarray(v) * radius).astype(F32), np.asarray(f, np.int32)
    verts.setflags(write=False), faces.setflags(write=False)
    return verts, faces


def longest_edge(verts, faces):
    v = np.asarray(verts, F64)[np.asarray(faces)]
    return float(max(np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=-1).max() for i in range(3)))


@functools.lru_cache(maxsize=None)
def degenerate_mesh():
    """a small mesh with faces of area zero (a repeated corner, three collinear corners, a leading one) and repeated faces ->
    (verts, faces); the last face has an area, so the clamp of the search never lands on a face of area zero"""
    rng = np.random.default_rng(3)
    verts = rng.uniform(-1, 1, (12, 3)).astype(F32)
    verts[9], verts[10], verts[11] = (0, 0, 0), (0.5, 0.25, 0.125), (1, 0.5, 0.25)          # collinear, exactly
    faces = np.array([(3, 3, 5), (0, 1, 2), (0, 1, 2), (9, 10, 11), (2, 3, 4), (4, 4, 4), (5, 6, 7), (2, 3, 4), (6, 7, 8), (1, 1, 0),
                      (7, 8, 0)], np.int32)
    verts.setflags(write=False), faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def one_face():
    verts = np.array([(0.25, -0.5, 1.0), (1.5, 0.75, -0.25), (-0.75, 1.25, 0.5)], F32)
    return verts, np.array([(0, 1, 2)], np.int32)


MESHES = {"icosphere": lambda: icosphere(2), "degenerate": degenerate_mesh, "one_face": one_face}
SAMPLE_M = (1, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def sample_case(name, M):
    """(verts, faces, cdf [F] float32: numpy's cumulative sum of the restatement's areas, u [M,3] in [0, 1)) and the restatement's
    result on it, computed once"""
    verts, faces = MESHES[name]()
    areas, flag = host_areas(verts, faces)
    assert flag == 0
    cdf = np.cumsum(areas, dtype=F32)
    u = np.random.default_rng(100 + M).random((M, 3), dtype=F32)
    assert u.max() < 1
    pts, nrm, face, flag = host_sample(verts, faces, cdf, u)
    assert flag == 0
    for a in (areas, cdf, u, pts, nrm, face):
        a.setflags(write=False)
    return dict(verts=verts, faces=faces, areas=areas, cdf=cdf, u=u, pts=pts, nrm=nrm, face=face)


def tile():
    return host_lib().ref_tile()


NEAREST_NQ = (1, 63, 64, 65, 1000)


def nearest_nr():
    t = tile()
    return (1, t - 1, t, t + 1, 3 * t + 7)


@functools.lru_cache(maxsize=None)
def nearest_case(Nq, Nr, kind="random"):
    """q [Nq,3], r [Nr,3] random fp32 in [-2, 2] and the restatement's (d2, idx) on them.  kind 'duplicates': a tenth of r are exact
    copies of other rows of r (the tie rule); 'self': the queries are the first Nq reference points (Nr >= Nq)"""
    rng = np.random.default_rng(7919 * Nq + Nr)
    q = rng.uniform(-2, 2, (Nq, 3)).astype(F32)
    r = rng.uniform(-2, 2, (Nr, 3)).astype(F32)
    if kind == "duplicates":
        n = max(1, Nr // 10)
        dst = rng.choice(Nr, n, replace=False)
        r[dst] = r[rng.integers(0, Nr, n)]
        q[: min(Nq, n)] = r[dst[: min(Nq, n)]] + F32(1e-3)          # queries whose nearest point exists at least twice
    elif kind == "self":
        assert Nr >= Nq
        q = r[:Nq].copy()
    d2, idx = host_nearest(q, r)
    for a in (q, r, d2, idx):
        a.setflags(write=False)
    return dict(q=q, r=r, d2=d2, idx=idx)


SCORE_N = (1, 64, 65, 4097)
SCORE_T = (1, 8)


@functools.lru_cache(maxsize=None)
def score_case(N, T, normals):
    """d2 [N], idx [N] into Nr = 37 reference normals, unit normals, T thresholds of which some equal sqrt(d2) of an item exactly
    (d2 = 0.0625 -> tau = 0.25) -> dict with the restatement's out"""
    rng = np.random.default_rng(31 * N + T)
    d2 = (rng.uniform(0, 0.3, N).astype(F32)) ** 2
    d2[::5] = F32(0.0625)
    d2[::7] = 0
    Nr = 37
    idx = rng.integers(0, Nr, N).astype(np.int32)
    unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(F32)      # noqa: E731
    nq, nr = (unit(rng.standard_normal((N, 3))), unit(rng.standard_normal((Nr, 3)))) if normals else (None, None)
    tau = np.array([0.25, 0.0, 0.1, 0.05, 0.2, 0.3, 1e-3, 0.15][:T], F32)
    out = host_score(d2, idx, nq, nr, tau)
    out.setflags(write=False)
    return dict(d2=d2, idx=idx, nq=nq, nr=nr, tau=tau, out=out)
