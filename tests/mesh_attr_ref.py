"""Helpers of the vertex-normal tests (tests/test_mesh_normals.py, tests/test_gpu_mesh_attrs.py): the serial restatement
mesh_normals_host of csrc/mesh_math.hpp built with g++ at test time, an independent float64 numpy evaluation of the definition it
is checked against, the grids of the definition's edges."""
import ctypes
import os

import numpy as np

import hostlib
import mesh_ref as m

F32 = np.float32

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_mesh_count(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, int32_t* ws, int* counts) {
    return mesh_count_host(sigma, nx, ny, nz, sx, sy, floor, iso, ws, counts);
}
int ref_mesh_normals(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, const int32_t* ws,
                     float* normals, int cap_v) {
    return mesh_normals_host(sigma, nx, ny, nz, sx, sy, floor, iso, ws, normals, cap_v);
}
}
'''


def host_lib():
    """g++ -std=c++17 -ffp-contract=off build of mesh_normals_host (as mesh_ref.host_lib builds the extractor)"""
    lib = hostlib.build("mesh_attr_ref", _WRAPPER % os.path.join(m.CSRC, "mesh_math.hpp"))
    c = ctypes
    grid = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, c.c_float, c.c_float, c.c_void_p]
    lib.ref_mesh_count.argtypes = grid + [c.c_void_p]
    lib.ref_mesh_normals.argtypes = grid + [c.c_void_p, c.c_int]
    return lib


def host_normals(sigma, iso, floor=-np.inf, cap_v=None):
    """mesh_normals_host on a float32 array whose innermost stride is 1 -> normals [V,3] float32 (cap_v: the first cap_v rows);
    guard words around every buffer"""
    lib = host_lib()
    assert sigma.dtype == F32 and sigma.ndim == 3 and sigma.strides[2] == 4
    nx, ny, nz = sigma.shape
    grid = (sigma.ctypes.data, nx, ny, nz, sigma.strides[0] // 4, sigma.strides[1] // 4, floor, iso)
    ws_buf, ws = m.guarded(nx * ny * nz, np.int32)
    cnt_buf, cnt = m.guarded(2, np.int32)
    assert lib.ref_mesh_count(*grid, ws.ctypes.data, cnt.ctypes.data) == 0
    V = int(cnt[0])
    cap = V if cap_v is None else cap_v
    n_buf, nrm = m.guarded(3 * max(cap, 1), F32)
    ws_before = ws.copy()
    assert lib.ref_mesh_normals(*grid, ws.ctypes.data, nrm.ctypes.data, cap) == 0
    assert all(m.guards_intact(b) for b in (ws_buf, cnt_buf, n_buf)), "a guard word was overwritten"
    assert np.array_equal(ws, ws_before)
    return nrm[:3 * cap].reshape(-1, 3).copy()


# ----------------------------------------------------------------------------- float64 evaluation of the definition
def gradient_f64(sigma, floor):
    """-> [nx,ny,nz,3] float64: central differences inside, one-sided on the faces, a difference that is not finite as 0"""
    s = m.floored(sigma, floor).astype(np.float64)
    g = np.zeros(s.shape + (3,))
    with np.errstate(invalid="ignore"):
        for a in range(3):
            v = np.moveaxis(s, a, 0)
            d = np.empty_like(v)
            d[1:-1] = 0.5 * (v[2:] - v[:-2])
            d[0], d[-1] = v[1] - v[0], v[-1] - v[-2]
            g[..., a] = np.moveaxis(np.where(np.isfinite(d), d, 0.), 0, a)
    return g


def normals_f64(sigma, iso, floor=-np.inf):
    """-> n64 [V,3], fallback [V] bool, g0 [V,3], g1 [V,3] (the gradients at the two ends), p [V,3], ax [V] in vertex order
    (grids of finite values)"""
    _, p, ax = m.crossing_edges(sigma, iso, floor)
    k = np.arange(len(p))
    pos, s0, s1 = m.vertex_positions_f64(sigma, iso, floor, p, ax)
    t = pos[k, ax] - p[k, ax]
    q = p.copy()
    q[k, ax] += 1
    g = gradient_f64(sigma, floor)
    g0, g1 = g[p[:, 0], p[:, 1], p[:, 2]], g[q[:, 0], q[:, 1], q[:, 2]]
    gv = g0 + t[:, None] * (g1 - g0)
    fallback = np.abs(gv).max(-1) == 0
    axis_n = np.zeros_like(gv)
    axis_n[k, ax] = np.where(s0 >= float(F32(iso)), 1., -1.)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.where(fallback[:, None], axis_n, -gv / np.linalg.norm(gv, axis=-1, keepdims=True))
    return n, fallback, g0, g1, p, ax


def face_normals(verts, faces):
    v = verts.astype(np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])


# ----------------------------------------------------------------------------- grids
def quadric_grid(shape=(24, 24, 24), centre=(12, 11, 13), R2=64.5):
    """R^2 - |q - c|^2 with an integer centre: every value and every difference is exact in fp32"""
    d = m.lattice(shape) - np.asarray(centre, np.float64)
    return (R2 - (d ** 2).sum(-1)).astype(F32)


def alternating_grid():
    """-1, 1, -1, 1, -1 along x, constant along y and z: on the edges 1 -> 2 and 2 -> 3 both ends have a zero gradient"""
    return np.broadcast_to(np.array([-1., 1., -1., 1., -1.], F32)[:, None, None], (5, 2, 2)).copy()


def wild_grid(seed=21, shape=(20, 21, 22)):
    """white noise with 300 NaN, 300 +inf and 300 -inf entries"""
    rng = np.random.default_rng(seed)
    wild = (rng.standard_normal(shape) * 4).astype(F32)
    for val in (np.nan, np.inf, -np.inf):
        wild.ravel()[rng.choice(wild.size, 300, replace=False)] = val
    return wild
