"""Helpers of the mesh-extraction tests (tests/test_mesh_extract.py, tests/test_gpu_mesh.py): the serial extractor of
csrc/mesh_math.hpp built with g++ at test time, the numpy predictions it is checked against, the test grids."""
import collections
import ctypes
import importlib.util
import os

import numpy as np

import hostlib
from helpers import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
GUARD = 0x5AFEC0DE        # guard word in front of and behind every buffer the extractor writes
N_GUARD = 16

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_mesh_count(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, int32_t* ws, int* counts) {
    return mesh_count_host(sigma, nx, ny, nz, sx, sy, floor, iso, ws, counts);
}
int ref_mesh_extract(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, const int32_t* ws,
                     float scale, float ox, float oy, float oz, float* verts, int cap_v, int* tris, int cap_t) {
    return mesh_extract_host(sigma, nx, ny, nz, sx, sy, floor, iso, ws, scale, ox, oy, oz, verts, cap_v, tris, cap_t);
}
unsigned long long ref_mc_case(int m) { return MC_CASE[m & 255]; }
}
'''


def host_lib():
    """g++ -std=c++17 -ffp-contract=off build of the serial extractor (csrc/mesh_math.hpp + csrc/mc_table.inc)"""
    lib = hostlib.build("mesh_ref", _WRAPPER % os.path.join(CSRC, "mesh_math.hpp"))
    c = ctypes
    lib.ref_mesh_count.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, c.c_float, c.c_float, c.c_void_p, c.c_void_p]
    lib.ref_mesh_extract.argtypes = ([c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, c.c_float, c.c_float, c.c_void_p]
                                     + [c.c_float] * 4 + [c.c_void_p, c.c_int, c.c_void_p, c.c_int])
    lib.ref_mc_case.restype = c.c_ulonglong
    return lib


def gen_table_module():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def guarded(n, dtype):
    """-> (whole buffer with N_GUARD guard words on either side, the view of the n payload elements)"""
    buf = np.full(n + 2 * N_GUARD, GUARD, np.uint32)
    return buf, buf[N_GUARD:N_GUARD + n].view(dtype)


def guards_intact(buf):
    return bool(np.all(buf[:N_GUARD] == GUARD) and np.all(buf[-N_GUARD:] == GUARD))


def host_extract(sigma, iso, floor=-np.inf, scale=1.0, offset=(0., 0., 0.), cap=None, check_guards=True):
    """The serial extractor on a float32 array whose innermost stride is 1 (a transposed view is passed as it is).
    -> verts [V,3] float32, faces [T,3] int32; cap = (cap_v, cap_t) limits what is written (the counts stay V, T)."""
    lib = host_lib()
    assert sigma.dtype == F32 and sigma.ndim == 3 and sigma.strides[2] == 4
    nx, ny, nz = sigma.shape
    sx, sy = sigma.strides[0] // 4, sigma.strides[1] // 4
    ptr = sigma.ctypes.data
    ws_buf, ws = guarded(nx * ny * nz, np.int32)
    cnt_buf, cnt = guarded(2, np.int32)
    rc = lib.ref_mesh_count(ptr, nx, ny, nz, sx, sy, floor, iso, ws.ctypes.data, cnt.ctypes.data)
    assert rc == 0, rc
    V, T = int(cnt[0]), int(cnt[1])
    cap_v, cap_t = (V, T) if cap is None else cap
    v_buf, verts = guarded(3 * max(cap_v, 1), F32)
    t_buf, tris = guarded(3 * max(cap_t, 1), np.int32)
    ws_before = ws.copy()
    rc = lib.ref_mesh_extract(ptr, nx, ny, nz, sx, sy, floor, iso, ws.ctypes.data, scale, *[float(x) for x in offset],
                              verts.ctypes.data, cap_v, tris.ctypes.data, cap_t)
    assert rc == 0, rc
    if check_guards:
        assert all(guards_intact(b) for b in (ws_buf, cnt_buf, v_buf, t_buf)), "a guard word was overwritten"
        assert np.array_equal(ws, ws_before)
    out_v = verts[:3 * cap_v].reshape(-1, 3).copy()
    out_t = tris[:3 * cap_t].reshape(-1, 3).copy()
    return (out_v, out_t) if cap is None else (out_v, out_t, V, T)


# ----------------------------------------------------------------------------- numpy predictions
def floored(sigma, floor):
    """the value the extraction reads: max(sigma, floor), a NaN as -inf"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(sigma), F32(-np.inf), np.maximum(sigma, F32(floor))).astype(F32)


def crossing_edges(sigma, iso, floor=-np.inf):
    """-> inside [nx,ny,nz] bool, p [V,3] int (lower ends), ax [V] int -- in the defined vertex order"""
    s = floored(sigma, floor)
    inside = s >= F32(iso)
    nx, ny, nz = s.shape
    keys, ps, axs = [], [], []
    for ax in range(3):
        d = np.diff(inside, axis=ax) != 0
        idx = np.argwhere(d)
        lin = (idx[:, 0] * ny + idx[:, 1]) * nz + idx[:, 2]
        keys.append(lin * 3 + ax)
        ps.append(idx)
        axs.append(np.full(len(idx), ax))
    keys, ps, axs = np.concatenate(keys), np.concatenate(ps), np.concatenate(axs)
    order = np.argsort(keys, kind="stable")
    return inside, ps[order], axs[order]


def vertex_positions_f64(sigma, iso, floor, p, ax):
    """float64 evaluation of p + t e_ax, t = (iso - s0) / (s1 - s0) (grids of finite values)"""
    s = floored(sigma, floor).astype(np.float64)
    q = p.copy()
    q[np.arange(len(p)), ax] += 1
    s0, s1 = s[p[:, 0], p[:, 1], p[:, 2]], s[q[:, 0], q[:, 1], q[:, 2]]
    t = np.clip((float(F32(iso)) - s0) / (s1 - s0), 0., 1.)       # (the threshold the extraction sees is a float32)
    pos = p.astype(np.float64)
    pos[np.arange(len(p)), ax] += t
    return pos, s0, s1


def cell_cases(inside):
    """-> [nx-1,ny-1,nz-1] int: the 8-bit mask of inside corners, corner number a + 2b + 4c"""
    nx, ny, nz = inside.shape
    m = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        a, b, cc = c & 1, (c >> 1) & 1, c >> 2
        m |= inside[a:a + nx - 1, b:b + ny - 1, cc:cc + nz - 1].astype(np.int64) << c
    return m


def directed_edges(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    return collections.Counter(map(tuple, e.tolist()))


def is_closed_oriented_manifold(faces):
    de = directed_edges(faces)
    return all(n == 1 and de.get((b, a), 0) == 1 for (a, b), n in de.items())


def euler_characteristic(n_verts, faces):
    return n_verts - len(directed_edges(faces)) // 2 + len(faces)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    return float(np.einsum("ij,ij->i", v[faces[:, 0]], np.cross(v[faces[:, 1]], v[faces[:, 2]])).sum() / 6.)


# ----------------------------------------------------------------------------- grids
def lattice(shape):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1)


CENTRE = np.array([13.3, 13.6, 13.1])


def sphere_grid(shape=(28, 28, 28), R=9.2, centre=CENTRE):
    return (R - np.linalg.norm(lattice(shape) - np.asarray(centre, np.float64), axis=-1)).astype(F32)


def torus_grid(shape=(28, 28, 28), major=8., minor=3., centre=CENTRE):
    d = lattice(shape) - centre
    return (minor - np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - major) ** 2 + d[..., 2] ** 2)).astype(F32)


def two_spheres_grid(shape=(28, 28, 28)):
    g = lattice(shape)
    a = 4.2 - np.linalg.norm(g - np.array([7.3, 8.1, 7.7]), axis=-1)
    b = 5.1 - np.linalg.norm(g - np.array([19.2, 18.6, 19.4]), axis=-1)
    return np.maximum(a, b).astype(F32)


def noise_grid(seed, shape=(28, 28, 28)):
    s = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = [F32(-5.)] * 6
    return s
