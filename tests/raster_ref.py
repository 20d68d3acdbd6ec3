"""Helpers of the rasteriser tests (tests/test_raster_host.py, tests/test_gpu_raster.py): the serial rasteriser of
csrc/raster_math.hpp built with g++ at test time, the numpy predictions it is checked against (integer coverage, float64 depth and
colour), the test scenes."""
import ctypes
import functools
import os

import numpy as np

import hostlib
import mesh_ref
from helpers import ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
GUARD = mesh_ref.GUARD
N_GUARD = mesh_ref.N_GUARD
COLOR, NORMAL, FLAT = 0, 1, 2
MODES = {"color": COLOR, "normal": NORMAL, "flat": FLAT}
TOL = 64 * 2.0 ** -24            # fewer than 64 fp32 roundings of at most 2^-24 each on values <= 1

_WRAPPER = '''#include <stddef.h>
#include <string.h>
#include "%s"
using namespace danbo;
extern "C" {
size_t ref_raster_workspace_bytes(int n_verts, int height, int width) { return raster_workspace_size(n_verts, height, width); }
int ref_raster_mesh(const float* verts, int n_verts, const int* tris, int n_tris, const float* attr, int mode, const float* views,
                    int n_views, float hx, int H, int W, const float* background, void* workspace, float* rgb, float* depth, int* tri_id) {
    return raster_mesh_host(verts, n_verts, tris, n_tris, attr, mode, views, n_views, hx, H, W, background, workspace, rgb, depth, tri_id);
}
void ref_raster_vertices(const float* verts, int n_verts, const float* attr, int mode, const float* M, float hx, int H, int W,
                         int* X, int* Y, float* z, int* valid, float* col) {
    for (int v = 0; v < n_verts; ++v) {
        float p[3];
        raster_view_point(M, verts + 3 * v, p);
        const RasterVertex o = raster_vertex(p, hx, H, W);
        X[v] = o.X; Y[v] = o.Y; z[v] = o.z; valid[v] = o.valid;
        raster_vertex_color(mode, M, attr ? attr + 3 * v : nullptr, p, col + 3 * v);
    }
}
unsigned long long ref_raster_key(float depth, int tri) { return raster_key(depth, tri); }
}
'''


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial rasteriser (csrc/raster_math.hpp)"""
    lib = hostlib.build("raster_ref", _WRAPPER % os.path.join(CSRC, "raster_math.hpp"))
    c = ctypes
    lib.ref_raster_workspace_bytes.argtypes = [c.c_int] * 3
    lib.ref_raster_workspace_bytes.restype = c.c_size_t
    lib.ref_raster_mesh.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_float, c.c_int,
                                    c.c_int] + [c.c_void_p] * 5
    lib.ref_raster_vertices.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_float, c.c_int, c.c_int] + [c.c_void_p] * 5
    lib.ref_raster_key.argtypes = [c.c_float, c.c_int]
    lib.ref_raster_key.restype = c.c_ulonglong
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, F32)


def host_vertices(verts, attr, mode, view, hx, H, W):
    """the vertex stage of the serial code for one view -> X, Y (int32, 1/256 pixel), z, valid, col [V,3]"""
    verts, attr, view = _f32(verts), _f32(attr), _f32(view).reshape(12)
    V = len(verts)
    X, Y, valid = (np.zeros(max(V, 1), np.int32) for _ in range(3))
    z, col = np.zeros(max(V, 1), F32), np.zeros((max(V, 1), 3), F32)
    host_lib().ref_raster_vertices(_ptr(verts), V, _ptr(attr), mode, _ptr(view), hx, H, W, *(_ptr(a) for a in (X, Y, z, valid, col)))
    return X[:V], Y[:V], z[:V], valid[:V].astype(bool), col[:V]


def host_raster(verts, faces, attr, mode, views, hx, H, W, background=(1., 1., 1.), want=("rgb", "depth", "tri_id")):
    """The serial rasteriser -> {'rgb': [n,H,W,3] float32, 'depth': [n,H,W] float32, 'tri_id': [n,H,W] int32} for the outputs in
    `want`; guard words around the workspace and every output are checked."""
    lib = host_lib()
    verts, attr, bg = _f32(verts).reshape(-1, 3), _f32(attr), _f32(background)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    views = _f32(views).reshape(-1, 12)
    n = len(views)
    n_bytes = lib.ref_raster_workspace_bytes(len(verts), H, W)
    assert n_bytes > 0 and n_bytes % 4 == 0
    ws_buf, ws = mesh_ref.guarded(n_bytes // 4, np.uint32)
    shapes = {"rgb": ((n, H, W, 3), F32), "depth": ((n, H, W), F32), "tri_id": ((n, H, W), np.int32)}
    bufs = {k: mesh_ref.guarded(int(np.prod(shapes[k][0])), shapes[k][1]) for k in want}
    ins = [a.copy() for a in (verts, faces, views, bg)]
    rc = lib.ref_raster_mesh(_ptr(verts), len(verts), _ptr(faces), len(faces), _ptr(attr), mode, _ptr(views), n, hx, H, W, _ptr(bg),
                             ws.ctypes.data, *(bufs[k][1].ctypes.data if k in bufs else None for k in ("rgb", "depth", "tri_id")))
    assert rc == 0, rc
    assert mesh_ref.guards_intact(ws_buf) and all(mesh_ref.guards_intact(b) for b, _ in bufs.values()), "a guard word was overwritten"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ins, (verts, faces, views, bg)))
    return {k: bufs[k][1].reshape(shapes[k][0]).copy() for k in want}


# ----------------------------------------------------------------------------- numpy predictions
def vertex_stage_f64(verts, view, hx, H, W):
    """float64 evaluation of the vertex stage -> 256 x_pix, 256 y_pix (not rounded), p [V,3]"""
    M = np.asarray(view, np.float64).reshape(3, 4)
    p = np.asarray(verts, np.float64) @ M[:, :3].T + M[:, 3]
    hx = float(F32(hx))
    return 256. * (p[:, 0] / (2 * hx) + 0.5) * W, 256. * (0.5 * H - p[:, 1] * (W / (2 * hx))), p


def normal_colors_f64(normals, view):
    M = np.asarray(view, np.float64).reshape(3, 4)[:, :3]
    n = np.asarray(normals, np.float64) @ M.T
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return 0.5 * np.where(ln > 0, n / np.where(ln > 0, ln, 1.), 0.) + 0.5


def flat_colors_f64(p, faces):
    """0.5 n + 0.5 of the unit normal of cross(B - A, C - A), per triangle, from the view-space positions p (0.5 where it has no length)"""
    a, b, c = (p[faces[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return 0.5 * np.where(ln > 0, n / np.where(ln > 0, ln, 1.), 0.) + 0.5


def flat_tolerance(p, faces):
    """Per triangle, how far the fp32 FLAT colour may lie from flat_colors_f64 of the SAME fp32 corners p: with u = B - A, v = C - A
    (one rounding each, relative 2^-24 = e) a component of u x v is two products and a difference, (3 + 3 + 1) e |u| |v| off at
    most; the vector sqrt(3) times that, 12.2 e |u| |v|; as a direction 12.2 e k with k = |u| |v| / |u x v| >= 1 (1 / sin of the
    corner's angle: a sliver's normal is ill-conditioned); the normalisation adds 5 e (three roundings under the root, the root, the
    division), the colour halves it and rounds once: (6.1 k + 3.5) e, stated as (8 k + 4) 2^-24."""
    a, b, c = (np.asarray(p, np.float64)[faces[:, k]] for k in range(3))
    lu, lv, lc = np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return 2.0 ** -24 * (8 * lu * lv / np.maximum(lc, 1e-300) + 4)


def _owns(E, dx, dy):
    return (E > 0) | ((E == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))


def predict(X, Y, valid, faces, H, W, z=None, col=None, tri_col=None):
    """The image the definitions predict from snapped vertices (X, Y: integers, 1/256 pixel): exact integer coverage, and in
    float64 the depth / colour of the nearest triangle.
    -> dict: count [H,W] (triangles covering the pixel), signed [H,W] (+1 per triangle of positive area2, -1 per negative),
       tri [H,W] (winner: largest float64 depth, lowest index at equal depth; -1: none), depth, second [H,W] float64 (largest and
       second largest depth), rgb [H,W,3] float64 (with col [V,3] per vertex or tri_col [T,3] per triangle)."""
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    assert np.abs(X).max(initial=0) < 2 ** 28 and np.abs(Y).max(initial=0) < 2 ** 28      # products of differences fit an int64
    count, signed = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    tri = np.full((H, W), -1, np.int64)
    depth, second = np.full((H, W), -np.inf), np.full((H, W), -np.inf)
    rgb = np.zeros((H, W, 3))
    V = len(X)
    for t, f in enumerate(np.asarray(faces, np.int64).reshape(-1, 3)):
        if f.min() < 0 or f.max() >= V or not valid[f].all():
            continue
        ia, ib, ic = (int(i) for i in f)
        area2 = int(X[ib] - X[ia]) * int(Y[ic] - Y[ia]) - int(Y[ib] - Y[ia]) * int(X[ic] - X[ia])
        if area2 == 0:
            continue
        sign = 1 if area2 > 0 else -1
        if area2 < 0:
            ib, ic, area2 = ic, ib, -area2
        xs, ys = X[[ia, ib, ic]], Y[[ia, ib, ic]]
        c0, c1 = max(-((128 - int(xs.min())) // 256), 0), min((int(xs.max()) - 128) // 256, W - 1)
        r0, r1 = max(-((128 - int(ys.min())) // 256), 0), min((int(ys.max()) - 128) // 256, H - 1)
        if c0 > c1 or r0 > r1:
            continue
        px = (256 * np.arange(c0, c1 + 1, dtype=np.int64) + 128)[None, :]
        py = (256 * np.arange(r0, r1 + 1, dtype=np.int64) + 128)[:, None]
        w = []
        inside = np.ones((r1 - r0 + 1, c1 - c0 + 1), bool)
        for u, v in ((1, 2), (2, 0), (0, 1)):
            dx, dy = xs[v] - xs[u], ys[v] - ys[u]
            E = dx * (py - ys[u]) - dy * (px - xs[u])
            inside &= _owns(E, dx, dy)
            w.append(E)
        if not inside.any():
            continue
        sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        count[sl] += inside
        signed[sl] += sign * inside
        if z is None:
            continue
        b = [wk / float(area2) for wk in w]
        d = b[0] * z[ia] + b[1] * z[ib] + b[2] * z[ic]
        wins = inside & (d > depth[sl])
        runner = inside & ~wins & (d > second[sl])
        second[sl] = np.where(wins, depth[sl], np.where(runner, d, second[sl]))
        depth[sl] = np.where(wins, d, depth[sl])
        tri[sl] = np.where(wins, t, tri[sl])
        if tri_col is not None:
            rgb[sl] = np.where(wins[..., None], tri_col[t], rgb[sl])
        elif col is not None:
            c = b[0][..., None] * col[ia] + b[1][..., None] * col[ib] + b[2][..., None] * col[ic]
            rgb[sl] = np.where(wins[..., None], c, rgb[sl])
    return dict(count=count, signed=signed, tri=tri, depth=depth, second=second, rgb=rgb)


# ----------------------------------------------------------------------------- views and scenes
def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def view_matrix(rx=0., ry=0., rz=0., scale=1., centre=(0., 0., 0.), shift=(0., 0., 0.)):
    """x -> scale R (x - centre) + shift as a [12] float32 view"""
    R = scale * rotation(rx, ry, rz)
    return np.concatenate([R, (np.asarray(shift, np.float64) - R @ np.asarray(centre, np.float64))[:, None]], axis=1).astype(F32).reshape(12)


def pixel_scene(px, py, z, H, W):
    """vertices that land on the pixel coordinates (px, py) (exactly, where W is a power of two) under the identity view with
    half_extent = W / 2: x_pix = x + W / 2, y_pix = H / 2 - y  -> verts [V,3] float32, view [12], half_extent"""
    px, py, z = (np.asarray(a, np.float64) for a in (px, py, z))
    verts = np.stack([px - W / 2., H / 2. - py, z], axis=1).astype(F32)
    return verts, view_matrix(), W / 2.


MESH_VIEWS = [view_matrix(0.3, 0.7, -0.2, 1. / 26, mesh_ref.CENTRE, (0.03, -0.02, 0.1)),
              view_matrix(-1.1, 2.9, 0.4, 1. / 31, mesh_ref.CENTRE, (-0.05, 0.04, -0.2)),
              view_matrix(2.2, -0.6, 1.3, 1. / 24, mesh_ref.CENTRE, (0., 0., 0.))]
MESH_HX = 0.6


@functools.lru_cache(maxsize=None)
def closed_mesh(name):
    """-> verts [V,3] float32 (index units), faces [T,3] int32, normals [V,3] float32 (unit, radial-ish: towards the outside of the
    density), colours [V,3] float32 in [0, 1]"""
    grid = {"sphere": mesh_ref.sphere_grid, "torus": mesh_ref.torus_grid, "two_spheres": mesh_ref.two_spheres_grid}[name]()
    v, f = mesh_ref.host_extract(grid, 0.)
    g = np.stack(np.gradient(grid.astype(np.float64)), -1)
    idx = np.clip(np.rint(v).astype(int), 0, np.array(grid.shape) - 1)
    n = -g[idx[:, 0], idx[:, 1], idx[:, 2]]
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
    col = np.random.default_rng(len(v)).random((len(v), 3))
    return v, f, n.astype(F32), col.astype(F32)
