"""Helpers of the grid-component tests (tests/test_grid_cc_host.py, tests/test_gpu_grid_cc.py): the serial restatement of
csrc/grid_cc_math.hpp (grid_cc_host / grid_keep_host) built with g++ at test time, the scipy / numpy predictions it is checked
against, and the test grids."""
import ctypes
import functools
import os

import numpy as np
import pytest

import hostlib
import mesh_ref
from helpers import ROOT

ndimage = pytest.importorskip("scipy.ndimage")

F32 = np.float32
CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")
INF = float("inf")

_WRAPPER = '''#include "%s"
using namespace danbo;
extern "C" {
int ref_grid_cc(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, int32_t* labels, int32_t* sizes,
                int32_t* stats) {
    return grid_cc_host(sigma, nx, ny, nz, sx, sy, floor, iso, labels, sizes, stats);
}
int ref_grid_keep(const float* sigma, int nx, int ny, int nz, long sx, long sy, float floor, float iso, const int32_t* labels,
                  const int32_t* sizes, const int32_t* stats, int keep_largest, int min_points, float fill, float* out, long osx,
                  long osy, int32_t* kept) {
    return grid_keep_host(sigma, nx, ny, nz, sx, sy, floor, iso, labels, sizes, stats, keep_largest, min_points, fill, out, osx, osy, kept);
}
}
'''
_c = ctypes
_GRID = [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_long, _c.c_float, _c.c_float]
LABEL_ARGTYPES = _GRID + [_c.c_void_p] * 3
KEEP_ARGTYPES = _GRID + [_c.c_void_p] * 3 + [_c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_long, _c.c_long, _c.c_void_p]


def host_lib():
    """g++ -O2 -std=c++17 -ffp-contract=off build of the serial restatement (csrc/grid_cc_math.hpp)"""
    lib = hostlib.build("grid_cc_ref", _WRAPPER % os.path.join(CSRC, "grid_cc_math.hpp"))
    lib.ref_grid_cc.argtypes = LABEL_ARGTYPES
    lib.ref_grid_keep.argtypes = KEEP_ARGTYPES
    return lib


def grid_args(sigma, iso, floor):
    assert sigma.dtype == F32 and sigma.ndim == 3 and sigma.strides[2] == 4
    return (sigma.ctypes.data, *sigma.shape, sigma.strides[0] // 4, sigma.strides[1] // 4, float(floor), float(iso))


def host_label(sigma, iso=0., floor=-INF, want_sizes=True):
    """grid_cc_host on a float32 array whose innermost stride is 1 (a transposed view is passed as it is) -> labels [nx,ny,nz]
    int32, sizes (the same shape, or None), stats [4] int32; guard words around every output checked"""
    n = sigma.size
    l_buf, labels = mesh_ref.guarded(n, np.int32)
    s_buf, sizes = mesh_ref.guarded(n, np.int32)
    t_buf, stats = mesh_ref.guarded(4, np.int32)
    rc = host_lib().ref_grid_cc(*grid_args(sigma, iso, floor), labels.ctypes.data, sizes.ctypes.data if want_sizes else None,
                                stats.ctypes.data)
    assert rc == 0, rc
    assert all(mesh_ref.guards_intact(b) for b in (l_buf, s_buf, t_buf)), "a guard word was overwritten"
    if not want_sizes:
        assert np.all(sizes.view(np.uint32) == mesh_ref.GUARD)
    return labels.reshape(sigma.shape).copy(), sizes.reshape(sigma.shape).copy() if want_sizes else None, stats.copy()


def host_keep(sigma, iso, floor, labels, sizes, stats, keep_largest=False, min_points=0, fill=None, transposed_out=False, rc_only=False):
    """grid_keep_host -> out (float32, contiguous; transposed_out: written through the x-y transposed view of a [ny,nx,nz] array,
    so with strides that differ from a contiguous sigma's), kept [2] int32; guard words checked"""
    if fill is None:
        fill = default_fill(iso, floor)
    nx, ny, nz = sigma.shape
    o_buf, flat = mesh_ref.guarded(sigma.size, F32)
    out = flat.reshape(ny, nx, nz).transpose(1, 0, 2) if transposed_out else flat.reshape(nx, ny, nz)
    k_buf, kept = mesh_ref.guarded(2, np.int32)
    labels, sizes, stats = (np.ascontiguousarray(a, np.int32) for a in (labels, sizes, stats))
    rc = host_lib().ref_grid_keep(*grid_args(sigma, iso, floor), labels.ctypes.data, sizes.ctypes.data, stats.ctypes.data,
                                  int(keep_largest), int(min_points), float(fill), out.ctypes.data, out.strides[0] // 4,
                                  out.strides[1] // 4, kept.ctypes.data)
    if rc_only:
        return rc
    assert rc == 0, rc
    assert mesh_ref.guards_intact(o_buf) and mesh_ref.guards_intact(k_buf), "a guard word was overwritten"
    return np.ascontiguousarray(out), kept.copy()


def default_fill(iso, floor):
    """the default of core.grid_components.keep_components: floor where that is outside, else -inf"""
    return float(floor) if float(floor) < float(iso) else -INF


def filtered(sigma, iso=0., floor=-INF, **kw):
    """the restatement's two calls in a row -> out, kept, stats"""
    labels, sizes, stats = host_label(sigma, iso, floor)
    out, kept = host_keep(sigma, iso, floor, labels, sizes, stats, **kw)
    return out, kept, stats


# ----------------------------------------------------------------------------- scipy / numpy predictions
def inside_set(sigma, iso=0., floor=-INF):
    return mesh_ref.floored(sigma, floor) >= F32(iso)


def predict(sigma, iso=0., floor=-INF):
    """-> labels, sizes, stats by the definitions: scipy.ndimage.label with its default (6-connected) structure, made canonical
    with ndimage.minimum over the logical linear index"""
    inside = inside_set(np.ascontiguousarray(sigma), iso, floor)
    lab, n = ndimage.label(inside)
    lin = np.arange(inside.size, dtype=np.int64).reshape(inside.shape)
    labels = np.full(inside.shape, -1, np.int32)
    sizes = np.zeros(inside.shape, np.int32)
    stats = np.array([0, 0, 0, -1], np.int32)
    if n:
        firsts = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, n + 1))).astype(np.int64)
        labels[inside] = firsts[lab[inside] - 1]
        counts = np.bincount(lab[inside], minlength=n + 1)[1:]
        sizes.reshape(-1)[firsts] = counts
        big = counts.max()
        stats[:] = [inside.sum(), n, big, firsts[counts == big].min()]
    return labels, sizes, stats


def predict_keep(sigma, labels, sizes, stats, keep_largest, min_points, fill):
    """-> out, kept by the keep rule, in numpy"""
    sigma = np.ascontiguousarray(sigma)
    inside = labels >= 0
    size_of = sizes.reshape(-1)[np.where(inside, labels, 0)]
    keep = inside & (size_of >= min_points) & ((not keep_largest) | (labels == stats[3]))
    out = sigma.copy()
    out[inside & ~keep] = F32(fill)
    roots = keep & (labels == np.arange(labels.size).reshape(labels.shape))
    return out, np.array([roots.sum(), keep.sum()], np.int32)


# ----------------------------------------------------------------------------- grids
def signs(inside):
    return np.where(inside, F32(1), F32(-1)).astype(F32)


def serpentine_plane(ny=9, nz=67):
    m = np.zeros((ny, nz), bool)
    m[0::2] = True
    for j in range(1, ny, 2):
        m[j, nz - 1 if (j // 2) % 2 == 0 else 0] = True
    return m


def serpentine_grid():
    m = np.zeros((5, 9, 67), bool)
    m[0::2] = serpentine_plane()
    return signs(m)


def snake_grid():
    m = np.zeros((9, 9, 67), bool)
    m[0::2] = serpentine_plane()
    for n, i in enumerate(range(1, 9, 2)):
        m[i, 8 if n % 2 == 0 else 0, 0] = True
    return signs(m)


BERNOULLI_P = (0.25, 0.3116, 0.5)


def bernoulli_grid(p, n=64, seed=0):
    return signs(np.random.default_rng(seed).random((n, n, n)) < p)


SMALL_SHAPES = ((2, 2, 2), (2, 3, 1024), (3, 5, 65))


def small_grids(shape):
    """-> [(tag, sigma, iso, floor)]"""
    rng = np.random.default_rng(sum(shape))
    one = np.full(shape, -1, F32)
    one[tuple(s // 2 for s in shape)] = 1
    odd = rng.standard_normal(shape).astype(F32)
    flat = odd.reshape(-1)
    flat[rng.choice(flat.size, 3, replace=False)] = [np.nan, np.inf, -np.inf]
    flat[0] = np.nan
    return [("all_inside", np.ones(shape, F32), 0., -INF), ("all_outside", -np.ones(shape, F32), 0., -INF), ("one_point", one, 0., -INF),
            ("nan_inf", odd, 0., -INF), ("floor0_iso10", rng.uniform(0, 20, shape).astype(F32), 10., 0.)]


@functools.lru_cache(maxsize=None)
def cases():
    """every grid of the tests: {name: (sigma, iso, floor)}; the arrays are shared, nobody writes them"""
    out = {"two_spheres": (mesh_ref.two_spheres_grid(), 0., -INF), "noise0": (mesh_ref.noise_grid(0), 0., -INF),
           "noise1": (mesh_ref.noise_grid(1), 0., -INF), "serpentine": (serpentine_grid(), 0., -INF), "snake": (snake_grid(), 0., -INF)}
    for p in BERNOULLI_P:
        out[f"bernoulli_{p}"] = (bernoulli_grid(p), 0., -INF)
    for shape in SMALL_SHAPES:
        for tag, sigma, iso, floor in small_grids(shape):
            out["%s_%dx%dx%d" % ((tag,) + shape)] = (sigma, iso, floor)
    for sigma, _, _ in out.values():
        sigma.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's labels, sizes, stats of a case, computed once"""
    sigma, iso, floor = cases()[name]
    ref = host_label(sigma, iso, floor)
    for a in ref:
        a.setflags(write=False)
    return ref


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
