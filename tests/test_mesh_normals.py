"""Vertex normals of the extracted meshes (csrc/mesh_math.hpp: mesh_normals_host, the scalar code k_mesh_normals inlines, compiled
by g++ at test time) on the CPU: against an independent float64 numpy evaluation of the definition, exactly on a quadric, oriented
like the triangles, on the edges of the definition; plus the library's host-side argument checks, the four .ply layouts and the
two flags of run_render."""
import ctypes
import os

import numpy as np
import pytest

import mesh_attr_ref as a
import mesh_ref as m
from helpers import ROOT

F32 = np.float32
U = 2.0 ** -24


def smooth_grids():
    return dict(sphere=m.sphere_grid(), torus=m.torus_grid(), two_spheres=m.two_spheres_grid())


def f64_cases():
    out = {k: (g, 0., -np.inf) for k, g in smooth_grids().items()}
    out.update(noise0=(m.noise_grid(0), 0., -np.inf), noise1=(m.noise_grid(1), 0., -np.inf))
    rng = np.random.default_rng(11)
    out["floored noise"] = ((rng.standard_normal((19, 12, 23)) * 5 - 1).astype(F32), 2., 0.)
    out["all six faces"] = (m.sphere_grid((12, 12, 12), R=6.3, centre=(5.5, 5.4, 5.6)), 0., -np.inf)
    out["2x2x2"] = (np.array([[[1., -1.], [-1., -1.]], [[-1., -1.], [-1., 2.]]], F32), 0., -np.inf)
    return out


def check_against_f64(sigma, iso, floor, name=""):
    """|n - n64| <= 2 |delta| / |g64| + 2^-22 per vertex, delta_a = 2^-22 (|g_a(p)| + |g_a(p + e)|): one rounding per difference,
    one for the interpolation, the 1.8e-7 of t, three for the normalisation; the fallback vertices exactly.  No vertex is left out."""
    n = a.host_normals(sigma, iso, floor)
    n64, fallback, g0, g1, p, ax = a.normals_f64(sigma, iso, floor)
    assert n.shape == n64.shape and n.dtype == F32
    assert np.array_equal(n[fallback].astype(np.float64), n64[fallback])
    ok = ~fallback
    k = np.arange(len(p))[ok]
    t = (m.vertex_positions_f64(sigma, iso, floor, p, ax)[0][np.arange(len(p)), ax] - p[np.arange(len(p)), ax])[:, None]
    g64 = np.linalg.norm(g0 + t * (g1 - g0), axis=-1)[ok]
    delta = np.linalg.norm(2.0 ** -22 * (np.abs(g0) + np.abs(g1)), axis=-1)[ok]
    err = np.linalg.norm(n[ok].astype(np.float64) - n64[ok], axis=-1)
    bound = 2 * delta / g64 + 2.0 ** -22
    print(name, "V", len(n), "fallback", int(fallback.sum()), "max |n - n64| / bound", float((err / bound).max()) if len(k) else 0.,
          "max |n - n64|", float(err.max()) if len(k) else 0.)
    assert np.all(err <= bound)
    return n


# ----------------------------------------------------------------------------- 1. float64
@pytest.mark.parametrize("name", sorted(f64_cases()))
def test_serial_normals_against_float64(name):
    sigma, iso, floor = f64_cases()[name]
    n = check_against_f64(sigma, iso, floor, name)
    assert len(n) > 0 and np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1) <= 4 * U)


def test_strided_view_is_read_through_its_strides():
    base = m.sphere_grid()
    view = np.ascontiguousarray(base.transpose(1, 0, 2)).transpose(1, 0, 2)
    assert not view.flags.c_contiguous and view.strides[2] == 4
    assert a.host_normals(view, 0.).tobytes() == a.host_normals(base, 0.).tobytes()


# ----------------------------------------------------------------------------- 2. exact on a quadric
def test_normals_of_a_quadric_are_the_radial_directions():
    """sigma = R^2 - |q - c|^2, integer c: central differences of a quadratic are exact, the interpolated gradient is -2 (v - c) at
    the vertex v, so n = (v - c) / |v - c| within 1e-6 (v = fl(p + t): 24 * 2^-24 / 8; the rest a few 2^-24)"""
    c = (12, 11, 13)
    sigma = a.quadric_grid(centre=c)
    v, f = m.host_extract(sigma, 0.)
    assert v.min() >= 1 and v.max() <= 22 and len(v) > 500                       # both ends of every edge have central differences
    n = a.host_normals(sigma, 0.)
    r = v.astype(np.float64) - np.asarray(c, np.float64)
    want = r / np.linalg.norm(r, axis=-1, keepdims=True)
    err = np.abs(n.astype(np.float64) - want).max()
    print("quadric: V", len(v), "max |n - (v - c) / |v - c||", err)
    assert err <= 1e-6


# ----------------------------------------------------------------------------- 3. orientation
def corner_dots(sigma, iso=0.):
    v, f = m.host_extract(sigma, iso)
    n = a.host_normals(sigma, iso).astype(np.float64)
    fn = a.face_normals(v, f)
    return np.einsum("fcj,fj->fc", n[f], fn), fn


@pytest.mark.parametrize("name", sorted(smooth_grids()))
def test_normals_point_the_way_the_triangles_do(name):
    dots, fn = corner_dots(smooth_grids()[name])
    assert len(dots) > 100 and np.all(np.linalg.norm(fn, axis=-1) > 0)
    print(name, "faces", len(dots), "min n_v . face normal", float(dots.min()))
    assert np.all(dots > 0)


def test_orientation_share_on_white_noise_is_reported():
    dots, fn = corner_dots(m.noise_grid(0))
    live = np.linalg.norm(fn, axis=-1) > 0
    print("white noise: share of corners with n_v . face normal > 0:", float((dots[live] > 0).mean()), "of", int(live.sum()) * 3)


# ----------------------------------------------------------------------------- 4. edges of the definition
def test_one_sided_gradients_on_the_smallest_grid():
    """2 x 2 x 2: every difference is one-sided; against the definition written out by hand"""
    s = np.array([[[1., -1.], [-1., -1.]], [[-1., -1.], [-1., 2.]]], F32)
    n = a.host_normals(s, 0.)
    _, p, ax = m.crossing_edges(s, 0.)
    assert len(n) == len(p) == 6
    for row, (q, e) in zip(n, zip(p, ax)):
        q1 = q.copy()
        q1[e] += 1
        grad = lambda u: np.array([float(s[tuple(np.where(np.arange(3) == c, 1, u))]) - float(s[tuple(np.where(np.arange(3) == c, 0, u))])  # noqa: E731
                                   for c in range(3)])
        s0, s1 = float(s[tuple(q)]), float(s[tuple(q1)])
        g = grad(q) + (0. - s0) / (s1 - s0) * (grad(q1) - grad(q))
        assert np.abs(row - (-g / np.linalg.norm(g))).max() <= 4 * U


def test_surface_touching_all_six_faces():
    sigma, iso, floor = f64_cases()["all six faces"]
    v, _ = m.host_extract(sigma, iso)
    for c in range(3):
        assert np.any(v[:, c] == 0) and np.any(v[:, c] == sigma.shape[c] - 1)
    check_against_f64(sigma, iso, floor, "all six faces")


def test_plateau_clamped_by_the_floor():
    """v = max(i - 3.5, 0) along x, iso 0.25: the crossing edge 3 -> 4 has t = 0.5, gradients 0.25 and 0.75 at its ends: n = -e_x
    exactly; the floored white noise of check 1 holds the float64 bound"""
    s = np.broadcast_to((np.arange(8, dtype=F32) - F32(3.5))[:, None, None], (8, 3, 3)).copy()
    n = a.host_normals(s, 0.25, 0.)
    assert len(n) == 9 and np.array_equal(n, np.tile(np.array([-1., 0., 0.], F32), (9, 1)))


def test_zero_gradient_takes_the_fallback_with_both_signs():
    s = a.alternating_grid()
    _, p, ax = m.crossing_edges(s, 0.)
    n = a.host_normals(s, 0.)
    assert len(n) == 16 and np.all(ax == 0)
    for row, q in zip(n, p):
        if q[0] == 1:           # inside -> outside, both gradients 0
            assert np.array_equal(row, np.array([1., 0., 0.], F32))
        elif q[0] == 2:         # outside -> inside
            assert np.array_equal(row, np.array([-1., 0., 0.], F32))
        else:                   # a one-sided difference of 2 at the face end: a proper gradient
            assert np.array_equal(np.abs(row), np.array([1., 0., 0.], F32))
    # infinite ends with floor = -inf: every difference is dropped
    s = np.full((3, 3, 3), -np.inf, F32)
    s[1, 1, 1] = np.inf
    _, p, ax = m.crossing_edges(s, 0.)
    n = a.host_normals(s, 0.)
    assert len(n) == 6
    for row, q, e in zip(n, p, ax):
        want = np.zeros(3, F32)
        want[e] = 1. if q[e] == 1 else -1.
        assert np.array_equal(row, want)


def test_nan_and_inf_entries_give_finite_unit_normals():
    n = a.host_normals(a.wild_grid(), 0.5)
    assert len(n) > 3000 and np.all(np.isfinite(n))
    assert np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1) <= 4 * U)


def test_values_near_the_end_of_the_range_do_not_overflow():
    """a power of two commutes with every rounding: the normals of 2^100 sigma (values up to 6e30) at 2^100 iso equal those of
    sigma bit for bit, and those of 2^-100 sigma too; values of 1e30 give finite unit normals"""
    s = m.noise_grid(3, (12, 13, 14))
    n = a.host_normals(s, 0.25)
    assert a.host_normals(s * F32(2.0 ** 100), float(F32(0.25) * F32(2.0 ** 100))).tobytes() == n.tobytes()
    assert a.host_normals(s * F32(2.0 ** -100), float(F32(0.25) * F32(2.0 ** -100))).tobytes() == n.tobytes()
    big = a.host_normals(s * F32(1e30), 1e29)
    assert np.all(np.isfinite(big)) and np.all(np.abs(np.linalg.norm(big.astype(np.float64), axis=-1) - 1) <= 4 * U)


def test_short_capacity_writes_the_first_rows_only():
    s = m.noise_grid(4, (9, 7, 5))
    n = a.host_normals(s, 0.)
    for cap in (len(n) - 1, len(n) // 2, 1, 0):
        assert a.host_normals(s, 0., cap_v=cap).tobytes() == n[:cap].tobytes()


# ----------------------------------------------------------------------------- 5. argument checks
def test_library_checks_the_normals_arguments_without_touching_the_gpu():
    from core import _hip
    lib = _hip.lib()
    assert lib.danbo_abi_version() == 9
    p = ctypes.c_void_p(4096)          # a non-null, aligned placeholder: every call below is rejected before it is looked at
    inf, nan = float("inf"), float("nan")
    good = dict(sigma=p, nx=8, ny=8, nz=8, sx=64, sy=8, floor=0., iso=1., ws=p, normals=p, cap_v=4)
    call = lambda **kw: (lambda g: lib.danbo_mesh_normals(g["sigma"], g["nx"], g["ny"], g["nz"], g["sx"], g["sy"], g["floor"], g["iso"],   # noqa: E731
                                                          g["ws"], g["normals"], g["cap_v"], None))({**good, **kw})
    bad = [dict(sigma=None), dict(ws=None), dict(nx=1), dict(ny=1025), dict(nz=0), dict(sx=-1), dict(sy=-8), dict(iso=nan), dict(iso=inf),
           dict(floor=nan), dict(floor=inf), dict(sigma=ctypes.c_void_p(4098)), dict(nx=2048), dict(nz=-8),
           dict(normals=None), dict(cap_v=-1), dict(normals=None, cap_v=0), dict(normals=ctypes.c_void_p(4098))]
    for kw in bad:
        assert call(**kw) == -22, kw
    with open(os.path.join(ROOT, "include", "danbo_hip.h")) as f:
        header = f.read()
    assert "int danbo_mesh_normals(const float* sigma, int nx, int ny, int nz, long stride_x, long stride_y, float floor, float iso," in header
    assert "compute_normal" in header
    assert len(_hip.SIGNATURES["danbo_mesh_normals"]) == 12


def test_serial_restatement_rejects_what_the_library_rejects():
    lib = a.host_lib()
    g = np.zeros((4, 4, 4), F32)
    ws, out = np.zeros(64, np.int32), np.zeros(12, F32)
    call = lambda *x, normals=out.ctypes.data, cap=4: lib.ref_mesh_normals(g.ctypes.data, *x, ws.ctypes.data, normals, cap)     # noqa: E731
    assert call(4, 4, 4, 16, 4, -np.inf, 0.) == 0
    for bad in ((1, 4, 4, 16, 4, 0., 0.), (4, 1025, 4, 16, 4, 0., 0.), (4, 4, 4, -16, 4, 0., 0.), (4, 4, 4, 16, 4, 0., np.nan),
                (4, 4, 4, 16, 4, 0., np.inf), (4, 4, 4, 16, 4, np.nan, 0.), (4, 4, 4, 16, 4, np.inf, 0.)):
        assert call(*bad) == -22, bad
    assert call(4, 4, 4, 16, 4, 0., 0., normals=None) == -22 and call(4, 4, 4, 16, 4, 0., 0., cap=-1) == -22


# ----------------------------------------------------------------------------- 6. .ply
OLD_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n")
NORMAL_PROPS = "property float nx\nproperty float ny\nproperty float nz\n"
COLOR_PROPS = "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"


@pytest.mark.parametrize("with_n,with_c,vertex_bytes", [(False, False, 12), (True, False, 24), (False, True, 16), (True, True, 28)])
def test_ply_layouts(tmp_path, with_n, with_c, vertex_bytes):
    from core.utils.mesh_io import read_ply, read_ply_attrs, write_ply
    sigma = m.sphere_grid((12, 12, 12), R=4.2, centre=(5.3, 5.6, 5.1))
    verts, faces = m.host_extract(sigma, 0., scale=1. / 11, offset=(-.5, -.5, -.5))
    normals = a.host_normals(sigma, 0.)
    colors = np.random.default_rng(2).integers(0, 256, (len(verts), 3)).astype(np.uint8)
    path = str(tmp_path / "mesh.ply")
    write_ply(path, verts, faces, normals=normals if with_n else None, colors=colors if with_c else None)
    raw = open(path, "rb").read()
    header = (OLD_HEADER % (len(verts), len(faces))).replace(
        "property float z\n", "property float z\n" + (NORMAL_PROPS if with_n else "") + (COLOR_PROPS if with_c else "")).encode()
    assert raw.startswith(header) and len(raw) == len(header) + vertex_bytes * len(verts) + 13 * len(faces)
    # the records, written out by hand
    body = b"".join(verts[i].astype("<f4").tobytes() + (normals[i].astype("<f4").tobytes() if with_n else b"")
                    + (colors[i].tobytes() + b"\xff" if with_c else b"") for i in range(len(verts)))
    body += b"".join(b"\x03" + faces[i].astype("<i4").tobytes() for i in range(len(faces)))
    assert raw == header + body
    v, f, attrs = read_ply_attrs(path)
    assert v.tobytes() == verts.tobytes() and f.tobytes() == faces.tobytes() and v.dtype == np.float32 and f.dtype == np.int32
    assert set(attrs) == ({"normals"} if with_n else set()) | ({"colors"} if with_c else set())
    if with_n:
        assert attrs["normals"].dtype == np.float32 and attrs["normals"].tobytes() == normals.tobytes()
    if with_c:
        assert attrs["colors"].dtype == np.uint8 and attrs["colors"].shape == (len(verts), 3) and np.array_equal(attrs["colors"], colors)
    v2, f2 = read_ply(path)
    assert v2.tobytes() == verts.tobytes() and f2.tobytes() == faces.tobytes()
    open(path, "wb").write(raw[:-5])
    with pytest.raises(ValueError):
        read_ply_attrs(path)
    with pytest.raises(ValueError):
        read_ply(path)


def test_ply_rejects_wrong_lengths_and_foreign_files(tmp_path):
    from core.utils.mesh_io import read_ply, read_ply_attrs, write_ply
    verts, faces = m.host_extract(m.sphere_grid((12, 12, 12), R=4.2, centre=(5.3, 5.6, 5.1)), 0.)
    path = str(tmp_path / "mesh.ply")
    with pytest.raises(ValueError):
        write_ply(path, verts, faces, normals=np.zeros((len(verts) - 1, 3), F32))
    with pytest.raises(ValueError):
        write_ply(path, verts, faces, colors=np.zeros((len(verts) + 1, 3), np.uint8))
    with pytest.raises(ValueError):
        write_ply(path, verts, faces, colors=np.zeros((len(verts), 4), np.uint8))
    foreign = (OLD_HEADER % (1, 0)).replace("property float z\n", "property float z\nproperty float quality\n").encode() + bytes(16)
    open(path, "wb").write(foreign)
    for reader in (read_ply, read_ply_attrs):
        with pytest.raises(ValueError):
            reader(path)
    open(path, "wb").write(b"not a ply file")
    with pytest.raises(ValueError):
        read_ply_attrs(path)
    # an empty mesh with attributes
    write_ply(path, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), F32), colors=np.zeros((0, 3), np.uint8))
    v, f, attrs = read_ply_attrs(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and attrs["normals"].shape == (0, 3) and attrs["colors"].shape == (0, 3)


# ----------------------------------------------------------------------------- 7. parser, wrappers
def test_entry_points_know_the_two_flags():
    import inspect
    import run_render
    from core import hip_ops
    from core.anerf_engine import AnerfEngine
    from core.raycasters import RayCaster
    from core.render_engine import DanboEngine
    base = ["--nerf_args", "x", "--ckptpath", "y", "--dataset", "synthetic", "--entry", "val", "--runname", "r", "--render_mesh"]
    args = run_render.config_parser().parse_args(base)
    assert args.mesh_normals is False and args.mesh_colors is False
    args = run_render.config_parser().parse_args(base + ["--mesh_normals", "--mesh_colors"])
    assert args.mesh_normals is True and args.mesh_colors is True
    assert "mesh_normals" in run_render.render_mesh.__doc__ and "mesh_colors" in run_render.render_mesh.__doc__
    assert inspect.signature(hip_ops.marching_cubes).parameters["normals"].default is False
    sig = inspect.signature(RayCaster.render_mesh_surface).parameters
    assert sig["normals"].default is False and sig["colors"].default is False and sig["cams"].default is None
    for eng in (DanboEngine, AnerfEngine):
        assert list(inspect.signature(eng.colors).parameters)[1:5] == ["pts", "dirs", "skts", "bones"]
