"""The serial rasteriser of csrc/raster_math.hpp (the statement the GPU kernels are compared with bit for bit in
tests/test_gpu_raster.py) against numpy: the vertex stage against float64, the covered set against exact integer arithmetic, depth,
colour and the winning triangle against float64 -- plus the argument checks of the library and the host layers, none of which
needs a GPU."""
import ctypes
import math

import numpy as np
import pytest

import mesh_ref
import raster_ref as rr

F32 = np.float32
SIZES = ((64, 64), (80, 96))


def covered(out):
    return out["tri_id"][0] >= 0


def check_coverage(verts, faces, view, hx, H, W, mode=rr.FLAT, attr=None):
    """the serial code's covered set and id map against the integer prediction from the library's own X, Y -> (out, prediction)"""
    X, Y, z, valid, _ = rr.host_vertices(verts, attr, mode, view, hx, H, W)
    out = rr.host_raster(verts, faces, attr, mode, [view], hx, H, W)
    pred = rr.predict(X, Y, valid, faces, H, W, z=z.astype(np.float64))
    assert np.array_equal(covered(out), pred["count"] > 0), "covered set differs from the integer prediction"
    return out, pred


# ----------------------------------------------------------------------------- 1. vertex stage
def test_vertex_stage_against_float64():
    rng = np.random.default_rng(5)
    verts = rng.uniform(-1, 1, (4000, 3)).astype(F32)
    normals = rng.standard_normal((4000, 3)).astype(F32)
    normals[:7] = 0.
    colors = rng.random((4000, 3)).astype(F32)
    worst = dict(x=0., y=0., z=0., col=0.)
    for H, W in SIZES + ((4096, 4096), (1, 1), (5, 7)):
        for view in (rr.view_matrix(0.3, 0.7, -0.2, 0.55, (0.1, -0.2, 0.05), (0.03, -0.02, 0.1)),
                     rr.view_matrix(-2.1, 1.9, 3.0, 0.41, (0., 0., 0.), (-0.15, 0.1, -0.3)), rr.view_matrix()):
            X, Y, z, valid, col = rr.host_vertices(verts, normals, rr.NORMAL, view, 0.6, H, W)
            x64, y64, p = rr.vertex_stage_f64(verts, view, 0.6, H, W)
            assert valid.all() and np.abs(x64).max() < 2 ** 12 * 256 * 1.5
            worst["x"] = max(worst["x"], np.abs(X - np.rint(x64)).max())
            worst["y"] = max(worst["y"], np.abs(Y - np.rint(y64)).max())
            worst["z"] = max(worst["z"], np.abs(z - p[:, 2]).max())
            worst["col"] = max(worst["col"], np.abs(col - rr.normal_colors_f64(normals, view)).max())
            _, _, _, _, c2 = rr.host_vertices(verts, colors, rr.COLOR, view, 0.6, H, W)
            assert np.array_equal(c2, colors)
            _, _, _, _, c3 = rr.host_vertices(verts, None, rr.FLAT, view, 0.6, H, W)
            worst["z"] = max(worst["z"], np.abs(c3 - p).max())
    print("vertex stage: max |X - X64|, |Y - Y64| (1/256 pixel), |z - z64|, |colour - colour64|:", worst)
    assert worst["x"] <= 1 and worst["y"] <= 1 and worst["z"] <= rr.TOL and worst["col"] <= rr.TOL
    assert np.all(rr.host_vertices(verts[:7], normals[:7], rr.NORMAL, rr.view_matrix(), 0.6, 8, 8)[4] == 0.5)      # no length: 0


def test_invalid_vertices_and_the_snap():
    inf, nan = np.inf, np.nan
    verts = np.array([[0, 0, 0], [nan, 0, 0], [0, inf, 0], [0, 0, -inf], [300, 0, 0], [0, -300, 0], [200, 0, 0]], F32)
    X, Y, z, valid, _ = rr.host_vertices(verts, None, rr.FLAT, rr.view_matrix(), 0.5, 4096, 4096)
    # x_pix = (x + 0.5) * 4096, the limit 2^28 / 256 = 2^20 pixels: x = 300 lies 1.17 * 2^20 pixels out (invalid), 200 lies 0.78 (valid)
    assert valid.tolist() == [True, False, False, False, False, False, True]
    assert (X[0], Y[0]) == (2048 * 256, 2048 * 256)
    # ties of the snap go to the even neighbour: x_pix = k / 512 + 1 / 1024 -> 256 x_pix = k / 2 + 1 / 4; k / 2 exact halves
    px = np.array([0.5 / 256, 1.5 / 256, 2.5 / 256, 3.25 / 256])
    v, view, hx = rr.pixel_scene(px + 32, px + 32, np.zeros(4), 64, 64)
    X, Y, *_ = rr.host_vertices(v, None, rr.FLAT, view, hx, 64, 64)
    assert (X - 32 * 256).tolist() == [0, 2, 2, 3] and (Y - 32 * 256).tolist() == [0, 2, 2, 3]


# ----------------------------------------------------------------------------- 2. coverage
def test_single_triangle_in_both_windings():
    px, py = [3.3, 40.7, 17.2], [5.1, 22.9, 55.6]
    v, view, hx = rr.pixel_scene(px, py, [0.1, 0.5, -0.3], 64, 64)
    a, pa = check_coverage(v, [[0, 1, 2]], view, hx, 64, 64)
    b, pb = check_coverage(v, [[0, 2, 1]], view, hx, 64, 64)
    assert covered(a).sum() > 300 and np.array_equal(covered(a), covered(b))
    assert set(np.unique(pa["signed"])) | set(np.unique(pb["signed"])) == {-1, 0, 1} and np.array_equal(pa["signed"], -pb["signed"])
    # both windings carry the same depth within the tolerance, and FLAT colours with opposite normals
    m = covered(a)
    assert np.abs(a["depth"][0][m] - pa["depth"][m]).max() <= rr.TOL and np.abs(b["depth"][0][m] - pa["depth"][m]).max() <= rr.TOL
    assert np.abs((a["rgb"][0][m] - 0.5) + (b["rgb"][0][m] - 0.5)).max() <= rr.TOL
    assert np.all(a["rgb"][0][~m] == 1.) and np.all(np.isneginf(a["depth"][0][~m])) and np.all(a["tri_id"][0][~m] == -1)


@pytest.mark.parametrize("diagonal", (0, 1))
def test_quad_on_pixel_centres_and_corners(diagonal):
    """corners of the quad on pixel corners (integers) and on pixel centres (+ 0.5).  An oriented triangle (area2 > 0) runs
    clockwise on the screen (y down); the rule gives a centre on an edge to the triangle whose edge runs downwards (dy > 0) or
    leftwards (dy == 0, dx < 0) there: the right and the bottom edge of the quad are in, the left and the top edge are out.
    Every such pixel centre is covered exactly once, and the id map is the prediction exactly"""
    for x0, y0, x1, y1 in ((8, 8, 24, 20), (8.5, 8.5, 24.5, 20.5), (8, 8.5, 24.5, 20)):
        v, view, hx = rr.pixel_scene([x0, x1, x1, x0], [y0, y0, y1, y1], [0., 0.2, 0.1, 0.3], 64, 64)
        X, Y, *_ = rr.host_vertices(v, None, rr.FLAT, view, hx, 64, 64)
        assert X.tolist() == [int(256 * x) for x in (x0, x1, x1, x0)] and Y.tolist() == [int(256 * y) for y in (y0, y0, y1, y1)]
        faces = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
        out, pred = check_coverage(v, faces, view, hx, 64, 64)
        assert pred["count"].max() == 1, "a pixel on the shared diagonal is hit twice"
        cx, cy = np.arange(64) + 0.5, np.arange(64) + 0.5
        want = ((cy > y0) & (cy <= y1))[:, None] & ((cx > x0) & (cx <= x1))[None, :]
        assert np.array_equal(covered(out), want)
        assert np.array_equal(out["tri_id"][0], pred["tri"])


def test_fan_sliver_offscreen_and_degenerate():
    H, W = 64, 64
    # a fan around a vertex on a pixel centre: the centre pixel belongs to exactly one triangle
    k = 7
    ang = 2 * np.pi * np.arange(k) / k + 0.1
    v, view, hx = rr.pixel_scene(np.r_[20.5, 20.5 + 9.3 * np.cos(ang)], np.r_[30.5, 30.5 + 9.3 * np.sin(ang)], np.zeros(k + 1), H, W)
    faces = [[0, 1 + i, 1 + (i + 1) % k] for i in range(k)]
    out, pred = check_coverage(v, faces, view, hx, H, W)
    assert pred["count"][30, 20] == 1 and pred["count"].max() == 1 and covered(out).sum() > 150
    assert np.array_equal(out["tri_id"][0], pred["tri"])
    # a sliver thinner than a pixel: a few centres or none, exactly the predicted ones
    v, view, hx = rr.pixel_scene([2.1, 60.3, 60.3], [10.2, 31.4, 31.7], [0., 0., 0.], H, W)
    out, pred = check_coverage(v, [[0, 1, 2]], view, hx, H, W)
    print("sliver: covered", int(covered(out).sum()))
    assert 0 < covered(out).sum() < 20
    # partly and wholly off-screen
    v, view, hx = rr.pixel_scene([-30.2, 40.1, 10.3, 70., 90., 80., -500., 900., 30.], [-20.4, 10.7, 90.2, 10., 10., 30., -300., -300., 700.],
                                 [0., 0., 0., 0., 0., 0., -1., -1., -1.], H, W)
    out, pred = check_coverage(v, [[0, 1, 2]], view, hx, H, W)
    assert 0 < covered(out).sum() < H * W
    out, pred = check_coverage(v, [[3, 4, 5]], view, hx, H, W)
    assert covered(out).sum() == 0
    out, pred = check_coverage(v, [[6, 7, 8], [0, 1, 2]], view, hx, H, W)           # a screen-filling one behind
    assert covered(out).all() and np.array_equal(out["tri_id"][0], pred["tri"]) and set(np.unique(pred["tri"])) == {0, 1}
    # zero area, a NaN vertex, an index out of range: nothing
    v, view, hx = rr.pixel_scene([5., 25., 45., 5., 50.], [5., 25., 45., 50., 5.], [0., 0., 0., 0., np.nan], H, W)
    for faces in ([[0, 1, 2]], [[0, 0, 3]], [[0, 3, 4]], [[0, 3, 5]], [[-1, 3, 1]], [[0, 3, 2 ** 31 - 1]]):
        out = rr.host_raster(v, faces, None, rr.FLAT, [view], hx, H, W)
        assert not covered(out).any() and np.all(out["rgb"] == 1.), faces
    out, _ = check_coverage(v, [[0, 3, 4], [0, 1, 3], [0, 3, 7]], view, hx, H, W)     # a good one between two bad ones
    assert set(np.unique(out["tri_id"])) == {-1, 1}


# ----------------------------------------------------------------------------- 3. closed meshes
@pytest.mark.parametrize("name,n_tris", (("sphere", 3176), ("torus", 2748), ("two_spheres", 1632)))
def test_closed_meshes_against_float64(name, n_tris):
    verts, faces, normals, colors = rr.closed_mesh(name)
    assert len(faces) == n_tris and mesh_ref.is_closed_oriented_manifold(faces)
    for (H, W), view in zip(SIZES, rr.MESH_VIEWS):
        X, Y, z, valid, col = rr.host_vertices(verts, normals, rr.NORMAL, view, rr.MESH_HX, H, W)
        x64, y64, p = rr.vertex_stage_f64(verts, view, rr.MESH_HX, H, W)
        assert valid.all() and np.abs(p).max() <= 1.
        p32 = rr.host_vertices(verts, None, rr.FLAT, view, rr.MESH_HX, H, W)[4]        # the fp32 view-space corners (test 1: within TOL of p)
        flat, flat_tol = rr.flat_colors_f64(p32.astype(np.float64), faces), rr.flat_tolerance(p32, faces)
        for mode, attr, kw in ((rr.NORMAL, normals, dict(col=rr.normal_colors_f64(normals, view))),
                               (rr.COLOR, colors, dict(col=colors.astype(np.float64))), (rr.FLAT, None, dict(tri_col=flat))):
            out = rr.host_raster(verts, faces, attr, mode, [view], rr.MESH_HX, H, W)
            pred = rr.predict(X, Y, valid, faces, H, W, z=p[:, 2], **kw)
            m = pred["count"] > 0
            assert np.array_equal(covered(out), m) and m.sum() > 0.1 * H * W
            assert not pred["signed"].any(), "a closed mesh: front and back hits cancel at every pixel (no crack, no double hit)"
            with np.errstate(invalid="ignore"):        # (background: -inf - -inf)
                clear = m & (pred["depth"] - pred["second"] >= 1e-4)
            excluded = (m.sum() - clear.sum()) / m.sum()
            e_d = np.abs(out["depth"][0][clear] - pred["depth"][clear]).max()
            e_c = np.abs(out["rgb"][0][clear] - pred["rgb"][clear]).max()
            print(f"{name} {H}x{W} mode {mode}: covered {int(m.sum())}, near-ties excluded {100 * excluded:.3f} %, "
                  f"|depth - f64| {e_d:.2e}, |rgb - f64| {e_c:.2e} (bound {rr.TOL:.2e})")
            assert excluded <= 0.005
            assert np.array_equal(out["tri_id"][0][clear], pred["tri"][clear])
            assert e_d <= rr.TOL
            if mode == rr.FLAT:         # the face normal of a small triangle is as good as its corners allow: rr.flat_tolerance
                worst = (np.abs(out["rgb"][0][clear] - pred["rgb"][clear]).max(-1) / flat_tol[pred["tri"][clear]]).max()
                print(f"    FLAT: |rgb - f64 face normal colour| / the triangle's bound: max {worst:.3f}")
                assert worst <= 1.
            else:
                assert e_c <= rr.TOL
            assert np.all(out["rgb"][0][~m] == 1.)


@pytest.mark.parametrize("name", ("sphere", "torus", "two_spheres"))
def test_closed_meshes_coarsened_onto_half_pixels(name):
    """vertices moved onto pixel centres and corners (multiples of half a pixel): edges and vertices fall on pixel centres all over
    the image, the covered set still equals the prediction and the signed coverage still cancels"""
    verts, faces, _, _ = rr.closed_mesh(name)
    for (H, W), view in zip(SIZES + ((40, 56),), rr.MESH_VIEWS):
        x64, y64, p = rr.vertex_stage_f64(verts, view, rr.MESH_HX, H, W)
        v, ident, hx = rr.pixel_scene(np.rint(x64 / 128) / 2, np.rint(y64 / 128) / 2, p[:, 2], H, W)
        X, Y, z, valid, _ = rr.host_vertices(v, None, rr.FLAT, ident, hx, H, W)
        assert np.all(X % 128 == 0) and np.all(Y % 128 == 0)         # (W = 96, 56: x_pix is within an ulp of k / 2, the snap lands on it)
        out = rr.host_raster(v, faces, None, rr.FLAT, [ident], hx, H, W, want=("tri_id",))
        pred = rr.predict(X, Y, valid, faces, H, W)
        assert np.array_equal(out["tri_id"][0] >= 0, pred["count"] > 0) and not pred["signed"].any()
        assert (pred["count"] > 0).sum() > 0.1 * H * W


# ----------------------------------------------------------------------------- 4. visibility, modes, guards
def test_equal_depth_goes_to_the_lower_index_and_the_key_orders_depths():
    verts, faces, normals, _ = rr.closed_mesh("two_spheres")
    H, W = 64, 64
    view = rr.MESH_VIEWS[0]
    once = rr.host_raster(verts, faces, normals, rr.NORMAL, [view], rr.MESH_HX, H, W)
    twice = rr.host_raster(verts, np.concatenate([faces, faces]), normals, rr.NORMAL, [view], rr.MESH_HX, H, W)
    assert all(np.array_equal(once[k], twice[k]) for k in once)
    swapped = rr.host_raster(verts, np.concatenate([faces[::-1], faces]), normals, rr.NORMAL, [view], rr.MESH_HX, H, W)
    m = covered(once)
    assert np.array_equal(swapped["tri_id"][0][m], len(faces) - 1 - once["tri_id"][0][m])
    assert np.array_equal(swapped["depth"], once["depth"]) and np.array_equal(swapped["rgb"], once["rgb"])
    key = rr.host_lib().ref_raster_key
    ds = [-np.inf, -3e38, -1., -1e-45, -0., 1e-45, 0.5, 1., 3e38, np.inf]
    keys = [key(d, 5) for d in ds]
    assert keys[4] == key(0., 5) and sorted(keys) == keys and len(set(keys)) == len(ds) and min(keys) > 0
    assert key(0.25, 3) > key(0.25, 4) > key(0.2499, 0) and key(np.nan, 1) == 0
    assert key(1., 7) & 0xFFFFFFFF == 0xFFFFFFFF - 7


def test_empty_inputs_views_and_untouched_outputs():
    verts, faces, normals, colors = rr.closed_mesh("sphere")
    H, W = 5, 7
    bg = (0.25, 0.5, 0.75)
    for v, f, a in ((verts, faces[:0], normals), (verts[:0], faces[:0], normals[:0]), (verts[:0], faces, normals[:0])):
        out = rr.host_raster(v, f, a, rr.NORMAL, rr.MESH_VIEWS[:2], rr.MESH_HX, H, W, background=bg)
        assert np.all(out["rgb"] == np.array(bg, F32)) and np.all(np.isneginf(out["depth"])) and np.all(out["tri_id"] == -1)
    # three views in one call = three calls
    out3 = rr.host_raster(verts, faces, colors, rr.COLOR, rr.MESH_VIEWS, rr.MESH_HX, 40, 56)
    for i, view in enumerate(rr.MESH_VIEWS):
        one = rr.host_raster(verts, faces, colors, rr.COLOR, [view], rr.MESH_HX, 40, 56)
        assert all(np.array_equal(out3[k][i], one[k][0]) for k in one)
    assert not np.array_equal(out3["tri_id"][0], out3["tri_id"][1])
    for want in (("rgb",), ("depth",), ("tri_id",), ("depth", "tri_id")):
        part = rr.host_raster(verts, faces, colors, rr.COLOR, rr.MESH_VIEWS, rr.MESH_HX, 40, 56, want=want)
        assert set(part) == set(want) and all(np.array_equal(part[k], out3[k]) for k in want)
    # 1 x 1: the one pixel centre
    one = rr.host_raster(verts, faces, colors, rr.COLOR, rr.MESH_VIEWS[:1], rr.MESH_HX, 1, 1)
    assert one["tri_id"].shape == (1, 1, 1) and one["tri_id"][0, 0, 0] >= 0


def _raster_call(lib_fn, **kw):
    p = ctypes.c_void_p(4096)          # a non-null, aligned placeholder: every call below is rejected before it is looked at
    a = dict(verts=p, V=8, tris=p, T=4, attr=p, mode=1, views=p, n_views=1, hx=0.6, H=16, W=16, bg=p, ws=p, rgb=p, depth=p, tri_id=p)
    a.update(kw)
    return lib_fn(a["verts"], a["V"], a["tris"], a["T"], a["attr"], a["mode"], a["views"], a["n_views"], a["hx"], a["H"], a["W"], a["bg"],
                  a["ws"], a["rgb"], a["depth"], a["tri_id"], *kw.get("tail", ()))


BAD_ARGUMENTS = [dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(V=-1), dict(T=-1), dict(n_views=0), dict(mode=3), dict(mode=-1),
                 dict(attr=None), dict(attr=None, mode=0), dict(hx=0.), dict(hx=-1.), dict(hx=float("nan")), dict(hx=float("inf")),
                 dict(verts=None), dict(tris=None), dict(views=None), dict(bg=None), dict(ws=None), dict(rgb=None, depth=None, tri_id=None),
                 dict(verts=ctypes.c_void_p(4098)), dict(tris=ctypes.c_void_p(4097)), dict(ws=ctypes.c_void_p(4100)),
                 dict(rgb=ctypes.c_void_p(4098)), dict(depth=ctypes.c_void_p(4099)), dict(tri_id=ctypes.c_void_p(4098)),
                 dict(views=ctypes.c_void_p(4098)), dict(bg=ctypes.c_void_p(4098)), dict(attr=ctypes.c_void_p(4098))]


def test_serial_code_rejects_what_the_library_rejects():
    fn = rr.host_lib().ref_raster_mesh
    for kw in BAD_ARGUMENTS:
        assert _raster_call(fn, **kw) == -22, kw
    assert rr.host_lib().ref_raster_workspace_bytes(10, 0, 4) == 0


def test_library_checks_raster_arguments_without_touching_the_gpu():
    from core import _hip
    lib = _hip.lib()
    assert lib.danbo_abi_version() == 9
    al = lambda n: (n + 255) // 256 * 256      # noqa: E731
    assert lib.danbo_raster_workspace_bytes(1000, 80, 96) == 256 + al(8 * 80 * 96) + al(16 * 1000) + al(12 * 1000)
    assert lib.danbo_raster_workspace_bytes(0, 1, 1) == 256 + 256
    assert lib.danbo_raster_workspace_bytes(3, 4096, 4096) == 256 + 8 * 4096 * 4096 + 512
    for dims in ((-1, 8, 8), (8, 0, 8), (8, 8, 0), (8, 4097, 8), (8, 8, 4097)):
        assert lib.danbo_raster_workspace_bytes(*dims) == 0
    assert lib.danbo_raster_workspace_bytes(1000, 80, 96) == rr.host_lib().ref_raster_workspace_bytes(1000, 80, 96)
    for kw in BAD_ARGUMENTS:
        assert _raster_call(lib.danbo_raster_mesh, tail=(None,), **kw) == -22, kw


def test_header_binding_and_wrappers_know_the_rasteriser():
    import torch
    from core import _hip, hip_ops
    # The two entries stand in include/danbo_raster.h; tests/test_abi_binding.py referees how they are bound.
    with open(_hip.header("danbo_raster.h").path) as f:
        text = f.read()
    assert "size_t danbo_raster_workspace_bytes(int n_verts, int height, int width);" in text
    assert "int danbo_raster_mesh(const float* verts, int n_verts, const int* tris, int n_tris," in text
    assert "render_mesh.py" in text and "render/camera.py:186-188" in text and _hip.C.DANBO_ABI_VERSION == 9
    assert hip_ops.RASTER_MODES == rr.MODES
    v, f, views = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.rasterize_mesh(v, f, mode="flat", views=views)
    from core.utils import mesh_render
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_render.turntable_views(v)
    import render_mesh
    a = render_mesh.config_parser().parse_args(["--basedir", "b", "--expname", "e", "-ww", "48", "-hh", "40", "--mesh_ind", "2", "--skip", "3",
                                                "--flip"])
    assert (a.width, a.height, a.mesh_ind, a.skip, a.flip, a.shade) == (48, 40, 2, 3, True, "normal")
    assert render_mesh.pick_shade("normal", {}, "x.ply") == "flat" and render_mesh.pick_shade("normal", {"normals": 0}, "x") == "normal"
    with pytest.raises(ValueError, match="no vertex colours"):
        render_mesh.pick_shade("color", {"normals": 0}, "x.ply")
    import run_render
    base = ["--nerf_args", "x", "--ckptpath", "y", "--dataset", "synthetic", "--entry", "val", "--runname", "r", "--render_mesh"]
    a = run_render.config_parser().parse_args(base)
    assert a.mesh_render is None and a.mesh_render_res == [512, 512]
    a = run_render.config_parser().parse_args(base + ["--mesh_render"])
    assert a.mesh_render == "normal"
    a = run_render.config_parser().parse_args(base + ["--mesh_render", "flat", "--mesh_render_res", "40", "56"])
    assert a.mesh_render == "flat" and a.mesh_render_res == [40, 56]


# ----------------------------------------------------------------------------- 5. the turntable's views
def turntable_f64(verts, n_frames, step_deg):
    """the reference's turntable restated from its description: rot, make_rotate(270, 180, 90 degrees), the uniform scale
    1 / (y_max - y_min) of the rotated vertices (not centred), then a turn about y by -(90 + step (j + 1)) degrees for frame j"""
    def rot_xyz(rx, ry, rz):
        sx, sy, sz, cx, cy, cz = math.sin(rx), math.sin(ry), math.sin(rz), math.cos(rx), math.cos(ry), math.cos(rz)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
        return Rz @ Ry @ Rx
    v = verts.astype(np.float64) @ np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float64).T
    R = rot_xyz(math.radians(270), math.radians(180), math.radians(90))
    v = v @ R.T
    s = 1. / (v[:, 1].max() - v[:, 1].min())
    out = []
    for j in range(n_frames):
        turn = rot_xyz(0, math.radians(-(90 + step_deg * (j + 1))), 0)
        out.append((v * s) @ turn.T)
    return np.stack(out)


def test_turntable_views_against_the_float64_restatement():
    """turntable_views needs a device tensor for its one reduction; its closed form (mesh_render.base_rotation / make_rotate)
    is checked here, the device part in tests/test_gpu_raster.py"""
    from core.utils import mesh_render as mr
    rng = np.random.default_rng(2)
    verts = (rng.standard_normal((500, 3)) * [0.3, 0.2, 0.5] + [0.1, 0., -0.2]).astype(F32)
    want = turntable_f64(verts, 91, 4.)
    B = mr.base_rotation()
    y = verts.astype(np.float64) @ B[1]
    got = np.stack([verts.astype(np.float64) @ (mr.make_rotate(0., math.radians(-(90. + 4. * (j + 1))), 0.) @ B / (y.max() - y.min())).T
                    for j in range(91)])
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(want[0] - want[90]).max() < 1e-12, "frame 0 and frame 90 differ by 360 degrees"
    assert np.abs(want[0] - want[45]).max() > 0.1
    assert abs((want[0][:, 1].max() - want[0][:, 1].min()) - 1.) < 1e-12 and mr.HALF_EXTENT == 0.6 and mr.N_FRAMES == 91
