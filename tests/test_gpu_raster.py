"""The rasteriser kernels (csrc/k_raster.hip through hip_ops.rasterize_mesh and the C entry danbo_raster_mesh) against the serial
restatement of csrc/raster_math.hpp -- tests/raster_ref.py, itself checked against numpy in tests/test_raster_host.py -- bit for
bit: rgb, depth and tri_id.  Then the turntable (core/utils/mesh_render.py) and the entry points on the synthetic model."""
import ctypes
import os

import numpy as np
import pytest
import torch

import raster_ref as rr
from helpers import ROOT, golden, T, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
GUARD = rr.GUARD
SIZES = ((1, 1), (5, 7), (64, 64), (80, 96))          # 80 x 96: W no multiple of 64, more than one wavefront per row


def gpu_raster(verts, faces, attr, mode, views, hx, H, W, background=(1., 1., 1.), want=("rgb", "depth", "tri_id")):
    from core import hip_ops
    name = {v: k for k, v in rr.MODES.items()}[mode]
    out = hip_ops.rasterize_mesh(T(np.reshape(verts, (-1, 3))), T(np.reshape(faces, (-1, 3)), torch.int32), None if attr is None else T(attr),
                                 mode=name, views=T(np.reshape(views, (-1, 12))), half_extent=hx, size=(H, W), background=background,
                                 want=want)
    assert set(out) == set(want) and all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def check_scene(verts, faces, attr, mode, views, hx, H, W, **kw):
    """kernels = serial code, bit for bit, on every output -> the serial result"""
    ref = rr.host_raster(verts, faces, attr, mode, views, hx, H, W, **kw)
    got = gpu_raster(verts, faces, attr, mode, views, hx, H, W, **kw)
    for k in ref:
        if not same_bits(got[k], ref[k]):
            bad = np.argwhere(got[k] != ref[k])
            raise AssertionError(f"{k} differs from the serial rasteriser at {len(bad)} places, first {bad[:4].tolist()}")
    return ref


def box_count(verts, face, view, hx, H, W):
    """pixel centres in the clipped bounding box of one triangle, from the library's own snapped vertices"""
    X, Y, *_ = rr.host_vertices(verts, None, rr.FLAT, view, hx, H, W)
    xs, ys = X[list(face)].astype(np.int64), Y[list(face)].astype(np.int64)
    nx = min((xs.max() - 128) // 256, W - 1) - max(-((128 - xs.min()) // 256), 0) + 1
    ny = min((ys.max() - 128) // 256, H - 1) - max(-((128 - ys.min()) // 256), 0) + 1
    return int(max(nx, 0) * max(ny, 0))


# ----------------------------------------------------------------------------- 1. kernels = serial rasteriser, bit for bit
@pytest.mark.parametrize("name", ("sphere", "torus", "two_spheres"))
def test_closed_meshes_equal_the_serial_rasteriser_bitwise(name):
    verts, faces, normals, colors = rr.closed_mesh(name)
    for H, W in SIZES:
        for mode, attr in ((rr.NORMAL, normals), (rr.COLOR, colors), (rr.FLAT, None)):
            n_views = 3 if (H, W) in ((5, 7), (80, 96)) else 1
            ref = check_scene(verts, faces, attr, mode, rr.MESH_VIEWS[:n_views], rr.MESH_HX, H, W)
            if H * W > 1000:
                assert (ref["tri_id"] >= 0).mean() > 0.1


def mixed_scene(H, W):
    """two screen-filling triangles (one of them behind, one cutting through), triangles of a few hundred pixels and 600 sub-pixel
    ones in front of and behind them"""
    rng = np.random.default_rng(9)
    big_x = [-3. * W, 4. * W, 0.5 * W, -2. * W, 3. * W, 0.3 * W, 10.3, 50.7, 22.1, 60.2, 20.4, 44.9]
    big_y = [-2. * H, -2.5 * H, 5. * H, 4. * H, 3.5 * H, -4. * H, 8.2, 19.4, 57.3, 50.1, 40.8, 9.9]
    big_z = [-0.5, -0.5, -0.5, 0.9, -0.9, -0.2, 0.3, 0.1, -0.7, 0.8, 0.8, -0.6]
    n = 600
    cx, cy = rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n)
    sx = np.repeat(cx, 3) + rng.uniform(-0.9, 0.9, 3 * n)
    sy = np.repeat(cy, 3) + rng.uniform(-0.9, 0.9, 3 * n)
    sz = np.repeat(rng.uniform(-1, 1, n), 3) + rng.uniform(-0.01, 0.01, 3 * n)
    verts, view, hx = rr.pixel_scene(np.r_[big_x, sx], np.r_[big_y, sy], np.r_[big_z, sz], H, W)
    faces = np.r_[np.arange(12).reshape(4, 3), 12 + np.arange(3 * n).reshape(n, 3)]
    order = rng.permutation(len(faces))          # the large ones scattered over the wavefronts
    return verts, faces[order].astype(np.int32), view, hx


def test_screen_filling_and_sub_pixel_triangles_together():
    H, W = 80, 96
    verts, faces, view, hx = mixed_scene(H, W)
    boxes = np.array([box_count(verts, f, view, hx, H, W) for f in faces])
    print("mixed scene: boxes of H * W:", int((boxes == H * W).sum()), "of 65 .. H * W - 1:", int(((boxes > 64) & (boxes < H * W)).sum()),
          "of 1 .. 64:", int(((boxes > 0) & (boxes <= 64)).sum()), "empty:", int((boxes == 0).sum()))
    assert (boxes == H * W).sum() == 2 and ((boxes > 64) & (boxes < H * W)).sum() == 2 and ((boxes > 0) & (boxes <= 4)).sum() > 300
    colors = np.random.default_rng(1).random((len(verts), 3)).astype(F32)
    for mode, attr in ((rr.COLOR, colors), (rr.FLAT, None)):
        ref = check_scene(verts, faces, attr, mode, [view], hx, H, W)
    assert (ref["tri_id"] >= 0).all() and len(np.unique(ref["tri_id"])) > 50        # (the scene: many small ones in front)


def test_boxes_of_64_and_65_pixel_centres_take_both_walks():
    """RASTER_LANE_BOX = 64: a box of exactly 64 centres is walked by its own lane, one of 65 by the wavefront -- unclipped and
    clipped at the image border, alone and side by side in one wavefront"""
    H, W = 64, 64
    tris = {"8x8": ([10.2, 17.9, 10.3], [10.2, 10.3, 17.9]), "5x13": ([30.2, 34.9, 30.3], [20.2, 20.3, 32.9]),
            "clipped 8x8": ([-20.3, 7.9, -5.2], [40.2, 40.4, 47.9]), "clipped 13x5": ([51.2, 90.7, 60.3], [59.1, 61.2, 80.4]),
            "4x16": ([40.1, 43.9, 40.6], [2.2, 2.4, 17.9]), "1x65 clipped to 1x64": ([20.2, 20.9, 20.4], [-0.8, 0.3, 64.4])}
    want = {"8x8": 64, "5x13": 65, "clipped 8x8": 64, "clipped 13x5": 65, "4x16": 64, "1x65 clipped to 1x64": 64}
    px = np.concatenate([t[0] for t in tris.values()])
    py = np.concatenate([t[1] for t in tris.values()])
    verts, view, hx = rr.pixel_scene(px, py, np.linspace(-0.5, 0.5, len(px)), H, W)
    faces = np.arange(len(px), dtype=np.int32).reshape(-1, 3)
    for i, name in enumerate(tris):
        assert box_count(verts, faces[i], view, hx, H, W) == want[name], name
        ref = check_scene(verts, faces[i:i + 1], None, rr.FLAT, [view], hx, H, W)
        assert (ref["tri_id"] >= 0).sum() > 20
    colors = np.random.default_rng(3).random((len(verts), 3)).astype(F32)
    check_scene(verts, faces, colors, rr.COLOR, [view], hx, H, W)
    check_scene(verts, faces[:, [0, 2, 1]], colors, rr.COLOR, [view], hx, H, W)          # the other winding


def test_offscreen_degenerate_invalid_and_empty_inputs():
    H, W = 64, 64
    verts, view, hx = rr.pixel_scene([-30.2, 40.1, 10.3, 70., 90., 80., 5., 25., 45., 5., 50., 3e6],
                                     [-20.4, 10.7, 90.2, 10., 10., 30., 5., 25., 45., 50., 5., 7.],
                                     [0., 0., 0., 0., 0., 0., 0.5, 0.5, 0.5, 0.5, np.nan, 0.5], H, W)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 6, 9], [6, 9, 10], [6, 9, 12], [-1, 9, 7], [6, 9, 2 ** 31 - 1], [6, 9, 11],
                      [6, 7, 9]], np.int32)
    ref = check_scene(verts, faces, None, rr.FLAT, [view], hx, H, W)
    assert set(np.unique(ref["tri_id"])) == {-1, 0, 9}
    normals = np.tile(np.array([[0., 0., 1.]], F32), (len(verts), 1))
    bg = (0.25, 0.5, 0.75)
    for v, f, a in ((verts, faces[:0], normals), (verts[:0], faces[:0], normals[:0]), (verts[:0], faces, normals[:0])):
        ref = check_scene(v, f, a, rr.NORMAL, rr.MESH_VIEWS[:2], hx, 5, 7, background=bg)
        assert np.all(ref["rgb"] == np.array(bg, F32)) and np.all(ref["tri_id"] == -1)
    check_scene(verts[:0], faces[:0], None, rr.FLAT, [view], hx, 64, 64)
    from core import _hip, hip_ops
    with pytest.raises(ValueError):
        hip_ops.rasterize_mesh(T(verts), T(faces, torch.int32), None, mode="normal", views=T(view).reshape(1, 12))
    with pytest.raises(ValueError):
        hip_ops.rasterize_mesh(T(verts), T(faces, torch.int64), None, mode="flat", views=T(view).reshape(1, 12))
    with pytest.raises(ValueError):
        hip_ops.rasterize_mesh(T(verts), T(faces, torch.int32), None, mode="flat", views=T(view).reshape(1, 12), want=())
    with pytest.raises(_hip.HipError):
        hip_ops.rasterize_mesh(T(verts), T(faces, torch.int32), None, mode="flat", views=T(view).reshape(1, 12), size=(4097, 8))


# ----------------------------------------------------------------------------- 2. guards, repeats, a captured graph
class RawCall:
    """danbo_raster_mesh through ctypes on buffers with guard words around the workspace and every output"""

    def __init__(self, verts, faces, attr, mode, views, hx, H, W, want=("rgb", "depth", "tri_id"), background=(1., 1., 1.)):
        from core import _hip
        self.lib = _hip.lib()
        self.verts, self.faces, self.views = T(verts), T(faces, torch.int32), T(np.reshape(views, (-1, 12)))
        self.attr, self.bg = None if attr is None else T(attr), T(background)
        self.n, self.H, self.W, self.mode, self.hx, self.want = len(self.views), H, W, mode, hx, want
        n_bytes = self.lib.danbo_raster_workspace_bytes(len(verts), H, W)
        assert n_bytes > 0 and n_bytes % 4 == 0
        self.ws_words = n_bytes // 4
        self.ws = torch.full((self.ws_words + 32,), GUARD, dtype=torch.int32, device=DEV)
        sizes = {"rgb": self.n * H * W * 3, "depth": self.n * H * W, "tri_id": self.n * H * W}
        self.sizes = sizes
        self.out = {k: torch.full((sizes[k] + 32,), GUARD, dtype=torch.int32, device=DEV) for k in ("rgb", "depth", "tri_id")}

    def __call__(self):
        P = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
        outs = [P(self.out[k], 64) if k in self.want else None for k in ("rgb", "depth", "tri_id")]
        rc = self.lib.danbo_raster_mesh(P(self.verts), len(self.verts), P(self.faces), len(self.faces), P(self.attr), self.mode, P(self.views),
                                        self.n, self.hx, self.H, self.W, P(self.bg), P(self.ws, 64), *outs,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def results(self):
        torch.cuda.synchronize()
        assert torch.all(self.ws[:16] == GUARD) and torch.all(self.ws[16 + self.ws_words:] == GUARD), "a write outside the workspace"
        res = {}
        for k, buf in self.out.items():
            n = self.sizes[k]
            assert torch.all(buf[:16] == GUARD) and torch.all(buf[16 + n:] == GUARD), f"a write outside {k}"
            if k in self.want:
                shape = (self.n, self.H, self.W, 3) if k == "rgb" else (self.n, self.H, self.W)
                res[k] = buf[16:16 + n].cpu().numpy().view(np.int32 if k == "tri_id" else F32).reshape(shape)
            else:
                assert torch.all(buf == GUARD), f"{k} was not asked for and was written"
        return res


def test_guards_repeats_and_outputs_not_asked_for():
    verts, faces, normals, _ = rr.closed_mesh("torus")
    mv, mf, view, hx = mixed_scene(80, 96)
    for args in ((verts, faces, normals, rr.NORMAL, rr.MESH_VIEWS, rr.MESH_HX, 80, 96), (verts, faces, normals, rr.NORMAL, rr.MESH_VIEWS[:1], rr.MESH_HX, 5, 7),
                 (mv, mf, None, rr.FLAT, [view], hx, 80, 96)):
        ref = rr.host_raster(*args)
        call = RawCall(*args)
        call()
        first = call.results()
        assert all(same_bits(first[k], ref[k]) for k in ref)
        call()                                                   # the same buffers again: the clear is part of the call
        second = call.results()
        assert all(same_bits(first[k], second[k]) for k in ref), "two runs differ"
        for want in (("rgb",), ("depth",), ("tri_id",)):
            part = RawCall(*args, want=want)
            part()
            res = part.results()
            assert set(res) == set(want) and same_bits(res[want[0]], ref[want[0]])


def test_capture_and_replay_in_a_graph():
    verts, faces, normals, _ = rr.closed_mesh("two_spheres")
    args = (verts, faces, normals, rr.NORMAL, rr.MESH_VIEWS, rr.MESH_HX, 80, 96)
    ref = rr.host_raster(*args)
    eager = RawCall(*args)
    eager()
    assert all(same_bits(v, ref[k]) for k, v in eager.results().items())
    call = RawCall(*args)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):            # one linear chain of 4 launches per view
        call()
    torch.cuda.synchronize()
    for _ in range(2):
        for buf in call.out.values():
            buf[16:-16] = 0
        g.replay()
        res = call.results()
        assert all(same_bits(res[k], ref[k]) for k in ref)


# ----------------------------------------------------------------------------- 3. the turntable, end to end
def test_turntable_views_on_the_device():
    from core.utils import mesh_render as mr
    from test_raster_host import turntable_f64
    verts, _, _, _ = rr.closed_mesh("two_spheres")
    v = (verts / 27. - 0.5).astype(F32)
    views = mr.turntable_views(T(v))
    assert tuple(views.shape) == (91, 3, 4) and views.dtype == torch.float32 and views.is_cuda
    views = views.cpu().numpy().astype(np.float64)
    assert np.all(views[:, :, 3] == 0)
    want = turntable_f64(v, 91, 4.)
    got = np.einsum("fij,vj->fvi", views[:, :, :3], v.astype(np.float64))
    # the matrices are float64 rounded once to float32: 2^-24 relative per entry, three entries of at most 1 / height per row
    assert np.abs(got - want).max() <= 3 * 2.0 ** -24 * np.abs(views).max() * np.abs(v).max() * 1.01
    assert np.array_equal(views[0], views[90])
    with pytest.raises(ValueError):
        mr.turntable_views(T(v[:0]))


_SURFACE = {}


def synthetic_surface():
    """the danbo_mesh golden's pose at res 24 through the caster, threshold = the median of the positive densities"""
    if not _SURFACE:
        from test_gpu_modules import build
        g = golden("danbo_mesh")
        caster, _ = build("h36m_zju/danbo_base.txt", g)
        args = (T(g["kps"][:1]), T(g["skts"][:1]), T(g["bones"][:1]))
        dens = caster(*args, fwd_type="mesh", radius=float(g["radius"]), res=24).cpu().numpy()
        thr = float(F32(np.median(dens[dens > 0])))
        v, f, n = caster(*args, fwd_type="mesh_surface", radius=float(g["radius"]), res=24, threshold=thr, normals=True)
        _SURFACE.update(v=v, f=f, n=n)
    return _SURFACE


def test_turntable_of_the_casters_surface_equals_the_serial_rasteriser():
    from core.utils import mesh_render as mr
    from core.utils.evaluation_helpers import to8b
    s = synthetic_surface()
    v, f, n = s["v"], s["f"], s["n"]
    assert len(v) > 100 and len(f) > 100
    views = mr.turntable_views(v, 3, 4.)
    H, W = 48, 48
    for shade, attr, mode in (("normal", n, rr.NORMAL), ("flat", None, rr.FLAT)):
        frames = mr.render_turntable(v, f, normals=n, size=(H, W), shade=shade, n_frames=3, chunk=2)
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (3, H, W, 3) and frames.is_cuda
        ref = rr.host_raster(v.cpu().numpy(), f.cpu().numpy(), None if attr is None else attr.cpu().numpy(), mode, views.cpu().numpy(),
                             mr.HALF_EXTENT, H, W, want=("rgb", "tri_id"))
        assert np.array_equal(frames.cpu().numpy(), to8b(ref["rgb"]))
        hit = ref["tri_id"] >= 0
        print(f"turntable {shade}: V {len(v)} T {len(f)}, covered {hit.mean():.3f} of the frames")
        assert 0.02 < hit.mean() < 0.9 and np.all(frames.cpu().numpy()[~hit] == 255)
    flipped = mr.render_turntable(v, f, normals=n, size=(H, W), shade="flat", n_frames=3, flip=True)
    assert torch.equal(flipped, frames.flip(2))
    col = (torch.rand(len(v), 3, device=DEV) * 255).to(torch.uint8)
    a = mr.render_turntable(v, f, colors=col, size=(H, W), shade="color", n_frames=2)
    b = mr.render_turntable(v, f, colors=col.float() / 255., size=(H, W), shade="color", n_frames=2)
    assert torch.equal(a, b) and not torch.equal(a[0], a[1])
    with pytest.raises(ValueError):
        mr.render_turntable(v, f, size=(H, W), shade="normal")


def test_entry_points_write_the_turntable(tmp_path):
    import render_mesh
    import run_nerf
    import run_render
    from core.utils.mesh_io import read_ply_attrs
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "20", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "selected", "--selected_idxs", "1", "--render_mesh", "--mesh_res", "15",
            "--mesh_radius", "1.2"]
    run_render.run_render(base + ["--runname", "probe"])
    assert not (tmp_path / "out" / "probe" / "mesh_render").exists()
    sig = np.load(tmp_path / "out" / "probe" / "meshes" / "000_sigma.npy")
    thr = float(F32(np.quantile(sig[sig > 0], 0.25)))
    # The network has seen 20 steps: its surface is a small blob off the grid's centre, and the reference's views scale a mesh to
    # unit height WITHOUT centring it, which moves such a blob up or down by its offset / its height.  A tall image (the vertical
    # half extent is 0.6 H / W = 1.8) keeps it in view; that it is, is checked from the .ply before the frames are looked at.
    H, W = 120, 40
    run_render.run_render(base + ["--runname", "turn", "--mesh_threshold", repr(thr), "--mesh_render", "normal", "--mesh_render_res", str(H), str(W)])
    from core.utils import mesh_render as mr
    v = read_ply_attrs(str(tmp_path / "out" / "turn" / "meshes" / "000.ply"))[0]
    y = v.astype(np.float64) @ mr.base_rotation()[1]
    y = y / (y.max() - y.min())
    print("run_render turntable: V", len(v), "scaled y range", y.min(), y.max(), "visible band +-", 0.6 * H / W)
    assert len(v) > 0 and y.max() > -0.6 * H / W + 0.1 and y.min() < 0.6 * H / W - 0.1, "the scene of this test left the view"
    frames = np.load(tmp_path / "out" / "turn" / "mesh_render" / "000.npy")
    assert frames.shape == (91, H, W, 3) and frames.dtype == np.uint8 and (frames != 255).any() and (frames == 255).any()
    v, f, attrs = read_ply_attrs(str(tmp_path / "out" / "turn" / "meshes" / "000.ply"))
    assert attrs == {}                     # --mesh_render computes the normals it needs; the .ply holds what it was asked to hold
    # the stand-alone tool on the .ply files of a run: a bare mesh falls back to face normals, one with normals gives the same frames
    run_render.run_render(base + ["--runname", "withn", "--mesh_threshold", repr(thr), "--mesh_normals"])
    written = render_mesh.render_meshes(["--basedir", str(tmp_path / "out"), "--expname", "withn", "-ww", str(W), "-hh", str(H)])
    assert written == [str(tmp_path / "out" / "withn" / "mesh_render" / "000.npy")]
    assert np.array_equal(np.load(written[0]), frames)
    written = render_mesh.render_meshes(["--basedir", str(tmp_path / "out"), "--expname", "turn", "-ww", str(W), "-hh", str(H), "--flip"])
    flat = np.load(written[0])
    # (a pixel is white in all three channels only where nothing is drawn: no unit normal maps to (1, 1, 1))
    assert flat.shape == frames.shape and np.array_equal((flat == 255).all(-1), (frames[:, :, ::-1] == 255).all(-1))
    assert not np.array_equal(flat, frames[:, :, ::-1])
    with pytest.raises(ValueError, match="no vertex colours"):
        render_mesh.render_meshes(["--basedir", str(tmp_path / "out"), "--expname", "turn", "--shade", "color"])
