"""Vertex normals and colours of the extracted meshes on the GPU: k_mesh_normals (hip_ops.marching_cubes(normals=True)) against
the serial restatement of csrc/mesh_math.hpp bit for bit, determinism and bounds of danbo_mesh_normals, engine.colors against the
oracle's network forward, RayCaster.render_mesh_surface(normals=True, colors=True) on the danbo_mesh golden's pose and
run_render --render_mesh --mesh_normals --mesh_colors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import danbo_oracle as o
import mesh_attr_ref as a
import mesh_ref as m
from helpers import ROOT, golden, oracle_for, T, N, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
U = 2.0 ** -24
COLOR_BOUND = 2.5e-5 + U          # the project's 1e-4 on a raw logit through the sigmoid's slope of 1/4, and the sigmoid's own rounding


# ----------------------------------------------------------------------------- 8. kernel = serial restatement, bit for bit
def grids():
    rng = np.random.default_rng(21)
    noise = rng.standard_normal((65, 33, 17)).astype(F32)
    sparse = noise.copy()
    sparse[3:60] = 0                                  # chunks without a vertex between chunks with vertices
    return {"2x2x2": (np.array([[[1., -1.], [-1., -1.]], [[-1., -1.], [-1., 2.]]], F32), 0., -np.inf),
            "9x7x5": (rng.standard_normal((9, 7, 5)).astype(F32), 0.1, -np.inf),
            "17x9x33": (m.sphere_grid((17, 9, 33), R=3.7, centre=(8.2, 4.1, 15.6)), 0., -np.inf),
            "65x33x17 noise": (noise, 0.3, -np.inf),
            "65x33x17 mostly zero": (sparse, 0.3, -np.inf),
            "floored noise": ((rng.standard_normal((19, 12, 23)) * 5 - 1).astype(F32), 2., 0.),
            "alternating": (a.alternating_grid(), 0., -np.inf),
            "nan / inf": (a.wild_grid(), 0.5, -np.inf)}


@pytest.mark.parametrize("name", sorted(grids()))
def test_normals_kernel_equals_the_serial_restatement_bitwise(name):
    from core import hip_ops
    sigma, iso, floor = grids()[name]
    want = a.host_normals(sigma, iso, floor)
    st = T(sigma)
    v, f, n = hip_ops.marching_cubes(st, iso, floor=floor, normals=True)
    assert n.dtype == torch.float32 and n.is_cuda and tuple(n.shape) == (len(want), 3)
    print(name, "V", len(want))
    assert len(want) > 0 and same_bits(N(n), want)
    v2, f2 = hip_ops.marching_cubes(st, iso, floor=floor)
    assert torch.equal(v, v2) and torch.equal(f, f2)
    hv, hf = m.host_extract(sigma, iso, floor)
    assert same_bits(N(v), hv) and same_bits(N(f), hf)


def test_normals_of_a_strided_view_of_an_empty_surface_and_of_a_scaled_output():
    from core import hip_ops
    base = m.sphere_grid()
    view = T(np.ascontiguousarray(base.transpose(1, 0, 2))).transpose(1, 0)         # the 28^3 sphere through a transposed view
    assert not view.is_contiguous() and view.stride(2) == 1
    want = a.host_normals(base, 0.)
    v, f, n = hip_ops.marching_cubes(view, 0., normals=True)
    assert len(want) > 1000 and same_bits(N(n), want)
    # scale and offset move the vertices and leave the (index-space) normals
    v2, f2, n2 = hip_ops.marching_cubes(view, 0., scale=1. / 27, offset=(-.5, -.5, -.5), normals=True)
    assert torch.equal(n2, n) and torch.equal(f2, f) and not torch.equal(v2, v)
    v0, f0, n0 = hip_ops.marching_cubes(T(np.full((9, 9, 9), F32(1.))), 2., normals=True)
    assert tuple(v0.shape) == (0, 3) and tuple(f0.shape) == (0, 3) and tuple(n0.shape) == (0, 3) and n0.dtype == torch.float32


# ----------------------------------------------------------------------------- 10. determinism and bounds
GUARD = 0x5AFEC0DE


def test_two_runs_give_the_same_bits_and_nothing_is_written_beyond_the_capacity():
    from core import _hip
    lib = _hip.lib()
    sigma = m.noise_grid(4, (33, 29, 70))
    want = a.host_normals(sigma, 0.)
    st = T(sigma)
    nx, ny, nz = st.shape
    n_bytes = lib.danbo_mesh_workspace_bytes(nx, ny, nz)
    ws = torch.full((n_bytes // 4 + 16,), GUARD, dtype=torch.int32, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grid = (P(st), nx, ny, nz, st.stride(0), st.stride(1), -np.inf, 0.)
    assert lib.danbo_mesh_count(*grid, P(ws), P(counts), stream) == 0
    V, Tn = counts.tolist()
    assert V == len(want) > 1000
    ws_before = ws.clone()
    guard_f = float(np.array([GUARD], np.uint32).view(F32)[0])

    def run(cap):
        buf = torch.full((16 + 3 * V + 16,), guard_f, dtype=torch.float32, device=DEV)
        rc = lib.danbo_mesh_normals(*grid, P(ws), ctypes.c_void_p(buf.data_ptr() + 64), cap, stream)
        torch.cuda.synchronize()
        words = N(buf).view(np.uint32)
        assert np.all(words[:16] == GUARD) and np.all(words[16 + 3 * cap:] == GUARD), "a write outside the cap_v rows"
        return rc, N(buf)[16:16 + 3 * cap].reshape(-1, 3)

    rc, first = run(V)
    rc2, second = run(V)
    assert rc == 0 and rc2 == 0 and same_bits(first, want) and same_bits(second, first)
    # a short capacity: the return value danbo_mesh_extract gives for one, the rows below it, the last slot untouched
    verts = torch.empty(3 * V, dtype=torch.float32, device=DEV)
    tris = torch.empty(3 * Tn, dtype=torch.int32, device=DEV)
    rc_extract = lib.danbo_mesh_extract(*grid, P(ws), 1.0, 0., 0., 0., P(verts), V - 1, P(tris), Tn, stream)
    for cap in (V - 1, V // 2, 1, 0):
        rc, rows = run(cap)
        assert rc == rc_extract == 0 and same_bits(rows, want[:cap]), cap
    assert torch.equal(ws, ws_before)


# ----------------------------------------------------------------------------- 11. engine.colors against the oracle
def mesh_pose():
    g = golden("danbo_mesh")
    return g, g["kps"][:1], g["skts"][:1], g["bones"][:1]


def colour_queries(orc, n=300, seed=5):
    """n points around the golden pose, half inside at least one bone volume of the DANBO oracle `orc` and half outside every one;
    unit directions, the six axis directions among them; frame-code indices"""
    g, kps, skts, bones = mesh_pose()
    rng = np.random.default_rng(seed)
    cand = (rng.uniform(-float(g["radius"]), float(g["radius"]), size=(6000, 3)) + kps[0, 0]).astype(F32)
    pts_t = o.bone_local(cand.reshape(-1, 1, 3), np.repeat(skts, len(cand), 0), orc.align)
    _, valid = o.in_volume(pts_t, orc.sd['graph_net.axis_scale'])
    inside = valid.reshape(len(cand), -1).any(-1)
    assert inside.sum() >= n // 2 and (~inside).sum() >= n // 2
    pts = np.concatenate([cand[inside][:n // 2], cand[~inside][:n - n // 2]])
    dirs = rng.standard_normal((n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(F32)
    dirs[:3], dirs[n // 2:n // 2 + 3] = np.eye(3, dtype=F32), -np.eye(3, dtype=F32)
    cams = rng.integers(0, int(g["n_framecodes"]), size=n).astype(np.int64)
    order = rng.permutation(n)                              # inside and outside rows mixed over the chunks
    return pts[order], dirs[order], cams[order], np.concatenate([np.ones(n // 2, bool), np.zeros(n - n // 2, bool)])[order]


def oracle_colours(orc, pts, dirs, cams):
    _, kps, skts, bones = mesh_pose()
    raw, _ = orc.forward(pts.reshape(-1, 1, 3), dirs, np.repeat(skts, len(pts), 0), np.repeat(bones, len(pts), 0), cam_idxs=cams)
    return 1. / (1. + np.exp(-raw[:, 0, :3].astype(np.float64)))


def check_colours(eng, orc, pts, dirs, cams, name):
    _, kps, skts, bones = mesh_pose()
    col = eng.colors(T(pts), T(dirs), T(skts), T(bones), cam_idx=T(cams, torch.int64), netchunk=128)
    assert tuple(col.shape) == (len(pts), 3) and col.dtype == torch.float32
    want = oracle_colours(orc, pts, dirs, cams)
    err = float(np.abs(N(col).astype(np.float64) - want).max())
    print(name, "max |colour - oracle|", err, "bound", COLOR_BOUND)
    assert N(col).min() >= 0 and N(col).max() <= 1
    assert err <= COLOR_BOUND
    one = eng.colors(T(pts), T(dirs), T(skts), T(bones), cam_idx=T(cams, torch.int64))          # one chunk: the same bits
    assert torch.equal(one, col)
    return col


def test_danbo_colours_against_the_oracle():
    from test_gpu_modules import build
    g = golden("danbo_mesh")
    caster, _ = build("h36m_zju/danbo_base.txt", g)
    orc = oracle_for(g)[0]
    pts, dirs, cams, inside = colour_queries(orc)
    eng = caster._engine()
    col = check_colours(eng, orc, pts, dirs, cams, "danbo")
    # rows outside every volume: the sigmoid of the row's empty-space raw
    _, kps, skts, bones = mesh_pose()
    _, raw_empty = eng.view_constants(T(dirs), T(skts), T(cams, torch.int64))
    out = torch.tensor(~inside, device=DEV)
    assert int(out.sum()) == 150 and torch.equal(col[out], torch.sigmoid(raw_empty[out, :3]))
    assert not torch.equal(col[~out], torch.sigmoid(raw_empty[~out, :3]))


def test_anerf_colours_against_the_oracle():
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    g = golden("anerf_stages")
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt"))
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=int(g["n_framecodes"]), rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    _, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    orc, cfg, sd, rest = oracle_for(g)
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    pts, dirs, cams, _ = colour_queries(oracle_for(golden("danbo_mesh"))[0])
    check_colours(caster._engine(), orc, pts, dirs, cams, "anerf")


_TWO_NET = {}


def two_net_surface():
    """a two-network DANBO caster on the golden pose at res 15: the surface with normals and colours"""
    if not _TWO_NET:
        from test_gpu_two_net import oracles, two_net_caster
        args, caster, kw, cfg, sds, _ = two_net_caster("h36m_zju/danbo_base.txt", "danbo_base")
        g, kps, skts, bones = mesh_pose()
        pose = (T(kps), T(skts), T(bones))
        dens = caster(*pose, fwd_type="mesh", radius=float(g["radius"]), res=15)
        pos = np.sort(N(dens)[N(dens) > 0])
        thr = float(pos[len(pos) // 2])
        v, f, n, c, dens2 = caster(*pose, fwd_type="mesh_surface", radius=float(g["radius"]), res=15, threshold=thr, normals=True,
                                   colors=True, return_density=True)
        assert torch.equal(dens2, dens)
        _TWO_NET.update(caster=caster, orcs=oracles(cfg, sds), pose=pose, g=g, v=v, f=f, n=n, c=c)
    return _TWO_NET


def test_two_network_caster_asks_the_fine_network_for_the_colours():
    from core.utils.evaluation_helpers import to8b
    r = two_net_surface()
    caster, g, (kps, skts, bones) = r["caster"], r["g"], r["pose"]
    orc_c, orc_f = r["orcs"]
    fine, coarse = caster._engine(network=caster.network_fine), caster._engine()
    pts, dirs, cams, _ = colour_queries(orc_f)
    check_colours(fine, orc_f, pts, dirs, cams, "two-network, fine")
    assert float(np.abs(N(coarse.colors(T(pts), T(dirs), skts, bones, cam_idx=T(cams, torch.int64))) - oracle_colours(orc_f, pts, dirs, cams)).max()) > 1e-2
    # the caster's colours are the fine network's
    v, n, c = r["v"], r["n"], r["c"]
    assert len(v) > 100 and c.dtype == torch.uint8 and tuple(c.shape) == (len(v), 3)
    world = kps[0, 0] + 2. * float(g["radius"]) * v
    assert np.array_equal(N(c), to8b(N(fine.colors(world, -n, skts, bones))))
    assert not np.array_equal(N(c), to8b(N(coarse.colors(world, -n, skts, bones))))


# ----------------------------------------------------------------------------- 12. the caster on the golden pose
def test_surface_with_normals_and_colours_of_the_golden_pose():
    """res 15, the threshold a value of the grid itself (so some vertices lie ON grid points, t = 0 or 1): the normals are the
    operator's on the returned grid, the colours to8b(engine.colors(root + 2 radius v, -n)), and a vertex on the grid point (i, j, k)
    of the returned (x-y swapped) array lies at that point's entry [j, i, k] of render_mesh_density's own 'xy'-meshgrid coordinates
    within 2^-21 max(1, |x|): v = fma(p, 1/15, -.5) carries 2^-26 + 2^-24, times 2 radius <= 2^-22; the product, the sum and the
    grid's own rounding of the float64 linspace are half an ulp each."""
    from core import hip_ops
    from core.raycasters import RayCaster
    from core.utils.evaluation_helpers import to8b
    from test_gpu_modules import build
    g = golden("danbo_mesh")
    caster, _ = build("h36m_zju/danbo_base.txt", g)
    kps, skts, bones = T(g["kps"][:1]), T(g["skts"][:1]), T(g["bones"][:1])
    radius, res = float(g["radius"]), 15
    dens = caster(kps, skts, bones, fwd_type="mesh", radius=radius, res=res)
    pos = np.sort(N(dens)[N(dens) > 0])
    thr = float(pos[len(pos) // 2])
    plain = caster(kps, skts, bones, fwd_type="mesh_surface", radius=radius, res=res, threshold=thr)
    assert len(plain) == 2
    v, f, n, c, dens2 = caster(kps, skts, bones, fwd_type="mesh_surface", radius=radius, res=res, threshold=thr, normals=True,
                               colors=True, return_density=True)
    assert torch.equal(dens2, dens) and torch.equal(v, plain[0]) and torch.equal(f, plain[1]) and len(v) > 100
    only_c = caster(kps, skts, bones, fwd_type="mesh_surface", radius=radius, res=res, threshold=thr, colors=True)
    only_n = caster(kps, skts, bones, fwd_type="mesh_surface", radius=radius, res=res, threshold=thr, normals=True)
    assert len(only_c) == 3 and torch.equal(only_c[2], c) and len(only_n) == 3 and torch.equal(only_n[2], n)
    vi, fi, ni = hip_ops.marching_cubes(dens, thr, floor=0., normals=True)
    assert torch.equal(ni, n) and torch.equal(fi, f)
    assert same_bits(N(n), a.host_normals(np.ascontiguousarray(N(dens)), thr, 0.))
    assert np.all(np.abs(np.linalg.norm(N(n).astype(np.float64), axis=-1) - 1) <= 4 * U)
    eng = caster._engine()
    world = kps[0, 0] + 2. * radius * v
    assert c.dtype == torch.uint8 and tuple(c.shape) == (len(v), 3)
    assert np.array_equal(N(c), to8b(N(eng.colors(world, -n, skts, bones))))
    # vertices on grid points
    idx = N(vi)
    on_grid = np.all(idx == np.round(idx), axis=1)
    assert on_grid.any()
    i, j, k = idx[on_grid].astype(np.int64).T
    coords = N(RayCaster.mesh_grid(radius, res, DEV)).astype(np.float64)[j, i, k] + g["kps"][0, 0].astype(np.float64)
    got = N(world)[on_grid].astype(np.float64)
    err = np.abs(got - coords) / np.maximum(1., np.abs(coords))
    print("golden pose: V", len(v), "vertices on grid points", int(on_grid.sum()), "max |world - grid| / max(1, |x|)", float(err.max()))
    assert err.max() <= 2.0 ** -21
    assert np.all(N(dens)[i, j, k] == F32(thr))
    # the density the network gives at those world positions is the grid's there (not that of the x-y swapped point)
    d_at = N(caster(world[torch.tensor(on_grid, device=DEV)].reshape(-1, 1, 3), kps, skts, bones, fwd_type="density")).reshape(-1)
    assert np.abs(d_at - thr).max() <= 1e-3 * thr


# ----------------------------------------------------------------------------- 13. entry point
def test_run_render_writes_normals_and_colours(tmp_path):
    import run_nerf
    import run_render
    from core.utils.mesh_io import read_ply, read_ply_attrs, write_ply
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "20", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "selected", "--selected_idxs", "1", "--render_mesh", "--mesh_res", "15",
            "--mesh_radius", "1.2"]
    run_render.run_render(base + ["--runname", "probe"])
    sig = np.load(tmp_path / "out" / "probe" / "meshes" / "000_sigma.npy")
    thr = float(F32(np.median(sig[sig > 0])))
    base += ["--mesh_threshold", repr(thr)]
    run_render.run_render(base + ["--runname", "plain"])
    plain = tmp_path / "out" / "plain" / "meshes" / "000.ply"
    v, f = read_ply(str(plain))
    assert len(v) > 0 and len(f) > 0
    write_ply(str(tmp_path / "again.ply"), v, f)
    assert open(plain, "rb").read() == open(tmp_path / "again.ply", "rb").read()
    hv, hf = m.host_extract(sig, thr, scale=1. / 15, offset=(-.5, -.5, -.5))
    assert same_bits(v, hv) and same_bits(f, hf)
    run_render.run_render(base + ["--runname", "attrs", "--mesh_normals", "--mesh_colors"])
    v2, f2, attrs = read_ply_attrs(str(tmp_path / "out" / "attrs" / "meshes" / "000.ply"))
    assert same_bits(v2, v) and same_bits(f2, f) and set(attrs) == {"normals", "colors"}
    n, c = attrs["normals"], attrs["colors"]
    assert n.shape == (len(v), 3) and np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1) <= 4 * U)
    assert same_bits(n, a.host_normals(sig, thr))
    assert c.dtype == np.uint8 and c.shape == (len(v), 3)
    print("run_render mesh attributes: threshold", thr, "V", len(v), "colour range", int(c.min()), int(c.max()))
