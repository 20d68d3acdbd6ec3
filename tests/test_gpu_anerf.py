"""GPU parity tests of the A-NeRF path (cutoff PE kernels + W = 448 trunk + colour head) against the numpy
oracle and against the reference's own outputs (tests/golden/anerf_stages.npz)."""
import os

import numpy as np
import pytest
import torch

import danbo_oracle as o
from helpers import ROOT, golden, oracle_for, max_err, rel_err, raw_err, raw_rel_unfloored, T, N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def env():
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    g = golden("anerf_stages")
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt"))
    n_codes = int(g["n_framecodes"])
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    tr, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    orc, cfg, sd, rest = oracle_for(g)
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    return g, caster, kw, orc


def call(caster, kw, g):
    pose = g["pose_of_ray"]
    return caster(T(g["ray_batch"]), N_samples=int(g["N_samples"]), kp_batch=T(g["kps"][pose]), skts=T(g["skts"][pose]),
                  cyls=T(g["cyls"][pose]), bones=T(g["bones"][pose]), cams=T(g["cam_idx"], torch.int64),
                  N_importance=int(g["N_importance"]), N_uniques=2, **kw)


def test_encode_kernel_matches_reference_density_inputs(env):
    from core import hip_ops as ops
    g, caster, kw, orc = env
    eng = caster._engine()
    rb = g["ray_batch"]
    R, S = g["z_coarse"].shape
    x0, w = ops.anerf_encode(T(rb[:, 0:3]), T(rb[:, 3:6]), T(g["skts"]), eng.align, eng.cutoff, 20.0, 7, 0, R * S,
                             z=T(g["z_coarse"]))
    assert x0.shape == (R * S, 432)
    # sin(64 sh) with sh = (c - v) 2/c - 1 amplifies 1e-6 of distance round-off 256x
    assert max_err(N(x0), g["density_inputs"]) < 2e-4
    assert max_err(N(x0)[:, 360:], g["r"].reshape(-1, 72)) < 3e-6
    wo = 1.0 - 1.0 / (1.0 + np.exp(-20.0 * (g["v"].reshape(-1, 24).astype(np.float64) - 0.5)))
    assert max_err(N(w), wo) < 2e-5
    # a window of rows, and explicit points instead of (rays, z), give the same rows bit for bit
    x1, w1 = ops.anerf_encode(T(rb[:, 0:3]), T(rb[:, 3:6]), T(g["skts"]), eng.align, eng.cutoff, 20.0, 7, 5 * S, 3 * S + 1,
                              z=T(g["z_coarse"]))
    assert torch.equal(x1, x0[5 * S:8 * S + 1]) and torch.equal(w1, w[5 * S:8 * S + 1])
    x2, _ = ops.anerf_encode(None, None, T(g["skts"]), eng.align, eng.cutoff, 20.0, 7, 0, R * S, pts=T(g["pts"]))
    assert max_err(N(x2), N(x0)) < 2e-4


def test_view_direction_encoding(env):
    from core import hip_ops as ops
    g, caster, kw, orc = env
    E = N(ops.anerf_view_pe(T(g["ray_batch"][:, 3:6]), T(g["skts"]), 4))
    assert E.shape == (48, 648)
    assert max_err(E[:, :72], g["view_dirs"]) < 1e-6
    d = g["view_dirs"].astype(np.float64)
    for l in range(4):
        assert max_err(E[:, 72 * (1 + 2 * l):72 * (2 + 2 * l)], np.sin(d * 2 ** l)) < 2e-6
        assert max_err(E[:, 72 * (2 + 2 * l):72 * (3 + 2 * l)], np.cos(d * 2 ** l)) < 2e-6


def test_model_forward_matches_reference_raw(env):
    g, caster, kw, orc = env
    pose = g["pose_of_ray"]
    rb = g["ray_batch"]
    inputs = dict(pts=T(g["pts"]), kps=T(g["kps"][pose]), skts=T(g["skts"][pose]), bones=T(g["bones"][pose]),
                  rest_pose=T(g["rest_pose"]).reshape(1, 1, 24, 3), align_transforms=caster.transforms[:1, None].to(DEV),
                  N_uniques=2, rays_o=T(rb[:, None, 0:3]), rays_d=T(rb[:, None, 3:6]), cam_idxs=T(g["cam_idx"], torch.int64))
    raw, enc = caster.network(inputs)
    assert raw.shape == (48, 12, 4)
    assert raw_err(N(raw), g["raw_coarse"]) < 1e-4          # north_star bound; measured 1.4e-5 (profiles/r03_parity_measured.txt)
    assert raw_rel_unfloored(N(raw), g["raw_coarse"]) < 1e-4
    # small row chunks (whole rays per chunk) give the same result
    caster._engine().rows_per_chunk = 5 * 12
    raw2, _ = caster.network(inputs)
    caster._engine().rows_per_chunk = 1 << 18
    assert raw_err(N(raw2), N(raw)) < 1e-5


def test_model_forward_matches_reference_raw_at_tau_2000(env):
    """BASELINE config 5's converged setting at the RAW level: tau = 2000 makes the cutoff weight a step --
    w = 1 - sigmoid(tau (v - c)) moves by tau / 4 = 500 per unit of distance AT the shell, so 1e-7 of fp32 round-off in a joint
    distance within a few mm of c = 0.5 m changes w by up to 1e-4 and the logits with it (the pinned oracle shows the same:
    tests/test_oracle_anerf.py::test_converged_tau_2000).  5 mm off the shell the sensitivity is tau exp(-10) = 0.09 per unit:
    every sample with NO joint distance inside that shell must meet the north_star bound; the shell samples a loose one."""
    g, caster, kw, orc = env
    pose = g["pose_of_ray"]
    rb = g["ray_batch"]
    inputs = dict(pts=T(g["pts"]), kps=T(g["kps"][pose]), skts=T(g["skts"][pose]), bones=T(g["bones"][pose]),
                  rest_pose=T(g["rest_pose"]).reshape(1, 1, 24, 3), align_transforms=caster.transforms[:1, None].to(DEV),
                  N_uniques=2, rays_o=T(rb[:, None, 0:3]), rays_d=T(rb[:, None, 3:6]), cam_idxs=T(g["cam_idx"], torch.int64))
    net = caster.network
    with torch.no_grad():
        net.pe_fn.tau.fill_(2000.0)
        net.dirs_pe_fn.tau.fill_(2000.0)
    try:
        raw, _ = net(inputs)
    finally:
        with torch.no_grad():
            net.pe_fn.tau.fill_(20.0)
            net.dirs_pe_fn.tau.fill_(20.0)
    raw, ref = N(raw), g["tau2000_raw_coarse"]
    assert not np.allclose(ref, g["raw_coarse"], atol=1e-2)             # tau does change the logits
    shell = (np.abs(g["v"].reshape(48, 12, 24) - 0.5) < 0.005).any(-1)  # [R,S]: some joint sits within 5 mm of the cutoff
    assert 0 < shell.sum() < 0.25 * shell.size
    floor = 0.05 * np.abs(ref).reshape(-1, 4).max(0)
    err = np.abs(raw - ref) / np.maximum(np.abs(ref), floor)
    print(f"tau 2000: off-shell raw_err {err[~shell].max():.3e} ({int((~shell).sum())} samples), shell {err[shell].max():.3e} ({int(shell.sum())})")
    assert err[~shell].max() < 1e-4
    assert err[shell].max() < 0.05


def test_anerf_cutoff_pe_mlp_custom_op(env):
    """torch.ops.danbo.anerf_cutoff_pe_mlp (the forward-only pair of SURVEY 8b) on state_dict tensors: the module's raw bit for bit,
    the reference's raw within the north_star bound; schema / fake-tensor opcheck"""
    from core import custom_ops  # noqa: F401
    g, caster, kw, orc = env
    net = caster.network
    pose = g["pose_of_ray"]
    rb = g["ray_batch"]
    sd = dict(net.state_dict())
    D = len(net.pts_linears)
    names = ([f"pts_linears.{i}.weight" for i in range(D)] + [f"pts_linears.{i}.bias" for i in range(D)]
             + ["alpha_linear.weight", "alpha_linear.bias", "feature_linear.weight", "feature_linear.bias", "views_linears.0.weight",
                "views_linears.0.bias", "rgb_linear.weight", "rgb_linear.bias", "pe_fn.cutoff_dist", "dirs_pe_fn.cutoff_dist",
                "framecodes.codes.weight"])
    params = [sd[k].detach() for k in names]
    skts_g = T(g["skts"])
    align = caster.transforms[0].to(DEV)
    args = (T(g["pts"]), T(rb[:, 3:6]), skts_g, align, T(g["cam_idx"], torch.int64), params, float(net.pe_fn.tau),
            int(net.pe_fn.num_freqs), int(net.dirs_pe_fn.num_freqs))
    raw = torch.ops.danbo.anerf_cutoff_pe_mlp(*args)
    inputs = dict(pts=T(g["pts"]), kps=T(g["kps"][pose]), skts=T(g["skts"][pose]), bones=T(g["bones"][pose]),
                  rest_pose=T(g["rest_pose"]).reshape(1, 1, 24, 3), align_transforms=caster.transforms[:1, None].to(DEV),
                  N_uniques=2, rays_o=T(rb[:, None, 0:3]), rays_d=T(rb[:, None, 3:6]), cam_idxs=T(g["cam_idx"], torch.int64))
    ref, _ = net(inputs)
    assert torch.equal(raw, ref)
    assert raw_err(N(raw), g["raw_coarse"]) < 1e-4
    torch.library.opcheck(torch.ops.danbo.anerf_cutoff_pe_mlp, args, test_utils=("test_schema", "test_faketensor"))


def test_caster_call_matches_reference_maps_tau20_and_tau2000(env):
    g, caster, kw, orc = env
    out = call(caster, kw, g)
    assert set(out) == {"rgb_map", "disp_map", "acc_map", "alpha", "T_i", "rgb0", "disp0", "acc0", "alpha0"}
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert max_err(N(out[k]), g["final_" + k]) < 5e-5, k            # measured 9.5e-6 (round 4's bound: 1e-3)
    assert o.psnr(N(out["rgb_map"]), g["final_rgb_map"]) > 90.0
    net = caster.network
    with torch.no_grad():
        net.pe_fn.tau.fill_(2000.0)
        net.dirs_pe_fn.tau.fill_(2000.0)
    try:
        out = call(caster, kw, g)
        assert max_err(N(out["rgb_map"]), g["tau2000_final_rgb_map"]) < 5e-5      # measured 7.2e-6 (round 4's bound: 5e-3)
        assert o.psnr(N(out["rgb_map"]), g["tau2000_final_rgb_map"]) > 90.0
    finally:
        with torch.no_grad():
            net.pe_fn.tau.fill_(20.0)
            net.dirs_pe_fn.tau.fill_(20.0)


def test_full_render_against_oracle_and_density_query(env):
    """more rays than one chunk, mean frame code (cams = -1), and forward_pts density"""
    from core.utils import synthetic as syn
    g, caster, kw, orc = env
    scene = syn.make_scene(n_poses=1, H=24, W=24, n_views=1, pose_seed=3)
    ro, rd = scene["rays"][0]
    rb = syn.ray_batch(ro, rd)
    R = len(ro)
    z = np.zeros(R, np.int64)
    caster._engine().rows_per_chunk = 100 * 16
    out = caster(T(rb), N_samples=16, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                 bones=T(scene["bones"][z]), cams=T(-np.ones(R), torch.int64), N_importance=8, N_uniques=1, **kw)
    caster._engine().rows_per_chunk = 1 << 18
    ref = orc.render(rb, scene["skts"][z], scene["bones"][z], scene["cyls"][z], cam_idxs=-np.ones(R, np.int64),
                     n_uniques=1, N_samples=16, N_importance=8, chunk=R)
    assert max_err(N(out["rgb_map"]), ref["rgb_map"]) < 5e-5                        # measured 5.4e-6 / 8.9e-6 (round 4's bounds: 2e-3)
    assert o.psnr(N(out["rgb_map"]), ref["rgb_map"]) > 90.0
    assert max_err(N(out["acc_map"]), ref["acc_map"]) < 5e-5
    pts = np.random.default_rng(0).uniform(-0.6, 0.6, size=(500, 3)).astype(np.float32) + scene["kps"][0, 0]
    dens = caster(T(pts).reshape(-1, 1, 3), T(scene["kps"]), T(scene["skts"]), T(scene["bones"]), fwd_type="density")
    raw, _ = orc.forward(pts.reshape(-1, 1, 3), np.zeros((500, 3), np.float32) + [0, 0, 1],
                         np.repeat(scene["skts"], 500, 0), cam_idxs=None)
    assert raw_err(N(dens).reshape(-1), raw[:, 0, 3]) < 1e-4      # measured 1.1e-5
