"""The two-network hierarchical mode (single_net = False: a coarse and a separate fine network) on the GPU: the two-network pdf of
every importance kernel against the numpy restatement, the A-NeRF and DANBO two-network renders against the composed oracle
(tests/test_two_net_oracle.py), the caster's whole-image and HIP-graph paths, and the autograd training path."""
import os

import numpy as np
import pytest
import torch

import danbo_oracle as o
from helpers import ROOT, max_err, raw_err, T, N
from test_two_net_oracle import importance_z_two_net, render_two_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("S,Sf", [(7, 3), (48, 16), (96, 48), (200, 64), (272, 24)])
def test_two_net_importance_kernels_match_the_restatement(S, Sf):
    """wave-per-ray kernel (S, Sf <= 64), its long-ray form (64 < S <= 256, Sf <= 64) and the per-thread fallback, each with the
    two-network pdf, deterministic and random u"""
    from core import hip_ops as ops
    rng = np.random.default_rng(S)
    R = 200
    z = np.sort(rng.uniform(2, 5, size=(R, S)).astype(np.float32), -1)
    # (no alpha_base in this pdf: weights bounded away from 0 keep t = (u - c0) / (c1 - c0) well conditioned)
    w = (0.02 + rng.uniform(size=(R, S)) ** 4).astype(np.float32)
    for u in (None, rng.uniform(size=(R, Sf)).astype(np.float32)):
        zs, zf, idx = ops.importance_samples(T(z), T(w), Sf, None if u is None else T(u), two_net=True)
        _, z_fine, _ = importance_z_two_net(z, w, Sf, u=u)
        assert max_err(N(zf), z_fine) < 1e-4
        assert np.mean(np.abs(N(zf) - z_fine)) < 2e-6
        cat = np.concatenate([z, N(zf)], -1)
        assert np.array_equal(N(zs), np.sort(cat, -1))
        assert np.array_equal(N(idx).astype(np.int64), np.argsort(cat, -1, kind="stable"))
        # ... and not the single-network pdf
        zs1, zf1, _ = ops.importance_samples(T(z), T(w), Sf, None if u is None else T(u))
        assert max_err(N(zf1), N(zf)) > 1e-3


def test_two_net_importance_over_a_ray_list_and_fused_composite():
    from core import hip_ops as ops
    rng = np.random.default_rng(7)
    # the long-ray kernel over a list: listed rows equal the full call, the others stay untouched
    R, S, Sf = 300, 96, 48
    z = np.sort(rng.uniform(2, 5, size=(R, S)).astype(np.float32), -1)
    w = (0.02 + rng.uniform(size=(R, S)) ** 4).astype(np.float32)
    full = ops.importance_samples(T(z), T(w), Sf, two_net=True)
    listed = np.sort(rng.choice(R, 117, replace=False)).astype(np.int32)
    flat = dict(z_fine=torch.full((R, Sf), -7.0, device=DEV), ray_list=T(listed, torch.int32),
                ray_count=T(np.array([len(listed)]), torch.int32))
    zs, zf, idx = ops.importance_samples(T(z), T(w), Sf, flat=flat, two_net=True)
    sel = torch.zeros(R, dtype=torch.bool, device=DEV)
    sel[T(listed, torch.int64)] = True
    assert torch.equal(zf[sel], full[1][sel]) and torch.equal(zs[sel], full[0][sel]) and torch.equal(idx[sel], full[2][sel])
    assert bool((zf[~sel] == -7.0).all())
    # the fused coarse composite + two-network resampling: bit for bit the composite followed by the two-network resampling
    R, S, Sf = 500, 48, 24
    z = np.sort(rng.uniform(2, 5, size=(R, S)).astype(np.float32), -1)
    raw = rng.normal(size=(R, S, 4)).astype(np.float32) * 3
    rd = rng.normal(size=(R, 3)).astype(np.float32)
    for u in (None, T(rng.uniform(size=(R, Sf)).astype(np.float32))):
        out0, zs, zf, idx = ops.composite_importance(T(raw), T(z), T(rd), Sf, 1.0, u=u, two_net=True)
        ref0 = ops.composite(T(raw), T(z), T(rd), 1.0)
        rzs, rzf, ridx = ops.importance_samples(T(z), ref0["weights"], Sf, u, two_net=True)
        for k in ("rgb_map", "disp_map", "acc_map", "weights", "alpha"):
            assert torch.equal(out0[k], ref0[k]), k
        assert torch.equal(zf, rzf) and torch.equal(zs, rzs) and torch.equal(idx, ridx)
        single = ops.composite_importance(T(raw), T(z), T(rd), Sf, 1.0, u=u)
        assert not torch.equal(single[2], zf)


# ----------------------------------------------------------------------------- casters
def two_net_caster(cfg_file, cfg_name, seeds=(3, 4), n_codes=20, rest_scale=0.48):
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", cfg_file))
    args.single_net = False
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(rest_scale), hwf=(64, 64, 80.))
    tr, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    assert caster.two_net
    cfg = syn.model_config(cfg_name)
    sds = [syn.make_state_dict(cfg, seed=s, n_framecodes=n_codes, rest=syn.rest_pose(rest_scale)) for s in seeds]
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sds[0].items()}, strict=True)
    caster.network_fine.load_state_dict({k: torch.tensor(v) for k, v in sds[1].items()}, strict=True)
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    return args, caster, kw, cfg, sds, tr


def oracles(cfg, sds, rest_scale=0.48):
    from core.utils import synthetic as syn
    cls = o.DanboOracle if cfg["nerf_type"] == "danbo" else o.AnerfOracle
    return [cls(cfg, sd, syn.rest_pose(rest_scale)) for sd in sds]


def body_scene(n=None, H=24, W=24, seed=3):
    from core.utils import synthetic as syn
    scene = syn.make_scene(n_poses=1, H=H, W=W, n_views=1, pose_seed=seed)
    ro, rd = scene["rays"][0]
    if n is not None:
        ro, rd = ro[:n], rd[:n]
    return scene, syn.ray_batch(ro, rd)


def cast(caster, kw, scene, rb, S, Sf, cams=None):
    R = len(rb)
    z = np.zeros(R, np.int64)
    cams = np.zeros(R, np.int64) if cams is None else cams
    return caster(T(rb), N_samples=S, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                  bones=T(scene["bones"][z]), cams=T(cams, torch.int64), N_importance=Sf, N_uniques=1, **kw)


def test_anerf_two_net_render_against_the_composed_oracle_and_density_query():
    args, caster, kw, cfg, sds, _ = two_net_caster("h36m_zju/anerf_base.txt", "anerf_base")
    orc_c, orc_f = oracles(cfg, sds)
    scene, rb = body_scene()
    R = len(rb)
    z = np.zeros(R, np.int64)
    cams = -np.ones(R, np.int64)
    out = {k: v.clone() for k, v in cast(caster, kw, scene, rb, 16, 8, cams).items()}
    ref = render_two_net(orc_c, orc_f, rb, scene["skts"][z], scene["bones"][z], scene["cyls"][z], cams, 1, 16, 8)
    assert out["alpha"].shape == (R, 24) and out["alpha0"].shape == (R, 16)
    for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
        assert max_err(N(out[k]), ref[k]) < 5e-5, k
    assert o.psnr(N(out["rgb_map"]), ref["rgb_map"]) > 90.0
    assert 0.05 < float(ref["acc_map"].mean())
    # a change of the fine network alone moves the final maps and leaves the coarse maps' bits
    with torch.no_grad():
        caster.network_fine.pts_linears[3].weight.mul_(1.5)
    out2 = cast(caster, kw, scene, rb, 16, 8, cams)
    assert torch.equal(out2["rgb0"], out["rgb0"]) and torch.equal(out2["acc0"], out["acc0"])
    assert max_err(N(out2["rgb_map"]), N(out["rgb_map"])) > 1e-4
    with torch.no_grad():
        caster.network_fine.pts_linears[3].weight.div_(1.5)
    # the density query uses the fine network (reference raycasters.py:716-724)
    pts = np.random.default_rng(0).uniform(-0.6, 0.6, size=(500, 3)).astype(np.float32) + scene["kps"][0, 0]
    dens = caster(T(pts).reshape(-1, 1, 3), T(scene["kps"]), T(scene["skts"]), T(scene["bones"]), fwd_type="density")
    raw_f, _ = orc_f.forward(pts.reshape(-1, 1, 3), np.zeros((500, 3), np.float32) + [0, 0, 1], np.repeat(scene["skts"], 500, 0))
    raw_c, _ = orc_c.forward(pts.reshape(-1, 1, 3), np.zeros((500, 3), np.float32) + [0, 0, 1], np.repeat(scene["skts"], 500, 0))
    assert raw_err(N(dens).reshape(-1), raw_f[:, 0, 3]) < 1e-4
    assert raw_err(N(dens).reshape(-1), raw_c[:, 0, 3]) > 1e-2


def _danbo_engines(sd_c, sd_f, cfg):
    from core.render_engine import DanboEngine
    orc_c, orc_f = oracles(cfg, [sd_c, sd_f], cfg["rest_scale"])
    eng_c = DanboEngine(dict(cfg), {k: T(v) for k, v in sd_c.items()}, T(orc_c.align))
    eng_f = DanboEngine(dict(cfg), {k: T(v) for k, v in sd_f.items()}, T(orc_f.align))
    return eng_c, eng_f, orc_c, orc_f


@pytest.mark.parametrize("case", ["fine_volumes_larger", "fine_positive_empty_density", "coarse_positive_empty_density"])
def test_danbo_two_net_render_against_the_composed_oracle_and_lazy_equals_dense(case):
    from core.utils import synthetic as syn
    cfg = syn.model_config("danbo_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd_c = syn.make_state_dict(cfg, seed=3, n_framecodes=8, rest=rest)
    sd_f = syn.make_state_dict(cfg, seed=4, n_framecodes=8, rest=rest)
    if case == "fine_volumes_larger":
        sd_f["graph_net.axis_scale"] = (sd_f["graph_net.axis_scale"] * 1.4).astype(np.float32)
    positive = {"fine_positive_empty_density": sd_f, "coarse_positive_empty_density": sd_c}.get(case)
    if positive is not None:
        # the empty-space density (the MLP's density of a zero feature row) moved to +0.5 through the density bias
        eng, _, _, _ = _danbo_engines(positive, positive, cfg)
        eng.refresh()
        positive["alpha_linear.bias"] = (positive["alpha_linear.bias"] + (0.5 - float(eng.empty_consts[128]))).astype(np.float32)
    eng_c, eng_f, orc_c, orc_f = _danbo_engines(sd_c, sd_f, cfg)
    eng_c.refresh()
    eng_f.refresh()
    if case == "fine_positive_empty_density":
        assert eng_c.flat_rays_ok and not eng_f.flat_rays_ok
    elif case == "coarse_positive_empty_density":
        assert not eng_c.flat_rays_ok and eng_f.flat_rays_ok
    scene = syn.make_scene(n_poses=1, H=32, W=32, n_views=1, pose_seed=4)
    ro, rd = scene["rays"][0]
    R = len(ro)
    cam = np.zeros(R, np.int64)
    args = (T(ro), T(rd), T(scene["skts"]), T(scene["bones"]), T(scene["cyls"]), T(cam, torch.int64))
    for S, Sf in ((24, 12), (96, 32)):       # the fused coarse composite, and the unfused pair (S > 64)
        a = eng_c.render_two_net(eng_f, *args, S, Sf)
        b = eng_c.render_two_net(eng_f, *args, S, Sf, dense=True)
        c = eng_c.render_two_net(eng_f, *args, S, Sf, keep=True)
        for k in ("rgb_map", "disp_map", "acc_map", "alpha", "T_i", "rgb0", "disp0", "acc0", "alpha0"):
            assert torch.equal(a[k], b[k]), (S, k)
            assert torch.equal(a[k], c[k]), (S, k)
        nf = (N(c["near"]).reshape(-1, 1), N(c["far"]).reshape(-1, 1))
        ref = render_two_net(orc_c, orc_f, syn.ray_batch(ro, rd), scene["skts"][cam], scene["bones"][cam], scene["cyls"][cam], cam, 1,
                             S, Sf, near_far=nf)
        assert np.array_equal(N(c["z_coarse"]), ref["z_coarse"])
        print("DANBO two-net %s S=%d: measured %s psnr %.1f" % (case, S, {k: "%.2e" % max_err(N(a[k]), ref[k]) for k in
                                                                       ("rgb_map", "acc_map", "rgb0", "acc0")}, o.psnr(N(a["rgb_map"]), ref["rgb_map"])))
        # measured on the MI355X: coarse maps <= 1.2e-6; final maps <= 1.6e-5, except 2.6e-4 (PSNR 105.8) at 96 + 32 with a positive
        # empty-space density in the coarse network (every sample carries weight: the importance depths, chaotic in the coarse weights'
        # round-off, move by ulps and the fine network sees other points) -- the final maps' bound is test_oracle_golden.py's 5e-4
        for k in ("rgb0", "acc0"):
            assert max_err(N(a[k]), ref[k]) < 1e-5, (S, k)
        for k in ("rgb_map", "acc_map"):
            assert max_err(N(a[k]), ref[k]) < 5e-4, (S, k)
        assert o.psnr(N(a["rgb_map"]), ref["rgb_map"]) > 100.0
        if case == "fine_volumes_larger":
            # the fine pass's in-volume mask is the fine network's: samples outside every coarse volume but inside a fine one
            fb = N(c["valid_bits_fine"]).reshape(R, S + Sf).astype(np.uint32)
            _, enc = orc_f.forward(o.sample_points(ro, rd, N(c["z_sorted"])), rd, scene["skts"][cam], scene["bones"][cam], cam, 1)
            want = (enc["valid"] * (1 << np.arange(24, dtype=np.uint64))).sum(-1).astype(np.uint32)
            assert np.array_equal(fb, want)
            _, enc_c = orc_c.forward(o.sample_points(ro, rd, N(c["z_sorted"])), rd, scene["skts"][cam], scene["bones"][cam], cam, 1)
            assert int((enc["valid"].any(-1) & ~enc_c["valid"].any(-1)).sum()) > 0


def test_danbo_caster_two_net_whole_image_and_graph_replay():
    from core import trainer
    from core.utils import synthetic as syn
    args, caster, kw, cfg, sds, _ = two_net_caster("h36m_zju/danbo_base.txt", "danbo_base", n_codes=8)
    scene = syn.make_scene(n_poses=1, H=48, W=48, n_views=2, pose_seed=2)
    ro, rd = (T(x) for x in scene["rays"][1])
    n = len(ro)
    exp = lambda x, dt=torch.float32: T(x, dt)[:1].expand(n, *x.shape[1:])  # noqa: E731
    kwargs = dict(kp_batch=exp(scene["kps"]), skts=exp(scene["skts"]), cyls=exp(scene["cyls"]), bones=exp(scene["bones"]),
                  cams=torch.zeros(1, dtype=torch.int64, device=DEV).expand(n), ray_caster=caster, N_samples=24, N_importance=12, **kw)
    whole = trainer.render(48, 48, 80., chunk=1000, rays=(ro, rd), **kwargs)
    orig = caster.render_rays_whole
    caster.render_rays_whole = lambda *a, **k: None
    try:
        caster.use_graphs = False
        loop = trainer.render(48, 48, 80., chunk=1000, rays=(ro, rd), **kwargs)
    finally:
        caster.render_rays_whole = orig
        caster.use_graphs = True
    for k in loop:
        assert torch.equal(whole[k], loop[k]), k
    # small chunks: a captured HIP graph equals the eager chain, and is captured again after either network's weights change
    scene, rb = body_scene(H=24, W=24)
    caster.use_graphs = False
    eager = {k: v.clone() for k, v in cast(caster, kw, scene, rb, 24, 12).items()}
    caster.use_graphs = True
    first = {k: v.clone() for k, v in cast(caster, kw, scene, rb, 24, 12).items()}
    again = cast(caster, kw, scene, rb, 24, 12)
    assert len(caster._graphs.graphs) == 1
    for k in eager:
        assert torch.equal(eager[k], first[k]) and torch.equal(eager[k], again[k]), k
    prev = eager
    for net in (caster.network_fine, caster.network):
        with torch.no_grad():
            net.alpha_linear.bias.add_(0.5)
        caster.use_graphs = False
        want = {k: v.clone() for k, v in cast(caster, kw, scene, rb, 24, 12).items()}
        caster.use_graphs = True
        got = cast(caster, kw, scene, rb, 24, 12)
        assert all(torch.equal(want[k], got[k]) for k in want)
        assert not torch.equal(want["rgb_map"], prev["rgb_map"])
        prev = want


# ----------------------------------------------------------------------------- training
def _train_batch(caster, tr, scene, rb, S, Sf):
    R = len(rb)
    z = np.zeros(R, np.int64)
    kw = {k: v for k, v in tr.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    kw.update(perturb=0., raw_noise_std=0.)
    return caster(T(rb), N_samples=S, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                  bones=T(scene["bones"][z]), cams=T(np.zeros(R), torch.int64), N_importance=Sf, N_uniques=1, **kw)


@pytest.mark.parametrize("cfg_file,cfg_name", [("h36m_zju/anerf_base.txt", "anerf_base"), ("h36m_zju/danbo_base.txt", "danbo_base")])
def test_two_net_autograd_training_step(cfg_file, cfg_name):
    """the fused steps stay single-network ('single_net=False' names the reason): the autograd path trains both networks -- the
    coarse one through rgb_loss0 alone (the sampling is detached), the fine one through the final maps, on all S + Sf samples"""
    from core import anerf_train_engine, train_engine
    args, caster, kw, cfg, sds, tr = two_net_caster(cfg_file, cfg_name, n_codes=8)
    mod = anerf_train_engine if cfg_name == "anerf_base" else train_engine
    assert mod.supported(args, caster) == 'single_net=False'
    scene, rb = body_scene(n=256, H=24, W=24)
    rb = rb[np.random.default_rng(0).permutation(len(rb))[:96]]
    S, Sf = 12, 6
    caster.train()
    try:
        out = _train_batch(caster, tr, scene, rb, S, Sf)
        R = len(rb)
        assert out["alpha"].shape == (R, S + Sf) and out["alpha0"].shape == (R, S)
        target = torch.rand(R, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        loss = ((out["rgb_map"] - target) ** 2).mean()
        loss0 = ((out["rgb0"] - target) ** 2).mean()
        # (A-NeRF's cutoff embedders are one module of both networks, as in the reference: left out of the separation checks)
        shared = {id(p) for p in caster.network.parameters()} & {id(p) for p in caster.network_fine.parameters()}
        net_c = [p for p in caster.network.parameters() if p.requires_grad and id(p) not in shared]
        net_f = [p for p in caster.network_fine.parameters() if p.requires_grad and id(p) not in shared]
        g_c = torch.autograd.grad(loss, net_c, allow_unused=True, retain_graph=True)
        assert all(g is None or not bool(g.any()) for g in g_c)          # no path from the final maps to the coarse network
        g_f0 = torch.autograd.grad(loss0, net_f, allow_unused=True, retain_graph=True)
        assert all(g is None or not bool(g.any()) for g in g_f0)         # nor from the coarse maps to the fine network
        g_c0 = torch.autograd.grad(loss0, net_c, allow_unused=True, retain_graph=True)
        g_f = torch.autograd.grad(loss, net_f, allow_unused=True, retain_graph=True)
        for gs in (g_c0, g_f):
            gs = [g for g in gs if g is not None]
            assert gs and all(bool(torch.isfinite(g).all()) for g in gs) and sum(float(g.abs().sum()) for g in gs) > 0
        if cfg_name == "danbo_base":      # the assignment logits of the loss: the fine pass's, one row per sample of S + Sf
            from core import train_path
            assert out["confd"].shape[:2] == (R, S + Sf) and out["part_invalid"].shape[:2] == (R, S + Sf)
            ssl = train_path.soft_softmax_loss(args, caster.network_fine, out)
            g_sf = torch.autograd.grad(ssl, net_f, allow_unused=True, retain_graph=True)
            assert sum(float(g.abs().sum()) for g in g_sf if g is not None) > 0
            g_sc = torch.autograd.grad(ssl, net_c, allow_unused=True, retain_graph=True)
            assert all(g is None or not bool(g.any()) for g in g_sc)
        # the eval render of the same rays: the same maps (the training forward and the eval kernels agree)
        with torch.no_grad():
            caster.eval()
            ev = cast(caster, kw, scene, rb, S, Sf)
        for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
            assert max_err(N(out[k]), N(ev[k])) < 2e-3, k
    finally:
        caster.eval()


# ----------------------------------------------------------------------------- training against float64
def _f64_two_net(cfg, sd_c, sd_f, rest, batch, z_c, z_all, args, kinks=None):
    """the two-network training step in float64 (oracle/torch_f64_anerf_train's network and composite): the coarse parameters on
    the coarse depths, the fine parameters on the path's sorted depths z_all, both composited as they are; depths and order come
    from the path under test (detached in the reference)"""
    import torch_f64_anerf_train as f64
    dt = f64._dtype()
    Tq = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=dt)  # noqa: E731
    ro, rd = np.asarray(batch["rays_o"], np.float32), np.asarray(batch["rays_d"], np.float32)
    R, G = ro.shape[0], batch["skts"].shape[0]
    skts_ray = np.asarray(batch["skts"], np.float32)[np.arange(R) // (R // G)]
    align = o.bone_align_transforms(rest).astype(np.float32)

    def params(sd):
        names = [k for k, v in sd.items() if np.asarray(v).dtype.kind == "f" and not k.endswith(".tau") and "cutoff_dist" not in k]
        p = {k: Tq(sd[k]).requires_grad_(True) for k in names}
        p["pe_fn.cutoff_dist"], p["dirs_pe_fn.cutoff_dist"] = Tq(sd["pe_fn.cutoff_dist"]), Tq(sd["dirs_pe_fn.cutoff_dist"])
        return p

    p_c, p_f = params(sd_c), params(sd_f)

    def pass_(p, z):
        pt = o.bone_local(o.sample_points(ro, rd, np.asarray(z, np.float32)), skts_ray, align)
        return f64.network(cfg, p, Tq(pt), Tq(rd), Tq(skts_ray), batch["cam_idx"], float(args["tau"]), kinks)

    B = float(args["density_scale"])
    out0 = f64.composite(pass_(p_c, z_c), Tq(z_c), Tq(rd), B)
    out = f64.composite(pass_(p_f, z_all), Tq(z_all), Tq(rd), B)
    target, bgs = Tq(batch["target"]), Tq(batch["bgs"])

    def nerf_loss(rgb, acc, w):
        if args["use_background"]:
            rgb = rgb + (1.0 - acc)[..., None] * bgs
        d = rgb - target
        return (d.abs().mean() if args["loss_fn"] == "L1" else (d * d).mean()) * w * float(args["rgb_loss_coef"])
    loss = {"rgb_loss": nerf_loss(out["rgb_map"], out["acc_map"], 1.0),
            "rgb_loss0": nerf_loss(out0["rgb_map"], out0["acc_map"], float(args["coarse_weight"]))}
    (loss["rgb_loss"] + loss["rgb_loss0"]).backward()
    grads = {}
    for tag, p in (("c", p_c), ("f", p_f)):
        for k, v in p.items():
            if v.requires_grad:
                grads[(tag, k)] = v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(v.shape)
    return dict(loss={k: float(v.detach()) for k, v in loss.items()}, grads=grads, rgb_map=out["rgb_map"].detach().numpy(),
                rgb0=out0["rgb_map"].detach().numpy())


def _f64_two_net_bracketed(*a):
    """_f64_two_net + the bracket of the ReLU-kink decisions fp32 does not determine (as torch_f64_anerf_train.step_bracketed)"""
    import torch_f64_anerf_train as f64
    import torch_f64_train as t64
    from torch_f64_train import Kinks
    k32, k64 = Kinks(), Kinks()
    t64.F64 = torch.float32
    try:
        _f64_two_net(*a, kinks=k32)
    finally:
        t64.F64 = torch.float64
    ret = _f64_two_net(*a, kinks=k64)
    masks = [((x.to(torch.float64) > 0) != (y > 0)) | (y.abs() < Kinks.KAPPA * (y - x.to(torch.float64)).abs()) for x, y in zip(k32.z, k64.z)]
    g_on = _f64_two_net(*a, kinks=Kinks(masks, 1))["grads"]
    g_off = _f64_two_net(*a, kinks=Kinks(masks, 0))["grads"]
    ret["bracket"] = {n: float(np.abs(g_on[n] - g_off[n]).max()) for n in g_on}
    assert f64 is not None
    return ret


@pytest.mark.parametrize("loss_fn", ["L1", "MSE"])
def test_anerf_two_net_autograd_step_matches_float64(loss_fn):
    """the autograd path of a two-network A-NeRF caster on the reference's training batch (anerf_train: 96 rays = 4 poses x 24,
    12 + 6 samples, perturb = 0, noise = 0): both losses and every gradient of BOTH networks against the float64 arbiter at the
    path's own depths -- the bounds of test_fused_anerf_step_matches_the_reference_and_float64 (kink bracket + 2e-4 of the max)"""
    from core import hip_ops as ops
    from core import train_path
    from core.utils import synthetic as syn
    from helpers import golden
    g = golden("anerf_train")
    S, Sf = int(g["N_samples"]), int(g["N_importance"])
    args, caster, kw, cfg, sds, tr = two_net_caster("h36m_zju/anerf_base.txt", "anerf_base", seeds=(int(g["weight_seed"]), 17),
                                                    n_codes=int(g["n_framecodes"]))
    args.loss_fn = loss_fn
    # the cutoff embedders are one module of both networks (as in the reference): one set of their entries
    for k in ("pe_fn.cutoff_dist", "dirs_pe_fn.cutoff_dist", "pe_fn.tau", "dirs_pe_fn.tau"):
        sds[1][k] = sds[0][k]
    caster.network_fine.load_state_dict({k: torch.tensor(v) for k, v in sds[1].items()}, strict=True)
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sds[0].items()}, strict=True)
    tau = float(caster.network.pe_fn.tau)
    pose, rb = g["pose_of_ray"], g["ray_batch"]
    seen = {}
    orig = ops.importance_samples

    def spy(z, w, Sf_, u=None, flat=None, two_net=False):
        res = orig(z, w, Sf_, u, flat=flat, two_net=two_net)
        seen.update(z=z.detach().cpu().numpy(), z_all=res[0].cpu().numpy(), two_net=two_net)
        return res
    ops.importance_samples = spy
    caster.train()
    try:
        kwt = {k: v for k, v in tr.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
        kwt.update(perturb=0., raw_noise_std=0.)
        out = caster(T(rb), N_samples=S, kp_batch=T(g["kps"][pose]), skts=T(g["skts"][pose]), cyls=T(g["cyls"][pose]),
                     bones=T(g["bones"][pose]), cams=T(g["cam_idx"], torch.int64), N_importance=Sf, N_uniques=int(g["n_uniques"]), **kwt)
        target, bgs = T(g["target"]), T(g["bgs"])
        loss = train_path.nerf_loss(args, out["rgb_map"], out["acc_map"], target, bgs)
        loss0 = train_path.nerf_loss(args, out["rgb0"], out["acc0"], target, bgs, loss_weight=args.coarse_weight)
        for p in caster.parameters():
            p.grad = None
        (loss + loss0).backward()
    finally:
        ops.importance_samples = orig
        caster.eval()
    assert seen["two_net"] and seen["z_all"].shape == (96, S + Sf)
    grads = {}
    for tag, net in (("c", caster.network), ("f", caster.network_fine)):
        for n, p in net.named_parameters():
            if p.requires_grad and "cutoff_dist" not in n:
                grads[(tag, n)] = N(p.grad).astype(np.float64) if p.grad is not None else np.zeros(tuple(p.shape))
    batch = dict(rays_o=rb[:, 0:3], rays_d=rb[:, 3:6], skts=g["skts"], cam_idx=g["cam_idx"], target=g["target"], bgs=g["bgs"])
    a = dict(loss_fn=loss_fn, use_background=bool(args.use_background), rgb_loss_coef=float(args.rgb_loss_coef),
             coarse_weight=float(args.coarse_weight), density_scale=float(args.density_scale), tau=tau)
    ref = _f64_two_net_bracketed(cfg, sds[0], sds[1], syn.rest_pose(0.48), batch, seen["z"], seen["z_all"], a)
    for got, k in ((float(loss), "rgb_loss"), (float(loss0), "rgb_loss0")):
        assert abs(got - ref["loss"][k]) <= 2e-5 * abs(ref["loss"][k]), (k, got, ref["loss"][k])
    assert np.abs(N(out["rgb_map"]) - ref["rgb_map"]).max() < 2e-5 and np.abs(N(out["rgb0"]) - ref["rgb0"]).max() < 2e-5
    assert set(ref["grads"]) == set(grads)
    worst, nonzero = 0.0, {"c": 0, "f": 0}
    for n, r in ref["grads"].items():
        if not np.abs(r).max() > 0:
            assert not np.abs(grads[n]).max() > 0, n
            continue
        nonzero[n[0]] += 1
        e = np.abs(grads[n] - r).max()
        worst = max(worst, (e - ref["bracket"][n]) / np.abs(r).max())
        assert e <= 2e-4 * np.abs(r).max() + ref["bracket"][n], (n, e, np.abs(r).max(), ref["bracket"][n])
    assert nonzero["c"] > 10 and nonzero["f"] > 10
    print("two-network A-NeRF autograd step vs float64 (%s): worst (error - bracket) / max = %.2e" % (loss_fn, worst))


# ----------------------------------------------------------------------------- entry points
def test_two_net_train_checkpoint_render_round_trip(tmp_path):
    """run_nerf.train on a two-network A-NeRF config (single_net off: a config file without it -- a store_true flag has no argv
    spelling that switches it off) writes a checkpoint with two distinct state dicts in the reference's layout; tau of both networks
    follows the schedule; run_render loads both networks from it and renders images equal to the trained caster's on the same rays"""
    import run_nerf
    import run_render
    src = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt")
    lines = [l for l in open(src) if not l.startswith(("single_net", "N_samples", "N_importance"))]
    cfg_path = tmp_path / "anerf_two_net.txt"
    cfg_path.write_text("".join(lines) + "N_samples = 16\nN_importance = 8\n")
    # start from seeded, lively weights (a fresh A-NeRF renders empty images): a two-network checkpoint of the reference's layout,
    # loaded through --ft_path -- the load path of both networks on the way in
    from core.utils import synthetic as syn
    mcfg = syn.model_config("anerf_base")
    sd_c, sd_f = (syn.make_state_dict(mcfg, seed=s, n_framecodes=4, rest=syn.rest_pose(0.48)) for s in (3, 4))
    for k in ("pe_fn.cutoff_dist", "dirs_pe_fn.cutoff_dist", "pe_fn.tau", "dirs_pe_fn.tau"):
        sd_f[k] = sd_c[k]
    init = tmp_path / "init.tar"
    torch.save({"global_step": 0, "network_fn_state_dict": {k: torch.tensor(v) for k, v in sd_c.items()},
                "network_fine_state_dict": {k: torch.tensor(v) for k, v in sd_f.items()}}, init)
    common = ["--config", str(cfg_path), "--basedir", str(tmp_path), "--expname", "two", "--syn_poses", "2", "--syn_cams", "2",
              "--syn_res", "32", "--N_rand", "256", "--N_sample_images", "2", "--i_print", "10", "--i_weights", "12",
              "--i_testset", "1000", "--render_factor", "0", "--ft_path", str(init)]
    trainer = run_nerf.train(common + ["--n_iters", "12"])
    caster = trainer.render_kwargs_train["ray_caster"]
    assert caster.two_net and not trainer.args.single_net
    assert trainer.fused_engine() is None and trainer.fused_reason == "single_net=False"
    log = tmp_path / "two"
    ckpt = torch.load(log / "000012.tar", map_location="cpu")
    a, b = ckpt["network_fn_state_dict"], ckpt["network_fine_state_dict"]
    assert set(a) == set(b) and not torch.equal(a["pts_linears.0.weight"], b["pts_linears.0.weight"])
    for key, net in (("network_fn_state_dict", caster.network), ("network_fine_state_dict", caster.network_fine)):
        for k, v in net.state_dict().items():
            assert torch.equal(ckpt[key][k].cpu(), v.cpu()), (key, k)
    # tau = 20 * rate^(global_step / (cutoff_step * 1000)), in both networks and in both state dicts
    want = 20.0 * trainer.args.cutoff_rate ** (ckpt["global_step"] / float(trainer.args.cutoff_step * 1000))
    assert ckpt["global_step"] > 0 and want > 20.0 * (1 + 1e-5)
    for net, sd in ((caster.network, a), (caster.network_fine, b)):
        for m in ("pe_fn", "dirs_pe_fn"):
            assert abs(float(getattr(net, m).tau) - want) <= 1e-6 * want and abs(float(sd[m + ".tau"]) - want) <= 1e-6 * want
    # run_render: the loaded caster holds both dicts, and its images are the trained caster's on the same rays
    loaded, calls = {}, []
    orig_load, orig_path = run_render.load_nerf, run_render.render_path

    def load(*x, **k):
        r = orig_load(*x, **k)
        loaded["kw"] = r[0]
        return r

    def path(**k):
        calls.append(k)
        return orig_path(**k)
    run_render.load_nerf, run_render.render_path = load, path
    try:
        rgbs, accs, _, _ = run_render.run_render(["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000012.tar"),
                                                  "--dataset", "synthetic", "--entry", "val", "--outputdir", str(tmp_path / "out"),
                                                  "--render_type", "bullet", "--n_bullet", "2", "--selected_idxs", "0", "--runname", "bt",
                                                  "--render_res", "32", "32", "--no_save"])
    finally:
        run_render.load_nerf, run_render.render_path = orig_load, orig_path
    rc = loaded["kw"]["ray_caster"]
    assert rc.two_net
    for key, net in (("network_fn_state_dict", rc.network), ("network_fine_state_dict", rc.network_fine)):
        for k, v in net.state_dict().items():
            assert torch.equal(ckpt[key][k].cpu(), v.cpu()), (key, k)
    assert rgbs.shape == (2, 32, 32, 3) and np.isfinite(rgbs).all() and np.isfinite(accs).all()
    k = dict(calls[0])
    k["render_kwargs"] = dict(k["render_kwargs"], ray_caster=caster.eval())
    again = orig_path(**k)[0]
    assert np.array_equal(again, rgbs)
