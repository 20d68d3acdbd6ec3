"""Softplus density (density_type = softplus) on the GPU: the composite kernels' softplus instantiations against the numpy
restatement of tests/test_softplus_oracle.py and float64, the fused forms against the separate kernels, the engines' renders with
no rays of constants, the caster's graph cache, the composite's backward and the autograd training path."""
import os

import numpy as np
import pytest
import torch

import danbo_oracle as o
from helpers import ROOT, max_err, raw_err, N
from test_softplus_oracle import check_composite, composite, regime_rays, regime_shares, render_composed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPS = ("rgb_map", "disp_map", "acc_map", "alpha", "T_i", "rgb0", "disp0", "acc0", "alpha0")


def T(x, dtype=torch.float32):
    return None if x is None else torch.tensor(np.ascontiguousarray(x), dtype=dtype, device=DEV)


def SP(shift):
    return ("softplus", float(shift))


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("S", [7, 48, 144])
@pytest.mark.parametrize("with_noise", [False, True])
def test_softplus_composite_against_the_restatement_and_float64(S, with_noise):
    """k_composite<DENSITY_SOFTPLUS> (S = 144: three chunks of the scan) on rays that cover t > 20, |t| small and t < -15, a third
    of them thin (density logits around -6: transmittance stays high deep into the ray), with lazily filled raw, and with logits of
    +-1e4 / +-1e30 -- the bounds of test_gpu_kernels.py::test_composite_long_rays_and_noise"""
    from core import hip_ops as ops
    for shift, B in ((1.0, 1.0), (0.25, 0.5)):
        raw, z, rays_d, noise = regime_rays(S + int(with_noise), 300, S, shift, with_noise, B, with_extremes=True)
        hi, mid, lo = regime_shares(raw[2:], None if noise is None else noise[2:], shift, B)
        assert hi >= 0.05 and mid >= 0.05 and lo >= 0.05, (hi, mid, lo)
        got = {k: N(v) for k, v in ops.composite(T(raw), T(z), T(rays_d), B, T(noise), act=SP(shift)).items()}
        assert all(np.all(np.isfinite(v)) for v in got.values())
        ref = composite(raw, z, rays_d, B, noise, act=shift)
        ref64 = composite(raw, z, rays_d, B, noise, act=shift, dtype=np.float64)
        for k in ("rgb_map", "acc_map", "weights", "alpha"):
            print("softplus composite S=%d noise=%d shift=%.2f %s: vs f32 %.2e, vs f64 %.2e" % (S, with_noise, shift, k, max_err(got[k], ref[k]),
                                                                                           max_err(got[k], ref64[k])))
        check_composite(got, ref, (S, with_noise, shift))
        check_composite(got, ref64, (S, with_noise, shift, "f64"))
        thin = np.arange(len(raw)) % 3 == 2
        assert float(np.median(1. - ref64["weights"][thin][:, :S // 2].sum(-1))) > 0.3      # T well above 0 half way into a thin ray
        assert max_err(got["rgb_map"], N(ops.composite(T(raw), T(z), T(rays_d), B, T(noise))["rgb_map"])) > 1e-3      # not relu
        # rows whose in-volume word is 0 were never written: they take the ray's empty-space raw and contribute density
        rng = np.random.default_rng(S)
        bits = (rng.integers(0, 2, size=raw.shape[:2]) * rng.integers(1, 1 << 24, size=raw.shape[:2])).astype(np.int32)
        empty = rng.normal(size=(len(raw), 4)).astype(np.float32)
        empty[:, 3] = ((rng.normal(size=len(raw)) - 2. + shift) * B).astype(np.float32)
        filled = np.where((bits != 0)[..., None], raw, empty[:, None, :]).astype(np.float32)
        junk = np.where((bits != 0)[..., None], raw, np.float32("nan")).astype(np.float32)
        a = ops.composite(T(filled), T(z), T(rays_d), B, T(noise), act=SP(shift))
        b = ops.composite(T(junk), T(z), T(rays_d), B, T(noise), bits=T(bits, torch.int32), raw_empty=T(empty), act=SP(shift))
        assert all(torch.equal(a[k], b[k]) for k in a)
        check_composite({k: N(v) for k, v in b.items()}, composite(filled, z, rays_d, B, noise, act=shift), (S, "lazy"))


@pytest.mark.parametrize("S,Sf", [(48, 16), (64, 64), (96, 32), (200, 64)])
def test_fused_softplus_forms_equal_the_separate_kernels(S, Sf):
    """under softplus: composite_importance == composite + importance_samples (both pdfs; S, Sf <= 64), composite_merged == merge +
    composite, lazily filled raw (NaN rows + bits + raw_empty) == pre-filled raw -- bit for bit"""
    from core import hip_ops as ops
    rng = np.random.default_rng(S * 100 + Sf)
    R, B, act = 777, 0.8, SP(0.5)
    raw, raw_f = T(rng.normal(0, 2.0, size=(R, S, 4))), T(rng.normal(0, 2.0, size=(R, Sf, 4)))
    z = T(rng.uniform(1, 3, size=(R, 1)) + np.sort(rng.uniform(0, 2, size=(R, S)), -1))
    d = T(rng.normal(size=(R, 3)))
    bits = T(rng.integers(0, 2, size=(R, S)) * rng.integers(1, 1 << 24, size=(R, S)), torch.int32)
    bits[::5] = 0                              # rays without a single in-volume coarse sample
    bits_f = T(rng.integers(0, 2, size=(R, Sf)) * 5, torch.int32)
    bits_f[::5] = 0
    empty = T(rng.normal(size=(R, 4)) - np.array([0, 0, 0, 1.5]))       # empty-space density logit mostly negative
    filled = torch.where((bits != 0)[..., None], raw, empty[:, None, :].expand(R, S, 4)).contiguous()
    filled_f = torch.where((bits_f != 0)[..., None], raw_f, empty[:, None, :].expand(R, Sf, 4)).contiguous()
    junk = torch.where((bits != 0)[..., None], raw, torch.full_like(raw, float("nan")))
    junk_f = torch.where((bits_f != 0)[..., None], raw_f, torch.full_like(raw_f, float("nan")))
    for rand_u in (False, True):
        u = T(rng.uniform(size=(R, Sf))) if rand_u else None
        noise = T(rng.normal(0, 0.2, size=(R, S))) if rand_u else None
        a = ops.composite(filled, z, d, B, noise, act=act)
        lazy = ops.composite(junk, z, d, B, noise, bits=bits, raw_empty=empty, act=act)
        assert all(torch.equal(a[k], lazy[k]) for k in a)
        assert not torch.equal(a["acc_map"], ops.composite(filled, z, d, B, noise)["acc_map"])
        assert float(a["acc_map"][::5].min()) > 0.          # a ray of nothing but empty space has density under softplus
        for two in (False, True):
            z_all, z_fine, order = ops.importance_samples(z, a["weights"], Sf, u, two_net=two)
            if S <= 64 and Sf <= 64:
                for rw, kw in ((filled, {}), (junk, dict(bits=bits, raw_empty=empty))):
                    b, z_all2, z_fine2, order2 = ops.composite_importance(rw, z, d, Sf, B, noise, u, two_net=two, act=act, **kw)
                    for k in a:
                        assert torch.equal(a[k], b[k]), (k, two)
                    assert torch.equal(z_all, z_all2) and torch.equal(z_fine, z_fine2) and torch.equal(order, order2)
        z_all, z_fine, order = ops.importance_samples(z, a["weights"], Sf, u)
        merged = ops.merge_samples(filled, filled_f, order)
        c = ops.composite(merged, z_all, d, B, act=act)
        e = ops.composite_merged(filled, filled_f, order, z_all, d, B, want_raw=True, act=act)
        g = ops.composite_merged(junk, junk_f, order, z_all, d, B, bits_a=bits, bits_b=bits_f, raw_empty=empty, act=act)
        for k in c:
            assert torch.equal(c[k], e[k]) and torch.equal(c[k], g[k]), k
        assert torch.equal(e["raw_sorted"], merged)
    with pytest.raises(AssertionError):        # a list of the rays that are NOT rays of constants cannot exist under softplus
        ops.composite(filled, z, d, B, flat=dict(out0=None), act=act)


# ----------------------------------------------------------------------------- engines
def _danbo_engine(seed=1, n_codes=8):
    from core.render_engine import DanboEngine
    from core.utils import synthetic as syn
    cfg = syn.model_config("danbo_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd = syn.make_state_dict(cfg, seed=seed, n_framecodes=n_codes, rest=rest)
    orc = o.DanboOracle(cfg, sd, rest)
    return DanboEngine(dict(cfg), {k: T(v) for k, v in sd.items()}, T(orc.align)), orc, cfg


@pytest.mark.parametrize("S,Sf", [(24, 12), (96, 32)])
def test_no_rays_of_constants_under_softplus(S, Sf):
    """The trap: a model whose empty-space density logit is negative and whose _flat_rays_ok() holds, a frame in which many rays
    miss every volume.  Under relu those rays are rays of constants (acc exactly 0); under softplus they have density on every
    sample: lazy, keep, dense and the C entry agree bit for bit, agree with the composed oracle, and switching back to relu gives
    relu's bits again."""
    from core import hip_ops as ops
    from core.utils import synthetic as syn
    eng, orc, cfg = _danbo_engine()
    eng.refresh()
    assert eng.flat_rays_ok and float(eng.empty_consts[128]) / float(cfg["density_scale"]) < 0
    scene = syn.make_scene(n_poses=1, H=48, W=48, n_views=1, pose_seed=4)
    ro, rd = scene["rays"][0]
    R = len(ro)
    cam = np.zeros(R, np.int64)
    args = (T(ro), T(rd), T(scene["skts"]), T(scene["bones"]), T(scene["cyls"]), T(cam, torch.int64))
    relu = {k: v.clone() for k, v in eng.render(*args, S, Sf).items()}
    near, far = eng.near_far(*args[:2], args[4], args[2])
    missed = ops.ray_bone_mask(args[0], args[1], args[2], eng.align, eng.axis_scale, near, far, want_flat=True)[3] != 0
    assert float(missed.float().mean()) > 0.30
    assert float(relu["acc_map"][missed].abs().max()) == 0.0 and float(relu["alpha"][missed].abs().max()) == 0.0
    for shift in (1.0, 0.25):
        eng.cfg["density_act"] = SP(shift)
        try:
            a = {k: v.clone() for k, v in eng.render(*args, S, Sf).items()}
            b = eng.render(*args, S, Sf, dense=True)
            c = eng.render(*args, S, Sf, keep=True)
            f = eng.render_frame_c(*args, S, Sf)
        finally:
            eng.cfg["density_act"] = ops.RELU
        for k in MAPS:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], f[k]), (shift, k)
        assert float(a["acc_map"][missed].min()) > 0. and float(a["acc0"][missed].min()) > 0.
        assert float(a["rgb_map"][missed].abs().sum(-1).min()) > 0.           # the empty-space colour, not zeros
        nf = (N(c["near"]).reshape(-1, 1), N(c["far"]).reshape(-1, 1))
        ref = render_composed(orc, None, syn.ray_batch(ro, rd), scene["skts"][cam], scene["bones"][cam], scene["cyls"][cam], cam, 1,
                              S, Sf, act=shift, near_far=nf)
        print("softplus render S=%d shift=%.2f: %s psnr %.1f" % (S, shift, {k: "%.2e" % max_err(N(a[k]), ref[k]) for k in
                                                                          ("rgb_map", "acc_map", "rgb0", "acc0")}, o.psnr(N(a["rgb_map"]), ref["rgb_map"])))
        for k in ("rgb0", "acc0"):             # tests/test_gpu_two_net.py:208-211
            assert max_err(N(a[k]), ref[k]) < 1e-5, (S, k)
        for k in ("rgb_map", "acc_map"):
            assert max_err(N(a[k]), ref[k]) < 5e-4, (S, k)
        assert o.psnr(N(a["rgb_map"]), ref["rgb_map"]) > 100.0
        assert max_err(N(a["rgb_map"]), N(relu["rgb_map"])) > 1e-2
    again = eng.render(*args, S, Sf)
    for k in MAPS:
        assert torch.equal(again[k], relu[k]), k
    f = eng.render_frame_c(*args, S, Sf)
    assert all(torch.equal(f[k], relu[k]) for k in MAPS)


def softplus_caster(cfg_file, cfg_name, shift, two_net, seeds=(3, 4), n_codes=8, extra=()):
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload", "--density_type", "softplus", "--softplus_shift", str(shift), *extra],
                      config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", cfg_file))
    if two_net:
        args.single_net = False
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    tr, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    assert caster.two_net == bool(two_net)
    cfg = syn.model_config(cfg_name)
    sds = [syn.make_state_dict(cfg, seed=s, n_framecodes=n_codes, rest=syn.rest_pose(0.48)) for s in seeds]
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sds[0].items()}, strict=True)
    if two_net:
        caster.network_fine.load_state_dict({k: torch.tensor(v) for k, v in sds[1].items()}, strict=True)
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    cls = o.DanboOracle if cfg["nerf_type"] == "danbo" else o.AnerfOracle
    orcs = [cls(cfg, sd, syn.rest_pose(0.48)) for sd in sds]
    return args, caster, kw, orcs, tr


def cast(caster, kw, scene, rb, S, Sf, cams=None):
    R = len(rb)
    z = np.zeros(R, np.int64)
    cams = np.zeros(R, np.int64) if cams is None else cams
    return caster(T(rb), N_samples=S, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                  bones=T(scene["bones"][z]), cams=T(cams, torch.int64), N_importance=Sf, N_uniques=1, **kw)


def body_scene(H=24, W=24, seed=3):
    from core.utils import synthetic as syn
    scene = syn.make_scene(n_poses=1, H=H, W=W, n_views=1, pose_seed=seed)
    ro, rd = scene["rays"][0]
    return scene, syn.ray_batch(ro, rd)


@pytest.mark.parametrize("cfg_file,cfg_name,two_net", [("h36m_zju/anerf_base.txt", "anerf_base", False),
                                                       ("h36m_zju/anerf_base.txt", "anerf_base", True),
                                                       ("h36m_zju/danbo_base.txt", "danbo_base", True)])
def test_softplus_renders_against_the_composed_oracle(cfg_file, cfg_name, two_net):
    """the A-NeRF engine and both two-network renders through the caster (density_type = softplus, shift 0.5) against the oracle's
    stages + the restated composite: the bounds of tests/test_gpu_two_net.py:136-137 (A-NeRF) / :208-211 (DANBO)"""
    args, caster, kw, orcs, _ = softplus_caster(cfg_file, cfg_name, 0.5, two_net)
    scene, rb = body_scene()
    R = len(rb)
    z = np.zeros(R, np.int64)
    cams = -np.ones(R, np.int64) if cfg_name == "anerf_base" else np.zeros(R, np.int64)
    caster.use_graphs = False
    out = cast(caster, kw, scene, rb, 16, 8, cams)
    ref = render_composed(orcs[0], orcs[1] if two_net else None, rb, scene["skts"][z], scene["bones"][z], scene["cyls"][z], cams, 1, 16, 8,
                          act=0.5)
    print("softplus %s two_net=%s: %s psnr %.1f" % (cfg_name, two_net, {k: "%.2e" % max_err(N(out[k]), ref[k]) for k in
                                                                      ("rgb_map", "acc_map", "rgb0", "acc0")}, o.psnr(N(out["rgb_map"]), ref["rgb_map"])))
    if cfg_name == "anerf_base":
        for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
            assert max_err(N(out[k]), ref[k]) < 5e-5, k
        assert o.psnr(N(out["rgb_map"]), ref["rgb_map"]) > 90.0
    else:
        for k in ("rgb0", "acc0"):
            assert max_err(N(out[k]), ref[k]) < 1e-5, k
        for k in ("rgb_map", "acc_map"):
            assert max_err(N(out[k]), ref[k]) < 5e-4, k
        assert o.psnr(N(out["rgb_map"]), ref["rgb_map"]) > 100.0
    relu = render_composed(orcs[0], orcs[1] if two_net else None, rb, scene["skts"][z], scene["bones"][z], scene["cyls"][z], cams, 1, 16,
                           8, act=None)
    assert max_err(N(out["rgb_map"]), relu["rgb_map"]) > 1e-2


def test_caster_graph_cache_is_keyed_on_the_activation_and_whole_image_equals_the_chunk_loop():
    import torch.nn.functional as F
    from core import trainer
    from core.raycasters import SoftplusDensity
    from core.utils import synthetic as syn
    args, caster, kw, orcs, _ = softplus_caster("h36m_zju/danbo_base.txt", "danbo_base", 1.0, False)
    assert isinstance(kw["preproc_kwargs"]["density_fn"], SoftplusDensity)
    scene = syn.make_scene(n_poses=1, H=32, W=32, n_views=1, pose_seed=3)
    ro, rd = scene["rays"][0]
    rb = syn.ray_batch(ro, rd)[256:768]                          # a 512-ray chunk: the graph path
    kws = {"softplus": kw, "relu": dict(kw, preproc_kwargs=dict(kw["preproc_kwargs"], density_fn=F.relu)),
           "softplus 0.25": dict(kw, preproc_kwargs=dict(kw["preproc_kwargs"], density_fn=SoftplusDensity(0.25)))}
    caster.use_graphs = False
    eager = {n: {k: v.clone() for k, v in cast(caster, k_, scene, rb, 24, 12).items()} for n, k_ in kws.items()}
    caster.use_graphs = True
    assert max_err(N(eager["softplus"]["rgb_map"]), N(eager["relu"]["rgb_map"])) > 1e-2
    assert max_err(N(eager["softplus"]["alpha"]), N(eager["softplus 0.25"]["alpha"])) > 1e-2
    for n in ("softplus", "softplus", "relu", "softplus", "softplus 0.25", "relu"):
        got = cast(caster, kws[n], scene, rb, 24, 12)
        for k in eager[n]:
            assert torch.equal(got[k], eager[n][k]), (n, k)
    assert len(caster._graphs.graphs) == 3
    # the whole-image cast == the loop over chunks
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
    assert float(whole["acc_map"].min()) > 0.


# ----------------------------------------------------------------------------- backward
def _f64_d_raw(raw, z, rays_d, B, noise, g_rgb, g_acc, shift, below_one):
    """d raw of sum(g_rgb * rgb_map) + sum(g_acc * acc_map) by float64 torch autograd of the restated composite (shift None: relu).
    below_one [R] bool: the branch of acc = min(sum w, 1) the kernel took per ray (oracle/torch_f64_train.py:149-162: `clamped`)"""
    D = torch.float64
    t = lambda x: torch.tensor(np.asarray(x), dtype=D)  # noqa: E731
    raw = t(raw).requires_grad_(True)
    z, d = t(z), t(rays_d)
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(d, dim=-1, keepdim=True)
    rgb = torch.sigmoid(raw[..., :3]) * 1.002 - 0.001
    x = raw[..., 3] / B
    if noise is not None:
        x = x + t(noise)
    sig = torch.relu(x) if shift is None else torch.nn.functional.softplus(x - shift, beta=1)
    alpha = 1. - torch.exp(-sig * dist)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    sw = w.sum(-1)
    acc = torch.where(torch.tensor(below_one), sw, torch.ones_like(sw))
    (((w[..., None] * rgb).sum(-2) * t(g_rgb)).sum() + (acc * t(g_acc)).sum()).backward()
    return raw.grad.numpy()


@pytest.mark.parametrize("S", [48, 144])
@pytest.mark.parametrize("upstream", ["rgb", "rgb+acc"])
def test_softplus_composite_backward_against_float64(S, upstream):
    """torch.ops.danbo.composite with softplus: d_raw for upstream gradients on rgb_map (and acc_map) against float64 autograd of
    the restated composite, error relative to the tensor's max.  The bound is 4 x what the relu kernel shows against float64 relu
    autograd on the same inputs, measured in the same test run (softplus has no kink: it should sit at or below relu's figure).
    sum w of nearly every softplus ray is 1 up to rounding, ON the kink of acc = min(sum w, 1): the float64 side takes the branch
    the FORWARD kernel took (acc_map < 1 of the forward under test).  The backward kernel decides from its own sum of weights
    (log-domain transmittance under softplus), which may fall on the other side for such a ray; the term the two branches differ
    by is at most |g_acc| x 2e-6 there (csrc/composite_bwd.hpp).  The rgb-only case does not depend on any of it.
    Measured on the MI355X (gradient_entry_rel_to_max, rgb and rgb + acc alike): S = 48: relu 1.79e-7, softplus 1.55e-7; S = 144: relu
    1.55e-7, softplus 2.37e-7.  (With the transmittance as a product of S rounded factors, as relu has it, softplus stood at
    1.26e-6 for S = 144 -- and so did fp32 torch autograd on the GPU, 1.32e-6: DESIGN.md 7c; it is taken in the log domain.)"""
    from core import train_path
    rng = np.random.default_rng(S)
    shift, B = 0.5, 0.7
    raw, z, rays_d, noise = regime_rays(S, 120, S, shift, True, B, with_extremes=True)
    g_rgb = rng.normal(size=(len(raw), 3)).astype(np.float32)
    g_acc = rng.normal(size=len(raw)).astype(np.float32) if upstream == "rgb+acc" else np.zeros(len(raw), np.float32)
    figs = {}
    for name, act, sh in (("relu", None, None), ("softplus", SP(shift), shift)):
        r = T(raw).requires_grad_(True)
        out = train_path.composite(r, T(z), T(rays_d), B, T(noise), act)
        ((out["rgb_map"] * T(g_rgb)).sum() + (out["acc_map"] * T(g_acc)).sum()).backward()
        ours = N(r.grad).astype(np.float64)
        assert np.all(np.isfinite(ours)), name
        ref = _f64_d_raw(raw, z, rays_d, B, noise, g_rgb, g_acc, sh, N(out["acc_map"]) < 1.0)
        figs[name] = float(np.abs(ours - ref).max() / np.abs(ref).max())
    print("composite backward S=%d upstream=%s: gradient_entry_rel_to_max relu %.3e softplus %.3e" % (S, upstream, figs["relu"],
                                                                                                   figs["softplus"]))
    assert figs["relu"] < 4e-7, figs           # the yardstick itself: 2 x what the relu kernel measured (1.8e-7)
    assert figs["softplus"] <= 4. * figs["relu"], figs


def test_softplus_composite_custom_op_opcheck_and_lazy_backward():
    import ctypes
    from core import _hip, custom_ops, hip_ops as ops  # noqa: F401
    rng = np.random.default_rng(3)
    raw, z, rays_d, noise = regime_rays(5, 64, 80, 0.5, True, 0.7)
    r = T(raw).requires_grad_(True)
    args = (r, T(z), T(rays_d), 0.7, T(noise), "softplus", 0.5)
    torch.library.opcheck(torch.ops.danbo.composite.default, args, test_utils=("test_schema", "test_faketensor"))
    g_rgb, g_acc = T(rng.normal(size=(64, 3))), T(rng.normal(size=64))
    torch.library.opcheck(torch.ops.danbo.composite_bwd.default, (T(raw), T(z), T(rays_d), 0.7, T(noise), g_rgb, g_acc, "softplus", 0.5),
                          test_utils=("test_schema", "test_faketensor"))
    # danbo_composite_bwd_lazy_act: un-filled raw (NaN rows + bits + raw_empty) == filled raw, bit for bit, and == the custom op
    bits = T(rng.integers(0, 2, size=(64, 80)) * 7, torch.int32)
    empty = T(rng.normal(size=(64, 4)))
    filled = torch.where((bits != 0)[..., None], T(raw), empty[:, None, :].expand(64, 80, 4)).contiguous()
    junk = torch.where((bits != 0)[..., None], T(raw), torch.full_like(T(raw), float("nan"))).contiguous()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    zt, dt, nt = T(z), T(rays_d), T(noise)
    res = []
    for rw, b, e in ((filled, None, None), (junk, bits, empty)):
        d_raw = torch.empty(64, 80, 4, device=DEV)
        _hip.check(_hip.lib().danbo_composite_bwd_lazy_act(p(rw), p(e), p(b), p(zt), p(dt), 64, 80, 0.7, p(nt), p(g_rgb), p(g_acc), p(d_raw),
                                                           1, 0.5, ops._stream()), "danbo_composite_bwd_lazy_act")
        res.append(d_raw)
    assert torch.equal(res[0], res[1]) and bool(torch.isfinite(res[0]).all())
    assert torch.equal(res[0], torch.ops.danbo.composite_bwd(filled, zt, dt, 0.7, nt, g_rgb, g_acc, "softplus", 0.5))
    assert not torch.equal(res[0], torch.ops.danbo.composite_bwd(filled, zt, dt, 0.7, nt, g_rgb, g_acc))


# ----------------------------------------------------------------------------- training on the autograd path
def _trainer(cfg_file, cfg_name, extra=(), n_codes=8, seed=3):
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.trainer import Trainer
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload", "--density_type", "softplus", "--softplus_shift", "0.5", "--N_samples", "12", "--N_importance", "6",
                       *extra], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", cfg_file))
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    tr_kw, te_kw, start, grad_vars, opt, _ = create_raycaster(args, da, device=DEV)
    caster = tr_kw["ray_caster"]
    sd = syn.make_state_dict(syn.model_config(cfg_name), seed, n_codes, syn.rest_pose(0.48))
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    return args, caster, Trainer(args, da, opt, None, tr_kw, te_kw, device=DEV), opt


@pytest.mark.parametrize("cfg_file,cfg_name", [("perfcap/danbo_fast.txt", "danbo_perfcap"), ("h36m_zju/anerf_base.txt", "anerf_base")])
@pytest.mark.parametrize("noise_std", [0.0, 1.0])
def test_softplus_training_takes_the_autograd_path(cfg_file, cfg_name, noise_std):
    """a Trainer with --density_type softplus: the fused step declines (density_type softplus), the autograd path runs end to end
    (also with raw_noise_std > 0), its training forward equals the eval render of the same rays, every gradient is finite, and a
    few optimiser steps lower the loss on a fixed batch"""
    from core.utils import synthetic as syn
    args, caster, trainer, opt = _trainer(cfg_file, cfg_name, ("--perturb", "0", "--raw_noise_std", str(noise_std)))
    assert trainer.fused_engine() is None and trainer.fused_reason == "density_type softplus"
    scene = syn.make_scene(n_poses=1, H=24, W=24, n_views=1, pose_seed=3)
    ro, rd = scene["rays"][0]
    sel = np.random.default_rng(0).permutation(len(ro))[:128]
    ro, rd = ro[sel], rd[sel]
    R = len(ro)
    zr = np.zeros(R, np.int64)
    gen = torch.Generator(device=DEV).manual_seed(0)
    batch = dict(rays_o=T(ro), rays_d=T(rd), target_s=torch.rand(R, 3, device=DEV, generator=gen), bgs=torch.rand(R, 3, device=DEV, generator=gen),
                 kp3d=T(scene["kps"][zr]), skts=T(scene["skts"][zr]), bones=T(scene["bones"][zr]), cyls=T(scene["cyls"][zr]),
                 cam_idxs=T(zr, torch.int64), N_uniques=1)
    kw = {k: v for k, v in trainer.render_kwargs_train.items() if k not in ("ray_caster", "use_viewdirs")}
    caster.train()
    losses = []
    try:
        for it in range(6):
            torch.manual_seed(7)                      # the same density noise every step: the loss is one function of the weights
            preds = caster(trainer._ray_batch(batch), kp_batch=batch["kp3d"], skts=batch["skts"], cyls=batch["cyls"], bones=batch["bones"],
                           cams=batch["cam_idxs"], N_uniques=1, **kw)
            loss = trainer.compute_loss(batch, preds)
            opt.zero_grad()
            loss["total_loss"].backward()
            grads = [p.grad for p in caster.parameters() if p.grad is not None]
            assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
            assert sum(float(g.abs().sum()) for g in grads) > 0
            if it == 0 and noise_std == 0.0:
                caster.eval()
                with torch.no_grad():
                    te = {k: v for k, v in trainer.render_kwargs_test.items() if k not in ("ray_caster", "use_viewdirs", "N_samples",
                                                                                          "N_importance")}
                    ev = caster(trainer._ray_batch(batch), N_samples=12, N_importance=6, kp_batch=batch["kp3d"], skts=batch["skts"],
                                cyls=batch["cyls"], bones=batch["bones"], cams=batch["cam_idxs"], N_uniques=1, **te)
                caster.train()
                for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
                    assert max_err(N(preds[k]), N(ev[k])) < 2e-3, k
                assert float(ev["acc_map"].min()) > 0.
            losses.append(float(loss["total_loss"].detach()))
            opt.step()
    finally:
        caster.eval()
    print("softplus autograd training %s noise %.1f: losses %s" % (cfg_name, noise_std, ["%.5f" % v for v in losses]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


@pytest.mark.parametrize("use_background", [False, True])
def test_anerf_two_net_softplus_autograd_step_matches_float64(use_background, monkeypatch):
    """test_gpu_two_net.py::test_anerf_two_net_autograd_step_matches_float64 under softplus: the arbiter's module-level composite
    is switched to a float64 softplus composite that keeps the `clamped` argument (the branch of acc = min(sum w, 1) the path under
    test took, per ray: under softplus nearly every ray sits on that kink); same helper, same bounds."""
    import torch_f64_anerf_train as f64
    from core import hip_ops as ops
    from core import train_path
    from core.utils import synthetic as syn
    from helpers import golden
    from test_gpu_two_net import _f64_two_net_bracketed
    shift = 0.5
    g = golden("anerf_train")
    S, Sf = int(g["N_samples"]), int(g["N_importance"])
    args, caster, kw, orcs, tr = softplus_caster("h36m_zju/anerf_base.txt", "anerf_base", shift, True, seeds=(int(g["weight_seed"]), 17),
                                                 n_codes=int(g["n_framecodes"]))
    cfg = syn.model_config("anerf_base")
    sds = [syn.make_state_dict(cfg, seed=s, n_framecodes=int(g["n_framecodes"]), rest=syn.rest_pose(0.48)) for s in (int(g["weight_seed"]), 17)]
    for k in ("pe_fn.cutoff_dist", "dirs_pe_fn.cutoff_dist", "pe_fn.tau", "dirs_pe_fn.tau"):
        sds[1][k] = sds[0][k]
    caster.network_fine.load_state_dict({k: torch.tensor(v) for k, v in sds[1].items()}, strict=True)
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sds[0].items()}, strict=True)
    args.use_background = use_background
    tau = float(caster.network.pe_fn.tau)
    pose, rb = g["pose_of_ray"], g["ray_batch"]
    seen = {}
    orig = ops.importance_samples

    def spy(z, w, Sf_, u=None, flat=None, two_net=False):
        res = orig(z, w, Sf_, u, flat=flat, two_net=two_net)
        seen.update(z=z.detach().cpu().numpy(), z_all=res[0].cpu().numpy(), two_net=two_net)
        return res
    monkeypatch.setattr(ops, "importance_samples", spy)
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
        caster.eval()
    assert seen["two_net"]
    # the branch each composite of the path under test took, in the order the arbiter calls its composite: coarse, fine
    clamped = [~(out["acc0"].detach().cpu() < 1.0), ~(out["acc_map"].detach().cpu() < 1.0)]
    calls = []

    def composite_softplus(raw, z, rays_d, B, noise=None, clamped_=None):
        d = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(rays_d, dim=-1, keepdim=True)
        rgb = torch.sigmoid(raw[..., :3]) * 1.002 - 0.001
        dens = raw[..., 3] / B
        if noise is not None:
            dens = dens + noise
        alpha = 1.0 - torch.exp(-torch.nn.functional.softplus(dens - shift, beta=1) * d)
        w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
        sw = w.sum(-1)
        if clamped_ is None:
            clamped_ = clamped[len(calls) % 2]
        calls.append(1)
        acc = torch.where(clamped_, torch.ones_like(sw), sw)
        return dict(rgb_map=(w[..., None] * rgb).sum(-2), acc_map=acc, weights=w, alpha=alpha)
    monkeypatch.setattr(f64, "composite", composite_softplus)
    grads = {}
    for tag, net in (("c", caster.network), ("f", caster.network_fine)):
        for n, p in net.named_parameters():
            if p.requires_grad and "cutoff_dist" not in n:
                grads[(tag, n)] = N(p.grad).astype(np.float64) if p.grad is not None else np.zeros(tuple(p.shape))
    batch = dict(rays_o=rb[:, 0:3], rays_d=rb[:, 3:6], skts=g["skts"], cam_idx=g["cam_idx"], target=g["target"], bgs=g["bgs"])
    a = dict(loss_fn=args.loss_fn, use_background=bool(args.use_background), rgb_loss_coef=float(args.rgb_loss_coef),
             coarse_weight=float(args.coarse_weight), density_scale=float(args.density_scale), tau=tau)
    ref = _f64_two_net_bracketed(cfg, sds[0], sds[1], syn.rest_pose(0.48), batch, seen["z"], seen["z_all"], a)
    assert len(calls) == 8
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
    print("two-network A-NeRF softplus autograd step vs float64 (background %s): worst (error - bracket) / max = %.2e" % (use_background, worst))


def _f64_softplus_composite_tuple(shift):
    """oracle/torch_f64_train.composite with softplus(x - shift) for relu: same signature, same `clamped` argument, same outputs"""
    def composite_softplus(raw, z, rays_d, B, noise=None, clamped=None):
        d = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(rays_d, dim=-1, keepdim=True)
        rgb = torch.sigmoid(raw[..., :3]) * 1.002 - 0.001
        s = raw[..., 3] / B
        if noise is not None:
            s = s + noise
        alpha = 1.0 - torch.exp(-torch.nn.functional.softplus(s - shift, beta=1) * d)
        w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
        sw = w.sum(-1)
        acc = torch.clamp(sw, max=1.0) if clamped is None else torch.where(clamped, torch.ones_like(sw), sw)
        return (w[..., None] * rgb).sum(-2), acc, w, alpha
    return composite_softplus


@pytest.mark.parametrize("use_background", [False, True])
def test_danbo_softplus_autograd_step_matches_float64(use_background, monkeypatch):
    """A Trainer built from perfcap/danbo_fast.txt with --density_type softplus on the reference's training batch
    (danbo_perfcap_train: perturb = 0, noise = 0): the fused step declines, and the autograd step's losses and EVERY parameter
    gradient are compared with the float64 arbiter oracle/torch_f64_train.step on the path's own depths, its module-level composite
    switched to softplus (keeping `clamped`: the branch of acc = min(sum w, 1) the path's forward took per ray) -- helper and
    bounds of tests/test_gpu_train_engine.py (F64_BOUND of the tensor's max + 1.5 x the ReLU-kink bracket).  use_background: the
    loss then reads acc_map, so g_acc is exercised."""
    import torch_f64_train as t64
    from core import hip_ops
    from helpers import golden
    from test_gpu_train_engine import F64_BOUND, _f64_reference
    from test_gpu_training import batch_of, build_trainer
    shift = 0.5
    g = golden("danbo_perfcap_train")
    args, caster, trainer, opt = build_trainer(g, ("--density_type", "softplus", "--softplus_shift", str(shift)))
    args.use_background = use_background
    assert trainer.args is args and trainer.fused_engine() is None and trainer.fused_reason == "density_type softplus"
    b = batch_of(g)
    kw = {k: v for k, v in trainer.render_kwargs_train.items() if k not in ("ray_caster", "use_viewdirs")}
    samp = {}
    orig = hip_ops.importance_samples

    def spy(z, w, n, u=None, **k):
        out = orig(z, w, n, u, **k)
        samp.update(z_c=z.detach().clone(), z_f=out[1].detach().clone(), order=out[2].detach().clone())
        return out
    monkeypatch.setattr(hip_ops, "importance_samples", spy)
    caster.train()
    try:
        preds = caster(trainer._ray_batch(b), kp_batch=b["kp3d"], skts=b["skts"], cyls=b["cyls"], bones=b["bones"], cams=b["cam_idxs"],
                       N_uniques=b["N_uniques"], **kw)
        loss = trainer.compute_loss(b, preds)
        caster.zero_grad()
        loss["total_loss"].backward()
    finally:
        caster.eval()
    grads = {n: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for n, p in caster.network.named_parameters()}
    samp.update(acc0=preds["acc0"], acc_map=preds["acc_map"])
    monkeypatch.setattr(t64, "composite", _f64_softplus_composite_tuple(shift))
    r64 = _f64_reference(g, args, caster, b, samp)
    # relu's arbiter on the same depths is another function: the comparison is sensitive to the activation
    for k in ("rgb_loss", "rgb_loss0", "soft_softmax_loss", "total_loss"):
        ref = r64["loss"][k]
        assert abs(float(loss[k].detach()) - ref) <= 2e-4 * max(abs(ref), 1e-3), (k, float(loss[k].detach()), ref)
    assert np.abs(N(preds["rgb_map"]) - r64["rgb_map"]).max() < 5e-4 and np.abs(N(preds["rgb0"]) - r64["rgb0"]).max() < 5e-5
    worst, name, nonzero = 0.0, "", 0
    for n, gr in grads.items():
        t = r64["grads"][n]
        scale = float(np.abs(t).max())
        d = float(np.abs(N(gr).astype(np.float64) - t).max())
        nonzero += scale > 0
        if d / (scale + 1e-30) > worst:
            worst, name = d / (scale + 1e-30), n
        assert d <= F64_BOUND * scale + 1.5 * r64["bracket"][n] + 1e-9, (n, d, scale, r64["bracket"][n])
    assert nonzero > 30
    print("DANBO softplus autograd step vs float64 (background %s): worst gradient deviation %.2e of the tensor's max in %s" % (
        use_background, worst, name))
    monkeypatch.undo()
    relu = _f64_reference(g, args, caster, b, samp)
    assert abs(relu["loss"]["rgb_loss"] - r64["loss"]["rgb_loss"]) > 1e-3 * abs(r64["loss"]["rgb_loss"])


def test_danbo_two_net_softplus_autograd_training_step():
    """tests/test_gpu_two_net.py::test_two_net_autograd_training_step for danbo_base under softplus: the autograd path trains both
    networks -- the coarse one through rgb_loss0 alone, the fine one through the final maps on all S + Sf samples -- with finite,
    non-zero gradients, and its training forward equals the eval render of the same rays"""
    from core import train_engine, train_path
    args, caster, kw, orcs, tr = softplus_caster("h36m_zju/danbo_base.txt", "danbo_base", 0.5, True)
    assert train_engine.supported(args, caster) is not None
    scene, rb = body_scene()
    rb = rb[:256][np.random.default_rng(0).permutation(256)[:96]]
    S, Sf = 12, 6
    R = len(rb)
    z = np.zeros(R, np.int64)
    kwt = {k: v for k, v in tr.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    kwt.update(perturb=0., raw_noise_std=0.)
    caster.train()
    try:
        out = caster(T(rb), N_samples=S, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                     bones=T(scene["bones"][z]), cams=T(np.zeros(R), torch.int64), N_importance=Sf, N_uniques=1, **kwt)
        assert out["alpha"].shape == (R, S + Sf) and out["alpha0"].shape == (R, S)
        target = torch.rand(R, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        loss = ((out["rgb_map"] - target) ** 2).mean()
        loss0 = ((out["rgb0"] - target) ** 2).mean()
        net_c = [p for p in caster.network.parameters() if p.requires_grad]
        net_f = [p for p in caster.network_fine.parameters() if p.requires_grad]
        g_c = torch.autograd.grad(loss, net_c, allow_unused=True, retain_graph=True)
        assert all(g is None or not bool(g.any()) for g in g_c)          # no path from the final maps to the coarse network
        g_f0 = torch.autograd.grad(loss0, net_f, allow_unused=True, retain_graph=True)
        assert all(g is None or not bool(g.any()) for g in g_f0)
        g_c0 = torch.autograd.grad(loss0, net_c, allow_unused=True, retain_graph=True)
        g_f = torch.autograd.grad(loss, net_f, allow_unused=True, retain_graph=True)
        for gs in (g_c0, g_f):
            gs = [g for g in gs if g is not None]
            assert gs and all(bool(torch.isfinite(g).all()) for g in gs) and sum(float(g.abs().sum()) for g in gs) > 0
        ssl = train_path.soft_softmax_loss(args, caster.network_fine, out)
        g_sf = torch.autograd.grad(ssl, net_f, allow_unused=True, retain_graph=True)
        assert sum(float(g.abs().sum()) for g in g_sf if g is not None) > 0
        with torch.no_grad():
            caster.eval()
            ev = cast(caster, kw, scene, rb, S, Sf)
        for k in ("rgb_map", "acc_map", "rgb0", "acc0"):
            assert max_err(N(out[k]), N(ev[k])) < 2e-3, k
        # ... and the eval render is the softplus one: the composed oracle's, not relu's
        ref = render_composed(orcs[0], orcs[1], rb, scene["skts"][z], scene["bones"][z], scene["cyls"][z], z, 1, S, Sf, act=0.5)
        assert max_err(N(ev["rgb_map"]), ref["rgb_map"]) < 5e-4 and max_err(N(ev["rgb0"]), ref["rgb0"]) < 1e-5
    finally:
        caster.eval()


# ----------------------------------------------------------------------------- entry points
def test_softplus_train_checkpoint_render_round_trip(tmp_path):
    """run_nerf.train with --density_type softplus --softplus_shift 0.5: args.txt carries both, the trainer takes the autograd
    path, run_render rebuilds the caster from args.txt and renders what the trained caster renders on the same rays"""
    import run_nerf
    import run_render
    from core.raycasters import SoftplusDensity
    src = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "perfcap", "danbo_fast.txt")
    lines = [l for l in open(src) if not l.startswith(("N_samples", "N_importance"))]
    cfg_path = tmp_path / "danbo_softplus.txt"
    cfg_path.write_text("".join(lines) + "N_samples = 16\nN_importance = 8\n")
    common = ["--config", str(cfg_path), "--basedir", str(tmp_path), "--expname", "sp", "--syn_poses", "2", "--syn_cams", "2",
              "--syn_res", "32", "--N_rand", "256", "--N_sample_images", "2", "--i_print", "10", "--i_weights", "6",
              "--i_testset", "1000", "--render_factor", "0", "--density_type", "softplus", "--softplus_shift", "0.5"]
    trainer = run_nerf.train(common + ["--n_iters", "6"])
    caster = trainer.render_kwargs_train["ray_caster"]
    assert trainer.fused_engine() is None and trainer.fused_reason == "density_type softplus"
    log = tmp_path / "sp"
    txt = open(log / "args.txt").read()
    assert "density_type = softplus" in txt and "softplus_shift = 0.5" in txt
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
        rgbs, accs, _, _ = run_render.run_render(["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000006.tar"),
                                                  "--dataset", "synthetic", "--entry", "val", "--outputdir", str(tmp_path / "out"),
                                                  "--render_type", "bullet", "--n_bullet", "2", "--selected_idxs", "0", "--runname", "bt",
                                                  "--render_res", "32", "32", "--no_save"])
    finally:
        run_render.load_nerf, run_render.render_path = orig_load, orig_path
    fn = loaded["kw"]["preproc_kwargs"]["density_fn"]
    assert isinstance(fn, SoftplusDensity) and fn.softplus_shift == 0.5
    assert rgbs.shape == (2, 32, 32, 3) and np.isfinite(rgbs).all() and np.isfinite(accs).all()
    k = dict(calls[0])
    k["render_kwargs"] = dict(k["render_kwargs"], ray_caster=caster.eval())
    again = orig_path(**k)[0]
    assert np.array_equal(again, rgbs)
