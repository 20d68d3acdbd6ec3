"""GPU tests of the training path: losses and gradients against the reference's own autograd
(tests/golden/danbo_train.npz: Trainer.compute_loss + backward with perturb = 0, raw_noise_std = 0),
finite-difference checks of the two hand-written backward kernels, and one optimiser step."""
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, golden, T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


CONFIG_OF = {"danbo_base": ("h36m_zju", "danbo_base.txt"), "danbo_perfcap": ("perfcap", "danbo_fast.txt")}


def build_trainer(g, extra=()):
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.trainer import Trainer
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload", "--N_samples", str(int(g["N_samples"])), "--N_importance", str(int(g["N_importance"])),
                       "--perturb", "0", "--raw_noise_std", "0", *extra],
                      config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", *CONFIG_OF[str(g["cfg_name"])]))
    n_codes = int(g["n_framecodes"])
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    tr_kw, te_kw, start, grad_vars, opt, _ = create_raycaster(args, da, device=DEV)
    caster = tr_kw["ray_caster"]
    cfg = syn.model_config(str(g["cfg_name"]))
    sd = syn.make_state_dict(cfg, int(g["weight_seed"]), n_codes, syn.rest_pose(0.48))
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    return args, caster, Trainer(args, da, opt, None, tr_kw, te_kw, device=DEV), opt


def batch_of(g):
    pose = g["pose_of_ray"]
    rb = g["ray_batch"]
    return dict(rays_o=T(rb[:, 0:3]), rays_d=T(rb[:, 3:6]), target_s=T(g["target"]), bgs=T(g["bgs"]),
                kp3d=T(g["kps"][pose]), skts=T(g["skts"][pose]), bones=T(g["bones"][pose]), cyls=T(g["cyls"][pose]),
                cam_idxs=T(g["cam_idx"], torch.int64), N_uniques=int(g["n_uniques"]))


@pytest.mark.parametrize("fixture", ["danbo_train", "danbo_perfcap_train"])
def test_losses_and_gradients_match_reference_autograd(fixture):
    """danbo_train: D-H36M (world rays, identity view, cylinder near/far); danbo_perfcap_train: BASELINE config 4's network
    (root_local rays, relray view, per-bone box near/far, its vol_scale_penalty)"""
    g = golden(fixture)
    args, caster, trainer, opt = build_trainer(g)
    caster.train()
    batch = batch_of(g)
    kw = {k: v for k, v in trainer.render_kwargs_train.items() if k not in ("ray_caster", "use_viewdirs")}
    preds = caster(trainer._ray_batch(batch), kp_batch=batch["kp3d"], skts=batch["skts"], cyls=batch["cyls"],
                   bones=batch["bones"], cams=batch["cam_idxs"], N_uniques=batch["N_uniques"], **kw)
    assert np.abs(preds["rgb_map"].detach().cpu().numpy() - g["rgb_map"]).max() < 5e-4
    assert np.abs(preds["rgb0"].detach().cpu().numpy() - g["rgb0"]).max() < 5e-5
    assert np.array_equal(preds["part_invalid"].cpu().numpy(), g["part_invalid"])
    loss = trainer.compute_loss(batch, preds)
    for k in ("rgb_loss", "rgb_loss0", "soft_softmax_loss", "vol_scale_loss", "total_loss"):
        ref = float(g["loss/" + k])
        assert abs(float(loss[k].detach()) - ref) <= 2e-4 * max(abs(ref), 1e-3), (k, float(loss[k].detach()), ref)
    caster.zero_grad()
    loss["total_loss"].backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in caster.network.named_parameters() if p.grad is not None}
    # every parameter the reference gives a gradient has one here, with the same norm
    for key in g.files:
        if key.startswith("gnorm/"):
            n = key[len("gnorm/"):]
            ours = float(np.sqrt((grads[n].astype(np.float64) ** 2).sum()))
            ref = float(g[key])
            assert abs(ours - ref) <= 5e-3 * ref + 1e-9, (n, ours, ref)
    for key in g.files:
        if not key.startswith("grad/"):
            continue
        n = key[len("grad/"):]
        if "[" in n:
            base, sl = n.split("[", 1)
            ours = eval("grads[base][" + sl)
        else:
            ours = grads[n]
        ref = g[key]
        scale = np.abs(ref).max() + 1e-12
        assert np.abs(ours - ref).max() <= 5e-3 * scale, (n, np.abs(ours - ref).max(), scale)


def test_composite_backward_matches_torch_autograd():
    from core import train_path
    rng = np.random.default_rng(1)
    R, S = 33, 80                                    # two wave chunks
    raw = T(rng.normal(0, 1.5, size=(R, S, 4))).requires_grad_(True)
    z = T(np.sort(rng.uniform(2, 5, size=(R, S)), -1))
    d = T(rng.normal(size=(R, 3)))
    noise = T(rng.normal(0, 0.3, size=(R, S)))
    out = train_path.composite(raw, z, d, 0.7, noise)
    g_rgb, g_acc = T(rng.normal(size=(R, 3))), T(rng.normal(size=(R,)))
    ((out["rgb_map"] * g_rgb).sum() + (out["acc_map"] * g_acc).sum()).backward()
    ours = raw.grad.clone()
    # the same function in eager torch (reference nerf.py:281-347)
    raw2 = raw.detach().clone().requires_grad_(True)
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1) * torch.norm(d, dim=-1, keepdim=True)
    rgb = torch.sigmoid(raw2[..., :3]) * 1.002 - 0.001
    alpha = 1. - torch.exp(-torch.relu(raw2[..., 3] / 0.7 + noise) * dist)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    rgb_map = (w[..., None] * rgb).sum(-2)
    acc = torch.minimum(w.sum(-1), torch.tensor(1., device=DEV))
    ((rgb_map * g_rgb).sum() + (acc * g_acc).sum()).backward()
    ref = raw2.grad
    assert float((ours - ref).abs().max()) <= 2e-4 * float(ref.abs().max())


def test_gather_backward_against_finite_differences():
    from core import custom_ops  # noqa: F401  (registers torch.ops.danbo.bone_gather)
    from core import hip_ops as ops
    from core.utils import synthetic as syn
    g = golden("danbo_stages")
    rb = g["ray_batch"]
    cfg = syn.model_config("danbo_base")
    sd = syn.make_state_dict(cfg, int(g["weight_seed"]), 20, syn.rest_pose(0.48))
    vols = T(g["volumes"]).transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)   # permuted strides, as einsum hands over
    sc = T(sd["graph_net.axis_scale"]).requires_grad_(True)
    geo = ops.Geometry(T(rb[:, 0:3]), T(rb[:, 3:6]), T(g["skts"]), T(g["align"]), sc.detach(), z=T(g["z_coarse"]))
    bits, lst, cnt = ops.bone_cull(geo, True)
    rows = torch.sort(lst[: int(cnt.item())]).values.contiguous()
    w = T(np.random.default_rng(0).normal(size=(rows.shape[0], 24, 15)))
    pts = (geo.rays_o[:, None, :] + geo.rays_d[:, None, :] * geo.z[..., None]).contiguous()     # o + d z, two roundings: the kernels' points
    gather = lambda v, s: torch.ops.danbo.bone_gather(v, s, pts, geo.skts, geo.align, rows)     # noqa: E731
    pf = gather(vols, sc)
    (pf * w).sum().backward()
    # d volumes: the forward is linear in the volumes -> exact directional check
    dv = T(np.random.default_rng(1).normal(size=tuple(vols.shape)))
    lin = (gather(dv, sc.detach()) * w).sum()
    assert abs(float((vols.grad * dv).sum()) - float(lin)) <= 1e-4 * abs(float(lin))
    # The C entry point in depth mode (rays + z: the package itself passes points): the kernel forms the same points bit for bit, so
    # every term of d volumes is the same float and only the order of the fp32 atomic additions differs from the run above.  A term
    # of d volumes has the sign of its upstream value (the interpolation weights and the window are >= 0), so the same call on |w|
    # gives sum |terms| per entry, and two orders of at most n additions differ by at most 2 n 2^-24 of it.
    vols_c = vols.detach().contiguous()

    def depth_mode(up):
        d_vol, d_sc = torch.zeros(tuple(vols.shape), device=DEV), torch.zeros(tuple(sc.shape), device=DEV)
        ops._call("danbo_bone_gather_bwd", *geo.head(), ops._p(vols_c), ops._p(rows), rows.shape[0], ops._p(up), ops._p(d_vol),
                  ops._p(d_sc), ops._stream())
        return d_vol
    bound = 2 * rows.shape[0] * 2.0 ** -24 * depth_mode(w.abs()) * (1 + 1e-3)
    diff = (depth_mode(w) - vols.grad).abs()
    print("depth mode against point mode: max |difference| of d volumes", float(diff.max()), "of", float(vols.grad.abs().max()),
          "; n =", rows.shape[0], ", entries above their bound:", int((diff > bound).sum()))
    assert bool((diff <= bound).all()) and float(vols.grad.abs().max()) > 0
    # d axis_scale: central differences on a few entries (window detached => freeze it via small eps only)
    base = sc.detach().clone()
    for (j, k) in [(1, 0), (4, 2), (9, 1), (16, 2)]:
        eps = 1e-3
        vals = []
        for sgn in (+1, -1):
            s2 = base.clone()
            s2[j, k] += sgn * eps
            vals.append(gather(vols.detach(), s2))
        # remove the (detached) window's own dependence on the scale: divide it out
        fd = float((((vals[0] - vals[1]) / (2 * eps)) * w).sum())
        an = float(sc.grad[j, k])
        if abs(fd) > 1e-3:   # the finite difference also moves the window; only the sign/magnitude class is comparable
            assert np.sign(fd) == np.sign(an) or abs(fd - an) < 0.5 * abs(fd)


def test_assign_blend_custom_op_forward_backward_and_opcheck():
    """torch.ops.danbo.assign_blend (gather + assignment GNN + masked sigmoid + blend, one HIP kernel each way) against the same
    computation spelled with torch ops on the materialised part_feat (torch.ops.danbo.bone_gather + einsums, train_path.py): h, p,
    confd and the gradient of every input that carries one -- the pose volumes, axis_scale, the 7 assignment-net parameters --
    with upstream gradients on BOTH differentiable outputs; schema / fake-tensor opcheck"""
    from core import custom_ops  # noqa: F401
    from core import hip_ops as ops, train_path
    from core.utils import synthetic as syn
    g = golden("danbo_stages")
    rb = g["ray_batch"]
    cfg = syn.model_config("danbo_base")
    sd = syn.make_state_dict(cfg, int(g["weight_seed"]), 20, syn.rest_pose(0.48))
    a = "prob_linears.layers."
    names = ["0.lin.weight", "0.adj_w", "0.adj", "0.bias", "1.weight", "1.bias", "2.weight", "2.bias"]
    rays_o, rays_d, z = T(rb[:, 0:3]), T(rb[:, 3:6]), T(g["z_coarse"])
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]).contiguous()
    skts, align = T(g["skts"]), T(g["align"])
    geo = ops.Geometry(rays_d, rays_d, skts, align, T(sd["graph_net.axis_scale"]), pts=pts)
    bits, lst, cnt = ops.bone_cull(geo, True)
    rows = torch.sort(lst[: int(cnt.item())]).values.contiguous()
    n = rows.shape[0]
    assert n > 20
    rng = np.random.default_rng(3)
    gh, gp = T(rng.normal(size=(n, 16)) * 1e-3), T(rng.normal(size=(n, 24)) * 1e-3)
    gh[:, 15] = 0.0

    def leaves():
        vols = T(g["volumes"]).requires_grad_(True)
        sc = T(sd["graph_net.axis_scale"]).requires_grad_(True)
        params = [T(sd[a + k]).requires_grad_(k != "0.adj") for k in names]
        return vols, sc, params

    vols, sc, params = leaves()
    h, p, confd = torch.ops.danbo.assign_blend(vols, sc, pts, skts, align, rows, bits, params)
    assert not confd.requires_grad or True
    ((h * gh).sum() + (p * gp).sum()).backward()

    vols_r, sc_r, params_r = leaves()
    w0, adj_w, adj, b0, w1, b1, w2, b2 = params_r
    pf = torch.ops.danbo.bone_gather(vols_r, sc_r, pts, skts, align, rows)
    y = torch.einsum("bkl,klj->bkj", pf, w0)
    y = torch.relu(torch.einsum("ij,bjc->bic", (adj_w * adj)[0], y) + b0)
    y = torch.relu(torch.einsum("bkl,klj->bkj", y, w1) + b1)
    logits = (torch.einsum("bkl,klj->bkj", y, w2) + b2)[..., 0]
    shifts = torch.arange(24, device=DEV, dtype=torch.int32)
    valid = ((bits[rows.long()].unsqueeze(-1) >> shifts) & 1).float()
    p_r = (torch.sigmoid(logits) * 1.002 - 0.001) * valid
    h_r = (pf * p_r[..., None]).sum(-2)
    ((h_r * gh[:, :15]).sum() + (p_r * gp).sum()).backward()

    assert (h[:, :15] - h_r).abs().max().item() <= 2e-6 * h_r.abs().max().item()
    assert (h[:, 15] == 0).all()
    assert (p - p_r).abs().max().item() <= 2e-6
    assert (confd - logits).abs().max().item() <= 2e-5 * logits.abs().max().item()
    worst = 0.0
    for name, x, r in [("volumes", vols.grad, vols_r.grad), ("axis_scale", sc.grad, sc_r.grad)] + \
            [(k, q.grad, r_.grad) for k, q, r_ in zip(names, params, params_r) if k != "0.adj"]:
        assert x is not None and r is not None, name
        e = ((x - r).abs().max() / (r.abs().max() + 1e-30)).item()
        worst = max(worst, e)
        assert e < 2e-4, (name, e)
    assert params[2].grad is None
    print("assign_blend op: worst gradient deviation relative to the tensor's max", worst)
    torch.library.opcheck(torch.ops.danbo.assign_blend,
                          (vols.detach(), sc.detach(), pts, skts, align, rows, bits, [q.detach() for q in params]),
                          test_utils=("test_schema", "test_faketensor"))


def test_pose_volumes_custom_op_forward_backward_and_opcheck():
    """torch.ops.danbo.pose_volumes (rot6d + PE + FactorizeGNN on k_pose_layer, adjoint on k_pose_layer_bwd / k_pose_mix_bwd)
    against the same network recorded layer by layer with torch ops in float64 (reference core/networks/gnn_backbone.py:683-704
    incl. mask_root and the doubled first layer): the volumes and the gradient of all ten parameters for a random upstream
    gradient; schema / fake-tensor opcheck"""
    from core import custom_ops  # noqa: F401
    from core import train_path
    from core.utils import synthetic as syn
    g = golden("danbo_stages")
    cfg = syn.model_config("danbo_base")
    sd = syn.make_state_dict(cfg, int(g["weight_seed"]), 20, syn.rest_pose(0.48))
    p_ = "graph_net.layers."
    names = ["0.lin.weight", "0.adj_w", "0.adj", "0.bias", "1.lin.weight", "1.adj_w", "1.adj", "1.bias", "2.weight", "2.bias", "3.weight", "3.bias"]
    bones = T(np.concatenate([g["bones"], g["bones"][::-1] * 0.7, np.zeros_like(g["bones"][:1])]))       # 5 poses incl. the rest pose
    L = cfg["multires_graph"]
    params = [T(sd[p_ + k]).requires_grad_(not k.endswith(".adj")) for k in names]
    vol, scratch = torch.ops.danbo.pose_volumes(bones, L, params)
    assert vol.shape == (bones.shape[0], 24, 240) and not scratch.requires_grad
    gv = T(np.random.default_rng(5).normal(size=tuple(vol.shape)) * 1e-3)
    (vol * gv).sum().backward()
    # float64 reference
    q = [T(sd[p_ + k], torch.float64).requires_grad_(not k.endswith(".adj")) for k in names]
    w0, aw0, a0, b0, w1, aw1, a1, b1, w2, b2, w3, b3 = q
    n = train_path.positional_encoding(train_path.axis_angle_to_rot6d(bones.double()), L)
    mask = torch.ones(1, 24, 1, device=DEV, dtype=torch.float64)
    mask[:, 0] = 0.
    n = n * mask
    y = torch.matmul((aw0 * a0)[0], torch.einsum("bkl,klj->bkj", n, w0)) + b0
    n = torch.relu(y + y)
    n = torch.relu(torch.matmul((aw1 * a1)[0], torch.einsum("bkl,klj->bkj", n, w1)) + b1)
    n = torch.relu(torch.einsum("bkl,klj->bkj", n, w2) + b2)
    ref = torch.einsum("bkl,klj->bkj", n, w3) + b3
    (ref * gv.double()).sum().backward()
    assert (vol.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    worst = 0.0
    for k, a, r in zip(names, params, q):
        if k.endswith(".adj"):
            assert a.grad is None
            continue
        e = ((a.grad.double() - r.grad).abs().max() / (r.grad.abs().max() + 1e-300)).item()
        worst = max(worst, e)
        assert a.grad.shape == a.shape and e < 5e-5, (k, e)
    print("pose_volumes op: worst parameter-gradient deviation from float64 (of the tensor's max):", worst)
    # the route core/train_path.py takes for a DANBO module, against its layer-by-layer fall-back
    torch.library.opcheck(torch.ops.danbo.pose_volumes, (bones, L, [t.detach() for t in params]), test_utils=("test_schema", "test_faketensor"))


def test_autograd_path_operators_equal_the_layerwise_torch_route():
    """core/train_path.py's differentiable caster forward on the three HIP operators (danbo.pose_volumes, danbo.assign_blend,
    danbo.pe_mlp) against the same forward recorded layer by layer with torch / library GEMMs (tests/torch_layerwise.py: test
    infrastructure since round 5 -- the product has no library route any more and raises for a network of another shape): loss
    terms and the gradient of EVERY parameter on the config-4 network."""
    from core import train_path
    g = golden("danbo_perfcap_train")

    import torch_layerwise

    def run(layerwise):
        saved = train_path.forward_train
        if layerwise:
            train_path.forward_train = torch_layerwise.forward_train
        try:
            args, caster, trainer, opt = build_trainer(g)
            caster.train()
            b = batch_of(g)
            kw = {k: v for k, v in trainer.render_kwargs_train.items() if k not in ("ray_caster", "use_viewdirs")}
            preds = caster(trainer._ray_batch(b), kp_batch=b["kp3d"], skts=b["skts"], cyls=b["cyls"], bones=b["bones"], cams=b["cam_idxs"],
                           N_uniques=b["N_uniques"], **kw)
            loss = trainer.compute_loss(b, preds)
            caster.zero_grad()
            loss["total_loss"].backward()
        finally:
            train_path.forward_train = saved
        return ({n: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for n, p in caster.network.named_parameters()},
                {k: float(v.detach()) for k, v in loss.items()})
    g_op, l_op = run(False)
    g_lw, l_lw = run(True)
    for k in l_op:
        assert abs(l_op[k] - l_lw[k]) <= 2e-6 * max(abs(l_lw[k]), 1e-3), (k, l_op[k], l_lw[k])
    worst, name = 0.0, ""
    for n, r in g_lw.items():
        e = float((g_op[n] - r).abs().max()) / (float(r.abs().max()) + 1e-30)
        if e > worst:
            worst, name = e, n
        assert e < 1e-4, (n, e)
    print("operators vs layer-by-layer torch route: worst gradient deviation (of the tensor's max)", worst, "in", name)


def test_one_optimiser_step_changes_parameters_and_stays_finite():
    g = golden("danbo_train")
    args, caster, trainer, opt = build_trainer(g, extra=["--raw_noise_std", "1.0", "--perturb", "1.0"])
    before = {n: p.detach().clone() for n, p in caster.network.named_parameters()}
    torch.manual_seed(0)
    loss, stats = trainer.train_batch(batch_of(g), i=0, global_step=0)
    assert np.isfinite(stats["total_loss"])
    assert stats["lrate"] == pytest.approx(5e-4 * 0.1 ** (1 / 500000), rel=1e-9)   # the reference decays from the optimizer step just made
    moved = [n for n, p in caster.network.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) >= 40 and "graph_net.axis_scale" in moved and "framecodes.codes.weight" in moved
    loss2, stats2 = trainer.train_batch(batch_of(g), i=1, global_step=1)
    assert np.isfinite(stats2["total_loss"])
    # the eval path picks up the updated weights (packed buffers are rebuilt from the parameter versions)
    caster.eval()
    kw = {k: v for k, v in trainer.render_kwargs_test.items() if k not in ("ray_caster", "use_viewdirs")}
    b = batch_of(g)
    out = caster(trainer._ray_batch(b), kp_batch=b["kp3d"], skts=b["skts"], cyls=b["cyls"], bones=b["bones"],
                 cams=b["cam_idxs"], N_uniques=b["N_uniques"], **kw)
    assert torch.isfinite(out["rgb_map"]).all()


def test_anerf_losses_and_gradients_match_reference_autograd():
    """A-NeRF (cutoff PE, W = 448): loss terms and gradients of every parameter against the reference's autograd"""
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.trainer import Trainer
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    g = golden("anerf_train")
    args = parse_args(["--no_reload", "--N_samples", str(int(g["N_samples"])), "--N_importance", str(int(g["N_importance"])),
                       "--perturb", "0", "--raw_noise_std", "0"],
                      config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt"))
    n_codes = int(g["n_framecodes"])
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    tr_kw, te_kw, start, grad_vars, opt, _ = create_raycaster(args, da, device=DEV)
    caster = tr_kw["ray_caster"]
    sd = syn.make_state_dict(syn.model_config("anerf_base"), int(g["weight_seed"]), n_codes, syn.rest_pose(0.48))
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    trainer = Trainer(args, da, opt, None, tr_kw, te_kw, device=DEV)
    caster.train()
    batch = batch_of(g)
    kw = {k: v for k, v in trainer.render_kwargs_train.items() if k not in ("ray_caster", "use_viewdirs")}
    preds = caster(trainer._ray_batch(batch), kp_batch=batch["kp3d"], skts=batch["skts"], cyls=batch["cyls"],
                   bones=batch["bones"], cams=batch["cam_idxs"], N_uniques=batch["N_uniques"], **kw)
    assert "confd" not in preds
    assert np.abs(preds["rgb_map"].detach().cpu().numpy() - g["rgb_map"]).max() < 1e-3
    loss = trainer.compute_loss(batch, preds)
    assert set(loss) == {"rgb_loss", "rgb_loss0", "total_loss"}
    for k in loss:
        ref = float(g["loss/" + k])
        assert abs(float(loss[k].detach()) - ref) <= 5e-4 * abs(ref), (k, float(loss[k].detach()), ref)
    caster.zero_grad()
    loss["total_loss"].backward()
    grads = {n: p.grad.detach().cpu().numpy() for n, p in caster.network.named_parameters() if p.grad is not None}
    for key in g.files:
        if key.startswith("gnorm/"):
            n = key[len("gnorm/"):]
            ours, ref = float(np.sqrt((grads[n].astype(np.float64) ** 2).sum())), float(g[key])
            assert abs(ours - ref) <= 2e-2 * ref + 1e-9, (n, ours, ref)
    for key in g.files:
        if not key.startswith("grad/"):
            continue
        n = key[len("grad/"):]
        if "[" in n:
            base, sl = n.split("[", 1)
            ours = eval("grads[base][" + sl)
        else:
            ours = grads[n]
        ref = g[key]
        assert np.abs(ours - ref).max() <= 2e-2 * (np.abs(ref).max() + 1e-12), (n, np.abs(ours - ref).max(), np.abs(ref).max())
    # and one optimiser step runs
    l2, stats = trainer.train_batch(batch, i=0, global_step=0)
    assert np.isfinite(stats["total_loss"])


@pytest.mark.parametrize("gscale", [1.0, 3e-7])
def test_linear16_autograd_function_matches_float64(gscale):
    """core/train_path.Linear16Fn (A-NeRF's training trunk: k_linear16 forward, transposed-weight k_linear16 for dX, k_dw16 for dW /
    db) against float64 autograd of relu([x1 | x2] W^T + b): one- and two-input (skip) layers of A-NeRF's widths, upstream
    gradients of ordinary size and at 3e-7 (what the loss hands the trunk: below fp16's normal range before the pre-scaling)"""
    from core import train_path
    gen = torch.Generator(device="cpu").manual_seed(17)
    M = 1500 - 13
    for K1, K2, N in ((432, 0, 448), (448, 0, 448), (432, 448, 448)):
        lin = torch.nn.Linear(K1 + K2, N).to(DEV)
        x1 = torch.randn(M, K1, generator=gen).to(DEV).requires_grad_(True)
        x2 = torch.randn(M, K2, generator=gen).to(DEV).requires_grad_(True) if K2 else None
        gy = (torch.randn(M, N, generator=gen) * gscale).to(DEV)
        y = train_path.linear16(lin, x1, relu=True, x2=x2, x_grad=True)
        assert y.grad_fn is not None and "Linear16Fn" in type(y.grad_fn).__name__
        (y * gy).sum().backward()
        w64, b64 = lin.weight.detach().double().requires_grad_(True), lin.bias.detach().double().requires_grad_(True)
        a1 = x1.detach().double().requires_grad_(True)
        a2 = x2.detach().double().requires_grad_(True) if K2 else None
        xin = a1 if a2 is None else torch.cat([a1, a2], -1)
        z64 = xin @ w64.t() + b64
        # the ReLU's branch per element is taken from the kernel's output (a pre-activation within fp32 round-off of 0 may sit on
        # either side: one such (row, unit) pair moves that unit's weight gradient by the row's whole contribution) -- after
        # checking that the two only disagree there
        mask = y.detach() > 0
        assert float(z64.detach()[mask != (z64.detach() > 0)].abs().max().item() if bool((mask != (z64.detach() > 0)).any()) else 0.0) < 1e-5
        y64 = z64 * mask
        (y64 * gy.double()).sum().backward()
        assert float((y.detach().double() - y64.detach()).abs().max()) <= 3e-6 * float(y64.detach().abs().max())
        pairs = [("weight", lin.weight.grad, w64.grad), ("bias", lin.bias.grad, b64.grad), ("x1", x1.grad, a1.grad)]
        if K2:
            pairs.append(("x2", x2.grad, a2.grad))
        for name, a, r in pairs:
            e = float((a.double() - r).abs().max()) / float(r.abs().max())
            assert e < 2e-5, (K1, K2, name, e)
