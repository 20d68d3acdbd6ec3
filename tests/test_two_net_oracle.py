"""The two-network hierarchical mode (single_net = False: a coarse and a separate fine network) on the CPU: a numpy restatement of
isample_from_lineseg(is_only=False), the two-network renders composed from two oracle instances, the host build of the kernels'
two-network importance_ray against the restatement, and -- where the reference tree exists -- the composed oracle against the
reference caster built with single_net = False."""
import contextlib
import io
import os
import subprocess
import tempfile

import numpy as np
import pytest

import danbo_oracle as o
from helpers import ROOT, max_err, raw_err

F32 = np.float32


# ----------------------------------------------------------------------------- restatements
def importance_z_two_net(z, weights, n_importance, u=None):
    """isample_from_lineseg(is_only=False) (reference core/utils/ray_utils.py:257-291): the pdf is weights[..., 1:-1] as they
    are (sample_pdf adds 1e-5), no max filter, no alpha_base; then the stable sort of [z, z_samples]."""
    mid = (F32(.5) * (z[:, 1:] + z[:, :-1])).astype(F32)
    zs = o.sample_pdf_det(mid, weights[:, 1:-1], n_importance, u)
    cat = np.concatenate([z, zs], -1)
    idx = np.argsort(cat, -1, kind='stable')
    return np.take_along_axis(cat, idx, -1), zs, idx


def render_two_net(coarse, fine, ray_batch, skts, bones, cyls, cams, n_uniques, S, Sf, near_far=None):
    """render_rays with a separate fine network (reference raycasters.py:330-377): `coarse` on the S coarse samples, the
    two-network pdf, `fine` on all S + Sf sorted samples, composited as they are (no merge of coarse and fine raw)."""
    rays_o, rays_d = ray_batch[:, 0:3], ray_batch[:, 3:6]
    if near_far is None:
        near, far = ray_batch[:, 6:7], ray_batch[:, 7:8]
        if isinstance(coarse, o.DanboOracle):
            near, far = coarse.near_far(rays_o, rays_d, cyls, skts, near, far)
        else:
            near, far = o.near_far_cylinder(rays_o, rays_d, cyls, near, far, None)
    else:
        near, far = near_far
    z = o.coarse_z(near, far, S)
    B = coarse.cfg['density_scale']
    raw, _ = coarse.forward(o.sample_points(rays_o, rays_d, z), rays_d, skts, bones, cams, n_uniques)
    out0 = o.composite(raw, z, rays_d, B)
    z_all, z_fine, order = importance_z_two_net(z, out0['weights'], Sf)
    raw_f, enc_f = fine.forward(o.sample_points(rays_o, rays_d, z_all), rays_d, skts, bones, cams, n_uniques)
    out = o.composite(raw_f, z_all, rays_d, B)
    return dict(rgb_map=out['rgb_map'], disp_map=out['disp_map'], acc_map=out['acc_map'], alpha=out['alpha'], T_i=out['weights'],
                rgb0=out0['rgb_map'], disp0=out0['disp_map'], acc0=out0['acc_map'], alpha0=out0['alpha'], z_coarse=z,
                z_fine=z_fine, z_sorted=z_all, sorted_idxs=order, raw_coarse=raw, raw_fine=raw_f, enc_fine=enc_f,
                near=near, far=far)


def two_oracles(cfg_name, seeds=(3, 4), n_framecodes=20):
    from core.utils import synthetic as syn
    cfg = syn.model_config(cfg_name)
    rest = syn.rest_pose(cfg["rest_scale"])
    sds = [syn.make_state_dict(cfg, seed=s, n_framecodes=n_framecodes, rest=rest) for s in seeds]
    cls = o.DanboOracle if cfg["nerf_type"] == "danbo" else o.AnerfOracle
    return cfg, rest, sds, [cls(cfg, sd, rest) for sd in sds]


# ----------------------------------------------------------------------------- the pdf
def test_two_net_pdf_is_the_plain_interior_weights():
    rng = np.random.default_rng(0)
    R, S, Sf = 64, 16, 8
    z = np.sort(rng.uniform(2, 5, size=(R, S)).astype(F32), -1)
    w = (rng.uniform(size=(R, S)) ** 4).astype(F32)
    z_all, zf, idx = importance_z_two_net(z, w, Sf)
    # the cdf the inverse walks is the normalised cumulative sum of w[1:-1] + 1e-5
    dw = (w[:, 1:-1] + F32(1e-5)).astype(F32)
    cdf = np.cumsum(dw / dw.sum(-1, keepdims=True), -1)
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    assert np.all(zf >= mid[:, :1] - 1e-6) and np.all(zf <= mid[:, -1:] + 1e-6)
    # a sample drawn at u lies in the bin whose cdf interval holds u
    u = o.torch_linspace01(Sf)
    for r in range(R):
        b = np.searchsorted(np.concatenate([[0.], cdf[r]]), u, side='right') - 1
        b = np.clip(b, 0, S - 2)
        assert np.all(zf[r] >= mid[r, np.maximum(b, 0)] - 1e-5)
    assert np.array_equal(np.take_along_axis(np.concatenate([z, zf], -1), idx, -1), z_all)
    # ... and differs from the single-network pdf (max filter + alpha_base)
    _, zf1, _ = o.importance_z(z, w, Sf)
    assert max_err(zf, zf1) > 1e-3
    # the weight of the first and of the last coarse sample take no part
    w2 = w.copy()
    w2[:, 0] = 7.0
    w2[:, -1] = 9.0
    assert np.array_equal(importance_z_two_net(z, w2, Sf)[1], zf)


def test_host_build_of_the_two_network_importance_ray(tmp_path):
    """importance_ray<true> of csrc/sample_math.hpp -- the code the gfx950 importance kernels inline -- compiled for the host
    (g++ -ffp-contract=off, as tests/host_emu) against the restatement; importance_ray<> with no argument stays the
    single-network form"""
    src = tmp_path / "two_net_emu.cpp"
    hpp = os.path.join(ROOT, "danbo-pytorch_amd", "csrc", "sample_math.hpp")
    src.write_text('#include "%s"\nusing namespace danbo;\nextern "C" {\n'
                   'void emu_importance(const float* z, const float* w, int R, int S, int Sf, const float* u, int two, float* cdf,\n'
                   '                    float* zf, float* zs, int32_t* idx) {\n'
                   '    for (int r = 0; r < R; ++r) {\n'
                   '        const float* ur = u ? u + (long)r * Sf : nullptr;\n'
                   '        if (two) importance_ray<true>(z + (long)r * S, w + (long)r * S, S, Sf, ur, cdf, zf + (long)r * Sf,\n'
                   '                                      zs + (long)r * (S + Sf), idx + (long)r * (S + Sf));\n'
                   '        else importance_ray(z + (long)r * S, w + (long)r * S, S, Sf, ur, cdf, zf + (long)r * Sf,\n'
                   '                            zs + (long)r * (S + Sf), idx + (long)r * (S + Sf));\n'
                   '    }\n}\n}\n' % hpp)
    so = tmp_path / "libtwo_net_emu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", str(so), str(src)])
    import ctypes
    lib = ctypes.CDLL(str(so))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rng = np.random.default_rng(1)
    for S, Sf in ((7, 3), (48, 16), (96, 48)):
        R = 40
        z = np.sort(rng.uniform(2, 5, size=(R, S)).astype(F32), -1)
        # the two-network pdf has no alpha_base: bins of weight ~1e-5 make t = (u - c0) / (c1 - c0) flip bins on the last bit of
        # a differently ordered sum -- weights bounded away from 0 keep the comparison about the arithmetic
        w = (0.02 + rng.uniform(size=(R, S)) ** 4).astype(F32)
        for two in (1, 0):
            zf = np.empty((R, Sf), F32)
            zs = np.empty((R, S + Sf), F32)
            idx = np.empty((R, S + Sf), np.int32)
            cdf = np.empty(S + 1, F32)
            lib.emu_importance(P(z), P(w), R, S, Sf, None, two, P(cdf), P(zf), P(zs), P(idx))
            ref_all, ref_f, ref_idx = (importance_z_two_net if two else o.importance_z)(z, w, Sf)
            assert max_err(zf, ref_f) < 1e-4 and np.mean(np.abs(zf - ref_f)) < 2e-6, (S, Sf, two)
            cat = np.concatenate([z, zf], -1)
            assert np.array_equal(zs, np.sort(cat, -1))
            assert np.array_equal(idx.astype(np.int64), np.argsort(cat, -1, kind="stable"))


# ----------------------------------------------------------------------------- composed renders
def _scene_rays(syn, n_poses=2, n_per=24, seed=5):
    scene = syn.make_scene(n_poses=n_poses, H=64, W=64, n_views=n_poses, pose_seed=seed)
    ro, rd, pose = [], [], []
    for p in range(n_poses):
        a, b = scene["rays"][p]
        H, W = scene["H"], scene["W"]
        js, is_ = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        sel = ((np.abs(is_ - W / 2) < W * 0.22) & (np.abs(js - H / 2) < H * 0.40)).reshape(-1)
        idx = np.sort(np.random.default_rng(100 + p).choice(np.nonzero(sel)[0], size=n_per, replace=False))
        ro.append(a[idx]); rd.append(b[idx]); pose += [p] * n_per
    return scene, np.concatenate(ro), np.concatenate(rd), np.array(pose)


@pytest.mark.parametrize("cfg_name", ["anerf_base", "danbo_base"])
def test_composed_two_net_render_uses_each_network_where_the_reference_does(cfg_name):
    from core.utils import synthetic as syn
    cfg, rest, sds, (orc_c, orc_f) = two_oracles(cfg_name)
    scene, ro, rd, pose = _scene_rays(syn)
    rb = syn.ray_batch(ro, rd)
    cams = (np.arange(len(pose)) % 7).astype(np.int64)
    args = (rb, scene["skts"][pose], scene["bones"][pose], scene["cyls"][pose], cams, 2, 12, 6)
    a = render_two_net(orc_c, orc_f, *args)
    assert 0.05 < float(a["acc_map"].mean()) and np.all(np.isfinite(a["rgb_map"]))
    # the coarse maps: the coarse network alone, as its single-network render's coarse maps
    single = orc_c.render(*args[:6], N_samples=12, N_importance=6)
    for k in ("rgb0", "acc0", "alpha0"):
        assert np.array_equal(a[k], single[k]), k
    # the fine maps: the fine network on the merged depths
    assert max_err(a["rgb_map"], single["rgb_map"]) > 1e-3
    b = render_two_net(orc_c, orc_c, *args)
    assert max_err(a["rgb_map"], b["rgb_map"]) > 1e-3 and np.array_equal(a["rgb0"], b["rgb0"])


# ----------------------------------------------------------------------------- the reference
# The reference's package is also called `core`: it runs in a child process (as oracle/gen_golden.py does in
# tests/test_golden_recipe.py), which writes its maps and bounds to an .npz this process compares against.
S_REF, SF_REF = 12, 6
CONFIGS = {"anerf_base": "configs/h36m_zju/anerf_base.txt", "danbo_base": "configs/h36m_zju/danbo_base.txt"}


def _reference_child(cfg_name, out):
    import importlib.util
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    spec = importlib.util.spec_from_file_location("two_net_synthetic", os.path.join(ROOT, "danbo-pytorch_amd", "core", "utils",
                                                                                    "synthetic.py"))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    import ref_harness as rh
    args = rh.parse_reference_config(CONFIGS[cfg_name])
    args.single_net = False          # (a store_true flag: no argv spelling switches it off)
    args.N_samples, args.N_importance = S_REF, SF_REF
    cfg = syn.model_config(cfg_name)
    rest = syn.rest_pose(cfg["rest_scale"])
    with contextlib.redirect_stdout(io.StringIO()):
        caster, _, kw_test = rh.build_reference_caster(args, rest, 20, tempfile.mkdtemp())
    assert caster.network_fine is not caster.network and not caster.single_net
    Tt = lambda x, dt=torch.float32: torch.tensor(np.asarray(x), dtype=dt)  # noqa: E731
    for net, seed in ((caster.network, 3), (caster.network_fine, 4)):
        sd = syn.make_state_dict(cfg, seed=seed, n_framecodes=20, rest=rest)
        net.load_state_dict({k: Tt(v) for k, v in sd.items()}, strict=True)
    caster.eval()
    scene, ro, rd, pose = _scene_rays(syn)
    rb = syn.ray_batch(ro, rd)
    kps, skts, bones, cyls = (scene[k][pose] for k in ("kps", "skts", "bones", "cyls"))
    cams = (np.arange(len(pose)) % 7).astype(np.int64)
    kw = {k: v for k, v in kw_test.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    with torch.no_grad():
        ref = caster(Tt(rb), N_samples=S_REF, kp_batch=Tt(kps), skts=Tt(skts), cyls=Tt(cyls), bones=Tt(bones),
                     cams=Tt(cams, torch.long), N_importance=SF_REF, N_uniques=2, **kw)
        near, far = caster.get_near_far(Tt(ro), Tt(rd), Tt(cyls), near=Tt(rb[:, 6:7]), far=Tt(rb[:, 7:8]), skts=Tt(skts))
    res = {k: v.numpy() for k, v in ref.items() if torch.is_tensor(v)}
    np.savez(out, near=near.numpy(), far=far.numpy(), **res)


@pytest.mark.parametrize("cfg_name", ["anerf_base", "danbo_base"])
def test_composed_oracle_reproduces_the_reference_two_network_caster(cfg_name, tmp_path):
    import sys
    import ref_harness as rh
    from core.utils import synthetic as syn
    if not rh.reference_available():
        pytest.skip("the reference tree is not on this machine")
    out = str(tmp_path / "ref.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), cfg_name, out], capture_output=True, text=True, timeout=900,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = dict(np.load(out))
    cfg, rest, sds, (orc_c, orc_f) = two_oracles(cfg_name)
    scene, ro, rd, pose = _scene_rays(syn)
    rb = syn.ray_batch(ro, rd)
    skts, bones, cyls = (scene[k][pose] for k in ("skts", "bones", "cyls"))
    cams = (np.arange(len(pose)) % 7).astype(np.int64)
    got = render_two_net(orc_c, orc_f, rb, skts, bones, cyls, cams, 2, S_REF, SF_REF, near_far=(ref["near"], ref["far"]))
    if cfg_name == "anerf_base":        # tests/test_oracle_anerf.py's bounds
        tol = dict(rgb_map=1e-3, acc_map=1e-3, rgb0=5e-4, acc0=5e-4)
        psnr_min = 65.0
    else:                               # tests/test_oracle_golden.py's
        tol = {k: 5e-4 for k in ("rgb_map", "acc_map", "alpha", "T_i", "rgb0", "acc0", "alpha0")}
        psnr_min = 70.0
    for k, t in tol.items():
        assert max_err(got[k], ref[k]) < t, (k, max_err(got[k], ref[k]))
    assert o.psnr(got["rgb_map"], ref["rgb_map"]) > psnr_min
    assert raw_err(got["disp0"], ref["disp0"]) < 5e-4
    assert 0.05 < float(ref["acc_map"].mean())
    # the fine network makes the final maps: the coarse network on the same depths does not reproduce them
    single = render_two_net(orc_c, orc_c, rb, skts, bones, cyls, cams, 2, S_REF, SF_REF, near_far=(ref["near"], ref["far"]))
    assert max_err(single["rgb_map"], ref["rgb_map"]) > 1e-3


if __name__ == "__main__":
    import sys
    _reference_child(sys.argv[1], sys.argv[2])
