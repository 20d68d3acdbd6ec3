"""Depth and normal maps on the GPU (danbo_depth_composite_fwd / danbo_depth_normals, core.depth_maps, the engines' depth=True, the
caster's render_depth, run_render --render_depth / --render_normal): both kernels against the serial restatement of
csrc/depth_math.hpp bit for bit and against the float64 statement of tests/depth_ref.py within its bounds, guard words around
every output, a second call, the ray list, rejected arguments, the three engines, the caster's graph and eager routes and the
entry point."""
import os

import numpy as np
import pytest
import torch

import depth_ref as ref
from helpers import DEV, EINVAL, ROOT, entry, T, same_bits
from test_gpu_part_maps import MAPS, S_E2E, SF_E2E, cast, clone, danbo_caster, danbo_engine      # the part-map tests' synthetic builders

pytestmark = pytest.mark.gpu
F32, F64, U = ref.F32, ref.F64, ref.U
N_GUARD = 64          # guard words on either side of an output
N_E2E = S_E2E + SF_E2E        # 12 + 6: the samples of the part-map end-to-end frames


def stream_ptr():
    from core import _hip
    return _hip.stream()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def guarded(n, dtype, fill):
    """-> (whole device buffer with N_GUARD guard elements on either side, the view of the n payload elements)"""
    buf = torch.full((n + 2 * N_GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[N_GUARD:N_GUARD + n]


def intact(buf, fill):
    return bool((buf[:N_GUARD] == fill).all()) and bool((buf[-N_GUARD:] == fill).all())


def gpu_composite(w, z, level, ray_list=None, ray_count=None):
    """the raw C call with guard words around both outputs, which start from the sentinel -> (depth [R], depth_level [R]) numpy"""
    w, z = dev(w), dev(z)
    R, n = w.shape
    fill = float(ref.SENTINEL)
    (buf_d, d), (buf_l, l) = guarded(R, torch.float32, fill), guarded(R, torch.float32, fill)
    lst = None if ray_list is None else dev(np.asarray(ray_list, np.int32))
    cnt = None if ray_count is None else dev(np.array([ray_count], np.int32))
    rc = entry("danbo_depth_composite_fwd")(w.data_ptr(), z.data_ptr(), R, n, float(level), None if lst is None else lst.data_ptr(),
                                            None if cnt is None else cnt.data_ptr(), d.data_ptr(), l.data_ptr(), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(buf_d, fill) and intact(buf_l, fill), "a guard word was overwritten"
    return d.cpu().numpy(), l.cpu().numpy()


def gpu_normals(c, jump, space, with_cast=True, acc_min=0.5, background=1.0):
    """the raw C call on a frames case with guard words around both outputs -> (rgb [N,H,W,3] float32, valid [N,H,W] uint8) numpy"""
    depth, acc, cast, c2w, intr = (dev(c[k]) for k in ("depth", "acc", "cast", "c2w", "intr"))
    N, H, W = depth.shape
    (buf_r, rgb), (buf_v, valid) = guarded(N * H * W * 3, torch.float32, -5.0), guarded(N * H * W, torch.uint8, 0xA5)
    rc = entry("danbo_depth_normals")(depth.data_ptr(), acc.data_ptr(), cast.data_ptr() if with_cast else None, c2w.data_ptr(),
                                      intr.data_ptr(), N, H, W, acc_min, jump, space, background, rgb.data_ptr(), valid.data_ptr(),
                                      stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(buf_r, -5.0) and intact(buf_v, 0xA5), "a guard word was overwritten"
    return rgb.reshape(N, H, W, 3).cpu().numpy(), valid.reshape(N, H, W).cpu().numpy()


# ----------------------------------------------------------------------------- 1. the composite kernel
@pytest.mark.parametrize("level", [0.5, 1.0])
@pytest.mark.parametrize("n", ref.N_CASES)
def test_composite_equals_the_restatement_bitwise(n, level):
    """R = 67 rays of n positions (one partial strip, one full strip, one position into the second strip, the limit) with the edge
    rays of depth_ref.composite_case: all weights +0, acc < level, the prefix exactly equal to the level (0.25 + 0.25, also across
    two strips), weights that sum to exactly 1 under level = 1, a NaN depth under a zero weight.  Bit for bit the restatement's
    result; against float64 within n 2^-24 sum|w z| and inside the acceptance set (depth_ref's head); two calls, the same bits."""
    c = ref.composite_case(n)
    want_d, want_l = ref.composite_expected(n, level)
    got_d, got_l = gpu_composite(c["w"], c["z"], level)
    assert same_bits(got_d, want_d), np.flatnonzero(got_d != want_d)
    assert same_bits(got_l, want_l), np.flatnonzero(got_l.view(np.uint32) != want_l.view(np.uint32))
    d64, _ = ref.depth64(c["w"], c["z"])
    err, bound = np.abs(got_d.astype(F64) - d64), ref.depth_bound(c["w"], c["z"])
    print(f"n = {n}, level = {level}: max |depth - depth64| = {err.max():.3e}, largest err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound) and ref.level_accepts(got_l, c["w"], c["z"], level) == []
    rays, z = c["rays"], c["z"]
    assert same_bits(got_d[rays["all_zero"]], F32(0)) and same_bits(got_l[rays["all_zero"]], F32(0))
    if level == 0.5:
        assert same_bits(got_l[rays["below_level"]], F32(0))
        assert same_bits(got_l[rays["exact_tie"]], z[rays["exact_tie"], 0 if n == 1 else ref.tie_positions(n)[1]])
        if "tie_across_strips" in rays:
            assert same_bits(got_l[rays["tie_across_strips"]], z[rays["tie_across_strips"], 64])
    else:
        assert same_bits(got_l[rays["exact_one"]], z[rays["exact_one"], n - 1]) and same_bits(got_l[rays["exact_tie"]], F32(0))
    again_d, again_l = gpu_composite(c["w"], c["z"], level)          # one repeat, not a stress loop
    assert same_bits(again_d, got_d) and same_bits(again_l, got_l)


@pytest.mark.parametrize("n", [18, 65, 320])
def test_composite_walks_the_ray_list(n):
    """41 of the 67 rays listed in a shuffled order: the listed rays hold the restatement's bits; the outputs of the others still
    hold the sentinel they were pre-set to, and their z rows are NaN -- had they been read, the sentinel would be gone"""
    c = ref.ray_list_case(n)
    got_d, got_l = gpu_composite(c["w"], c["z"], 0.5, c["ray_list"], c["ray_count"])
    want_d, want_l = ref.host_composite(c["w"], c["z"], 0.5, c["ray_list"], c["ray_count"], init=ref.SENTINEL)
    assert same_bits(got_d, want_d) and same_bits(got_l, want_l)
    listed = c["listed"]
    full_d, full_l = ref.composite_expected(n, 0.5)
    assert same_bits(got_d[listed], full_d[listed]) and same_bits(got_l[listed], full_l[listed])
    assert np.all(got_d[~listed] == ref.SENTINEL) and np.all(got_l[~listed] == ref.SENTINEL) and int((~listed).sum()) == 26
    assert np.isnan(c["z"][~listed]).all()
    # a count of 0: nothing is written
    none_d, none_l = gpu_composite(c["w"], c["z"], 0.5, c["ray_list"], 0)
    assert np.all(none_d == ref.SENTINEL) and np.all(none_l == ref.SENTINEL)


def test_python_composite_and_its_flat_argument():
    from core.depth_maps import composite_depth
    c = ref.ray_list_case(65)
    d, l = composite_depth(dev(ref.composite_case(65)["w"]), dev(ref.composite_case(65)["z"]), 0.5)
    want = ref.composite_expected(65, 0.5)
    assert same_bits(d.cpu().numpy(), want[0]) and same_bits(l.cpu().numpy(), want[1])
    flat = dict(ray_list=dev(c["ray_list"]), ray_count=dev(np.array([c["ray_count"]], np.int32)))
    d, l = composite_depth(dev(c["w"]), dev(c["z"]), 0.5, flat=flat)
    want = ref.host_composite(c["w"], c["z"], 0.5, c["ray_list"], c["ray_count"])          # the outputs start from +0
    assert same_bits(d.cpu().numpy(), want[0]) and same_bits(l.cpu().numpy(), want[1])
    assert float(d[dev(~c["listed"])].abs().sum()) == 0. and not bool(torch.signbit(d).any())
    with pytest.raises(ValueError):
        composite_depth(dev(c["w"]), dev(c["z"]), 0.0)
    with pytest.raises(ValueError):
        composite_depth(torch.zeros(2, 321, device=DEV), torch.zeros(2, 321, device=DEV))
    with pytest.raises(ValueError):
        composite_depth(dev(c["w"]), dev(c["z"])[:, :5])


# ----------------------------------------------------------------------------- 2. rejected arguments
def test_rejected_arguments_leave_the_outputs_untouched():
    """every DANBO_EINVAL case of the header on real device buffers: the outputs still hold their sentinel"""
    w, z = dev(ref.composite_case(18)["w"][:4]), dev(ref.composite_case(18)["z"][:4])
    d, l = (torch.full((4,), 77.0, device=DEV) for _ in range(2))
    spare = torch.zeros(8, dtype=torch.int32, device=DEV)
    ptrs = dict(weights=w.data_ptr(), z_sorted=z.data_ptr(), depth=d.data_ptr(), depth_level=l.data_ptr(), ray_list=spare.data_ptr(),
                ray_count=spare.data_ptr())
    call = entry("danbo_depth_composite_fwd")
    assert call(*ref.composite_args(ptrs), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert same_bits(d.cpu().numpy(), ref.composite_expected(18, 0.5)[0][:4])
    d.fill_(77.0), l.fill_(77.0)
    for kw in ref.COMPOSITE_REJECTS:
        assert call(*ref.composite_args(ptrs, **kw), stream_ptr()) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((d == 77.0).all()) and bool((l == 77.0).all())

    c = ref.frames_case()
    depth, acc, c2w, intr = (dev(c[k][:1, :4, :4] if k in ("depth", "acc") else c[k][:1]) for k in ("depth", "acc", "c2w", "intr"))
    depth, acc = depth.contiguous(), acc.contiguous()
    rgb = torch.full((4 * 4 * 3,), 77.0, device=DEV)
    ptrs = dict(depth=depth.data_ptr(), acc=acc.data_ptr(), c2w=c2w.data_ptr(), intr=intr.data_ptr(), out_rgb=rgb.data_ptr())
    call = entry("danbo_depth_normals")
    for kw in ref.NORMALS_REJECTS:
        assert call(*ref.normals_args(ptrs, **kw), stream_ptr()) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((rgb == 77.0).all())
    assert call(*ref.normals_args(ptrs), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((rgb == 77.0).any())


# ----------------------------------------------------------------------------- 3. / 4. the engines
@pytest.fixture(scope="module")
def frame():
    """the 32 x 32 frame of the part-map end-to-end tests (S, Sf = 12, 6), rendered once: plain, keep=True, depth=True"""
    from core.utils import synthetic as syn
    eng = danbo_engine()
    scene = syn.make_scene(n_poses=1, H=32, W=32, n_views=1, pose_seed=40)
    ro, rd = scene["rays"][0]
    assert len(ro) == 1024
    args = (T(ro), T(rd), T(scene["skts"]), T(scene["bones"]), T(scene["cyls"]), torch.zeros(1024, dtype=torch.int64, device=DEV))
    plain = clone(eng.render(*args, S_E2E, SF_E2E))
    keep = clone(eng.render(*args, S_E2E, SF_E2E, keep=True))
    deep = clone(eng.render(*args, S_E2E, SF_E2E, depth=True))
    return dict(eng=eng, scene=scene, rays=(ro, rd), args=args, plain=plain, keep=keep, deep=deep)


def check_identity_and_sum(plain, keep, deep, what):
    """depth=True changes none of the nine maps; depth_map is the float64 sum T_i z_sorted of the keep=True render within
    18 2^-24 sum|w z| (the issue's n 2^-24 sum|w z| at n = S + Sf = 18); depth_med lies in its acceptance set"""
    assert set(deep) == set(plain) | {"depth_map", "depth_med"}
    for k in MAPS:
        assert torch.equal(deep[k], plain[k]) and torch.equal(keep[k], plain[k]), (what, k)
    w, z = keep["T_i"].cpu().numpy(), keep["z_sorted"].cpu().numpy()
    assert w.shape == z.shape == (len(w), N_E2E)
    d64, a64 = ref.depth64(w, z)
    got = deep["depth_map"].cpu().numpy()
    assert got.dtype == F32 and got.shape == (len(w),)
    err = np.abs(got.astype(F64) - d64)
    print(f"{what}: {int((d64 > 0).sum())} rays with depth, max {d64.max():.3f}; max |depth_map - float64| = {err.max():.3e}, "
          f"largest err / bound = {np.max(err / np.maximum(N_E2E * U * a64, 1e-300)):.3f}")
    assert np.all(err <= N_E2E * U * a64) and float(a64.max()) > 0
    assert ref.level_accepts(deep["depth_med"].cpu().numpy(), w, z, 0.5) == []
    return w, z, d64


def test_danbo_engine_depth(frame):
    """the single-network engine on a frame with rays of constants: (i) the nine maps are bit for bit the plain render's, with
    lazy and the rays of constants still on; (ii) depth_map against float64; (iii) the rays of constants have depth exactly +0;
    (iv) where acc > 1e-3, depth / (acc + 1e-10) agrees with 1 / disp_map within 32 x 2^-24, relatively: both are sums of the
    same 18 positive terms w z, each within (1 + 17) 2^-24 of the exact sum whatever its order (one product, at most 17
    additions on a path) -- the composite's own sum and ours, 7 at most here --, and disp_map adds three roundings (acc + 1e-10,
    the quotient, the reciprocal): (7 + 18 + 3) 2^-24 <= 32 x 2^-24."""
    from core import hip_ops as ops
    eng, args, plain, keep, deep = (frame[k] for k in ("eng", "args", "plain", "keep", "deep"))
    w, z, d64 = check_identity_and_sum(plain, keep, deep, "single network")
    near, far = eng.near_far(args[0], args[1], args[4], args[2])
    flat = ops.ray_bone_mask(args[0], args[1], args[2], eng.align, eng.axis_scale, near, far, want_flat=True)[3] != 0
    assert eng.skip_flat_rays and eng.flat_rays_ok and 100 < int(flat.sum()) < 1024
    for k in ("depth_map", "depth_med"):
        v = deep[k][flat]
        assert float(v.abs().sum()) == 0. and not bool(torch.signbit(v).any()), k
    # with the rays of constants switched off every z row exists: the same bits
    eng.skip_flat_rays = False
    try:
        off = eng.render(*args, S_E2E, SF_E2E, depth=True)
    finally:
        eng.skip_flat_rays = True
    for k in MAPS + ("depth_map", "depth_med"):
        assert torch.equal(off[k], deep[k]), k
    kept = eng.render(*args, S_E2E, SF_E2E, depth=True, keep=True)
    dense = eng.render(*args, S_E2E, SF_E2E, depth=True, dense=True)
    for k in ("depth_map", "depth_med"):
        assert torch.equal(kept[k], deep[k]) and torch.equal(dense[k], deep[k]), k
    # (iv)
    acc, disp, depth = (deep[k].double().cpu().numpy() for k in ("acc_map", "disp_map", "depth_map"))
    solid = acc > 1e-3
    assert int(solid.sum()) >= 50 and np.all(z[w > 0] > 0) and np.all(w >= 0)
    q = depth[solid] / (acc[solid] + 1e-10)
    rel = np.abs(q * disp[solid] - 1.0)
    print(f"depth / (acc + 1e-10) against 1 / disp_map on {int(solid.sum())} rays: max relative difference {rel.max():.3e} (bound {32 * U:.3e})")
    assert np.all(q > 1e-10) and np.all(rel <= 32 * U)
    # the median lies on the ray, between its first and last weighted position, and another level gives another map
    med = deep["depth_med"].cpu().numpy()
    has = med > 0
    assert int(has.sum()) >= 50 and np.all(med[has] >= z[has].min(1)) and np.all(med[has] <= z[has].max(1))
    other = eng.render(*args, S_E2E, SF_E2E, depth=True, depth_level=0.9)
    assert torch.equal(other["depth_map"], deep["depth_map"]) and not torch.equal(other["depth_med"], deep["depth_med"])
    # depth combines with a part map: the part map's colours, the same depths
    part = eng.render(*args, S_E2E, SF_E2E, depth=True, part_map="confd")
    assert torch.equal(part["depth_map"], deep["depth_map"]) and torch.equal(part["depth_med"], deep["depth_med"])
    assert torch.equal(part["rgb_map"], eng.render(*args, S_E2E, SF_E2E, part_map="confd")["rgb_map"])


def test_two_net_engine_depth(frame):
    eng_c, eng_f, args = frame["eng"], danbo_engine(seed=4), frame["args"]
    plain = clone(eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E))
    keep = clone(eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E, keep=True))
    deep = eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E, depth=True)
    check_identity_and_sum(plain, keep, deep, "two networks")
    assert int((deep["depth_map"] > 0).sum()) >= 50


def anerf_engine():
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt"))
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=10, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    _, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    sd = syn.make_state_dict(syn.model_config("anerf_base"), 5, 10, syn.rest_pose(0.48))
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    return caster, kw


def test_anerf_engine_depth(frame):
    from core.anerf_engine import AnerfEngine
    caster, kw = anerf_engine()
    eng = caster._engine()
    assert isinstance(eng, AnerfEngine)
    args = tuple(a[:256] if a.shape[0] == 1024 else a for a in frame["args"][:5]) + (None,)
    plain = clone(eng.render(*args, S_E2E, SF_E2E))
    keep = clone(eng.render(*args, S_E2E, SF_E2E, keep=True))
    deep = eng.render(*args, S_E2E, SF_E2E, depth=True)
    check_identity_and_sum(plain, keep, deep, "A-NeRF")
    # and through its caster (the eager route: A-NeRF takes no graph): the two keys arrive
    from core.utils import synthetic as syn
    ro, rd = frame["rays"]
    rb = syn.ray_batch(ro[:256], rd[:256])
    a = clone(cast(caster, kw, frame["scene"], rb))
    b = cast(caster, kw, frame["scene"], rb, render_depth=True)
    assert set(b) == set(a) | {"depth_map", "depth_med"} and all(torch.equal(a[k], b[k]) for k in a)


# ----------------------------------------------------------------------------- 5. the caster
def test_caster_graph_eager_and_whole_image(frame):
    """render_rays(render_depth=True) on the graph path (its own graph: both values join the key) and on the eager path give the
    same bits; every other map is the plain cast's; the whole image in one cast (render_rays_whole) equals the engine's casts
    chunk by chunk"""
    from core import trainer
    from core.utils import synthetic as syn
    caster, kw = danbo_caster()
    scene, (ro, rd) = frame["scene"], frame["rays"]
    rb = syn.ray_batch(ro, rd)
    assert len(rb) <= caster.graph_max_rays and caster.use_graphs
    plain = clone(cast(caster, kw, scene, rb))
    deep = clone(cast(caster, kw, scene, rb, render_depth=True))
    assert len(caster._graphs.graphs) == 2
    level9 = clone(cast(caster, kw, scene, rb, render_depth=True, depth_level=0.9))
    assert len(caster._graphs.graphs) == 3
    replay = cast(caster, kw, scene, rb, render_depth=True)
    assert len(caster._graphs.graphs) == 3
    caster.use_graphs = False
    try:
        eager = clone(cast(caster, kw, scene, rb, render_depth=True))
        both = cast(caster, kw, scene, rb, render_depth=True, render_entropy=True)
    finally:
        caster.use_graphs = True
    assert set(deep) == set(plain) | {"depth_map", "depth_med"}
    for k in plain:
        assert torch.equal(plain[k], deep[k]), k
    for k in deep:
        assert torch.equal(deep[k], eager[k]) and torch.equal(replay[k], eager[k]), k
    assert torch.equal(level9["depth_map"], deep["depth_map"]) and not torch.equal(level9["depth_med"], deep["depth_med"])
    assert torch.equal(both["depth_map"], deep["depth_map"]) and not torch.equal(both["rgb_map"], deep["rgb_map"])
    assert int((deep["depth_map"] > 0).sum()) >= 50 and deep["depth_map"].shape == (1024,)
    # the whole image in one cast against the chunked loop
    n = len(ro)
    exp = lambda x, dt=torch.float32: T(x, dt)[:1].expand(n, *x.shape[1:])  # noqa: E731
    kwargs = dict(kp_batch=exp(scene["kps"]), skts=exp(scene["skts"]), cyls=exp(scene["cyls"]), bones=exp(scene["bones"]),
                  cams=torch.zeros(1, dtype=torch.int64, device=DEV).expand(n), ray_caster=caster, N_samples=S_E2E,
                  N_importance=SF_E2E, render_depth=True, **kw)
    whole = trainer.render(32, 32, 80., chunk=256, rays=(T(ro), T(rd)), **kwargs)
    orig = caster.render_rays_whole
    caster.render_rays_whole = lambda *a, **k: None
    try:
        loop = trainer.render(32, 32, 80., chunk=256, rays=(T(ro), T(rd)), **kwargs)
    finally:
        caster.render_rays_whole = orig
    assert "depth_map" in whole and "depth_med" in whole and set(whole) == set(loop)
    for k in loop:
        assert torch.equal(whole[k], loop[k]), k


# ----------------------------------------------------------------------------- 6. the normals kernel
@pytest.mark.parametrize("kw", ref.NORMAL_VARIANTS, ids=lambda kw: f"jump={kw['jump']}-space={kw['space']}")
def test_normals_equal_the_restatement_bitwise(kw):
    """two frames of 9 x 11 with holes, border pixels and acc below the threshold (depth_ref.frames_case), jump on and off, both
    spaces: bit for bit the restatement's colours and mask, and within normals64's bound of float64"""
    c = ref.frames_case()
    want_rgb, want_valid = ref.normals_expected(kw["jump"], kw["space"])
    rgb, valid = gpu_normals(c, kw["jump"], kw["space"])
    assert same_bits(valid, want_valid)
    assert same_bits(rgb, want_rgb), np.argwhere(rgb.view(np.uint32) != want_rgb.view(np.uint32))[:5]
    r64, ok, bound = ref.normals64(c["depth"], c["acc"], c["cast"], c["c2w"], c["intr"], 0.5, kw["jump"], kw["space"], 1.0)
    err = np.abs(rgb.astype(F64) - r64).max(-1)
    print(f"{kw}: {int(ok.sum())} pixels with a normal, max err {err.max():.3e}, largest err / bound {np.max(err[ok] / bound[ok]):.3f}")
    assert np.array_equal(valid.astype(bool), ok) and np.all(err <= bound)
    again = gpu_normals(c, kw["jump"], kw["space"])
    assert same_bits(again[0], rgb) and same_bits(again[1], valid)
    if kw["space"] == 0 and kw["jump"] == 0:
        no_cast = gpu_normals(c, 0.0, 0, with_cast=False)
        assert same_bits(no_cast[0], ref.normals_expected(0.0, 0, with_cast=False)[0])
        grey = gpu_normals(c, 0.0, 0, background=0.25)[0]
        assert np.all(grey[valid == 0] == 0.25) and same_bits(grey[valid == 1], rgb[valid == 1])


@pytest.mark.parametrize("space", ["camera", "world"])
def test_exact_plane_and_the_python_entry(space):
    """the tilted plane at 9 x 11 through core.depth_maps.normal_maps: the restatement's bits, and the plane's normal within twice
    normals64's bound (tests/test_depth_host.py::test_exact_plane)"""
    from core.depth_maps import normal_maps
    c2w, intr = ref.cameras(2)
    D = ref.plane_depth(intr).astype(F32)
    ones = np.ones_like(D)
    c2w4 = np.concatenate([c2w, np.tile(np.array([0, 0, 0, 1], F32), (2, 1, 1))], 1)
    rgb, valid = normal_maps(dev(D), dev(ones), c2w4, intr[:, :2], centers=intr[:, 2:], space=space, return_valid=True)
    s = 0 if space == "camera" else 1
    want_rgb, want_valid = ref.host_normals(D, ones, None, c2w, intr, 0.5, 0.0, s, 1.0)
    assert same_bits(rgb.cpu().numpy(), want_rgb) and same_bits(valid.cpu().numpy(), want_valid) and bool(valid.all())
    want = ref.PLANE_NORMAL if s == 0 else np.einsum("nij,j->ni", c2w[:, :, :3].astype(F64), ref.PLANE_NORMAL)[:, None, None, :]
    _, _, bound = ref.normals64(D, ones, None, c2w, intr, 0.5, 0.0, s, 1.0)
    err = np.abs(rgb.double().cpu().numpy() - (0.5 * want + 0.5)).max(-1)
    assert np.all(err <= 2 * bound)
    # a cast mask of bools, and the refusals
    mask = torch.ones(2, 9, 11, dtype=torch.bool, device=DEV)
    assert torch.equal(normal_maps(dev(D), dev(ones), c2w4, intr[:, :2], centers=intr[:, 2:], cast_mask=mask, space=space), rgb)
    with pytest.raises(ValueError):
        normal_maps(dev(D), dev(ones), c2w4, intr[:, :2], space="object")
    with pytest.raises(ValueError):
        normal_maps(dev(D), dev(ones), c2w4, intr[:, :2], jump=-1.0)
    with pytest.raises(ValueError):
        normal_maps(dev(D), dev(ones)[:, :4], c2w4, intr[:, :2])


# ----------------------------------------------------------------------------- 7. the entry point
def test_run_render_writes_depth_and_normal(tmp_path):
    """train -> checkpoint -> run_render --render_depth --render_normal on the synthetic source: the three files with the stated
    shapes and dtypes; image.npy, acc.npy and bboxes.npy are those of the run without the flags"""
    import run_nerf
    import run_render
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "1000", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "val", "--render_res", "32", "32", "--white_bkgd"]
    out = tmp_path / "out"
    run_render.run_render(base + ["--runname", "plain"])
    seen, orig = [], run_render.save_depth_maps

    def spy(args, basedir, geo, accs, render_data, device):
        seen.append((geo, render_data))
        return orig(args, basedir, geo, accs, render_data, device)
    run_render.save_depth_maps = spy
    try:
        rgbs, accs, _, _ = run_render.run_render(base + ["--runname", "geo", "--render_depth", "--render_normal", "--normal_acc_min", "0.01"])
    finally:
        run_render.save_depth_maps = orig
    n = len(rgbs)
    for name in ("image.npy", "acc.npy"):
        assert same_bits(np.load(out / "geo" / name), np.load(out / "plain" / name)), name
    assert (out / "geo" / "bboxes.npy").read_bytes() == (out / "plain" / "bboxes.npy").read_bytes()
    assert not (out / "plain" / "depth.npy").exists() and not (out / "plain" / "normal.npy").exists()
    depth, med, normal = (np.load(out / "geo" / f) for f in ("depth.npy", "depth_med.npy", "normal.npy"))
    assert depth.shape == med.shape == (n, 32, 32) and depth.dtype == med.dtype == F32
    assert normal.shape == (n, 32, 32, 3) and normal.dtype == np.uint8
    acc = accs[..., 0]
    print(f"run_render: acc max {acc.max():.3f}, depth max {depth.max():.3f}, pixels with a normal: {int((normal != 255).any(-1).sum())}")
    assert np.isfinite(depth).all() and depth.min() >= 0 and depth.max() > 0
    assert np.all(depth[acc == 0] == 0) and np.all(med[acc < 0.5 - 1e-5] == 0)
    # the six-tuple of render_path, and normal.npy from it: the restatement on the saved depth and the acc frames with every
    # frame's c2w, focal and centre, quantised like image.npy
    from core.depth_maps import camera_rows
    (geo, render_data), = seen
    assert set(geo) == {"depth", "depth_med", "cast"} and geo["cast"].dtype == bool and geo["cast"].shape == (n, 32, 32)
    assert same_bits(geo["depth"], depth) and not geo["depth"][~geo["cast"]].any() and not acc[~geo["cast"]].any()
    H, W, focals = render_data["hwf"]
    c2w, intr = camera_rows(render_data["render_poses"], focals, render_data["centers"], n, H, W, "cpu")
    want, valid = ref.host_normals(depth, acc, geo["cast"], c2w.numpy(), intr.numpy(), 0.01, 0.0, 0, 1.0)
    assert same_bits(normal, (want * 255).astype(np.uint8)) and int(valid.sum()) == int((normal != 255).any(-1).sum())
    # the same frames through the world-space option, on device frames (--eval_device): same depth, other normals
    run_render.run_render(base + ["--runname", "world", "--render_depth", "--render_normal", "--normal_acc_min", "0.01", "--normal_space", "world",
                                  "--eval_device"])
    assert same_bits(np.load(out / "world" / "depth.npy"), depth) and same_bits(np.load(out / "world" / "depth_med.npy"), med)
    world = np.load(out / "world" / "normal.npy")
    assert np.array_equal((world != 255).any(-1), (normal != 255).any(-1))
    if (normal != 255).any():
        assert not np.array_equal(world, normal)
