"""danbo_bone_cull_rays (csrc/k_cull_rays.hip, include/danbo_cull.h): depths, in-volume words and compacted rows for the listed rays
of a frame only, against the kernels it stands in for -- danbo_ray_bone_mask + danbo_flat_rays + danbo_coarse_samples +
danbo_bone_cull on the same inputs.  Everything here is bit for bit: the per-sample arithmetic is the same device code.

Scene: core.utils.synthetic.make_scene at 32 x 32 rays (R = 1024), one pose, the danbo_base synthetic weights; (S, Sf) = (48, 16),
(10, 4) (S no multiple of 4) and (96, 32) (the unfused composites)."""
import pytest
import torch

import isa
from helpers import ADDR as P, T     # P: an address no check follows -- the calls that take it return before any launch

DEV = "cuda:0"
SHAPES = [(48, 16), (10, 4), (96, 32)]
CANARY_F, CANARY_I = -777.25, -12345
KEYS = ("rgb_map", "disp_map", "acc_map", "alpha", "T_i", "rgb0", "disp0", "acc0", "alpha0")


@pytest.fixture(scope="module")
def world():
    """engine, rays, bounds, ray mask and flags of the scene -- made once, read only"""
    from core import hip_ops as ops
    from core.render_engine import DanboEngine
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import bone_align_transforms
    cfg = syn.model_config("danbo_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd = syn.make_state_dict(cfg, seed=1, n_framecodes=8, rest=rest)
    scene = syn.make_scene(n_poses=1, H=32, W=32, n_views=2, pose_seed=1)
    ro, rd = scene["rays"][0]
    eng = DanboEngine(cfg, {k: T(v) for k, v in sd.items()}, T(bone_align_transforms(rest)))
    eng.refresh()
    args = (T(ro), T(rd), T(scene["skts"]), T(scene["bones"]), T(scene["cyls"]), torch.zeros(len(ro), dtype=torch.int64, device=DEV))
    near, far = eng.near_far(args[0], args[1], args[4], args[2])
    rm = ops.ray_bone_mask(args[0], args[1], args[2], eng.align, eng.axis_scale, near, far, want_flat=True)
    R = args[0].shape[0]
    assert R == 1024 and args[2].shape[0] == 1
    flat = rm[3] != 0
    assert int(flat.sum()) > 100 and int((~flat).sum()) > 100          # both kinds of ray
    return dict(ops=ops, eng=eng, args=args, near=near, far=far, rm=rm, R=R, passes={})


def passes_of(world, S, Sf):
    """the reference of one (S, Sf), made once: the frame's ray list, and per pass (coarse, fine) the depths of every ray and the
    existing cull's words / rows for them"""
    if (S, Sf) not in world["passes"]:
        ops, eng, args, rm = world["ops"], world["eng"], world["args"], world["rm"]
        fr = ops.flat_rays(rm[1], rm[3], S, Sf)
        z = ops.coarse_samples(world["near"], world["far"], S)
        z_fine = eng.render(*args, S, Sf, keep=True)["z_fine"].contiguous()         # the importance depths of EVERY ray
        ref = {}
        for tag, zz in (("coarse", z), ("fine", z_fine)):
            bits, lst, cnt = ops.bone_cull(ops.Geometry(args[0], args[1], args[2], eng.align, eng.axis_scale, z=zz, ray_mask=rm[:3]), True)
            ref[tag] = dict(z=zz, bits=bits, rows=lst[:int(cnt.item())].long())
        assert ref["coarse"]["rows"].numel() > 0 and ref["fine"]["rows"].numel() > 0
        world["passes"][(S, Sf)] = (fr, ref)
    return world["passes"][(S, Sf)]


def cull_rays(world, ray_list, ray_count, z, coarse, rm=None, rays_per_wg=0, G=1, check=True):
    """danbo_bone_cull_rays on caller-made buffers full of canaries -> (status, z, bits, list, count)"""
    from core import _hip
    ops, eng, args = world["ops"], world["eng"], world["args"]
    rm = world["rm"] if rm is None else rm
    R, S = z.shape
    z = torch.full_like(z, CANARY_F) if coarse else z.clone()
    bits = torch.full((R * S,), CANARY_I, dtype=torch.int32, device=DEV)
    lst = torch.full((R * S,), CANARY_I, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = _hip.ptr
    near, far = (world["near"].reshape(-1).contiguous(), world["far"].reshape(-1).contiguous()) if coarse else (None, None)
    rc = _hip.lib().danbo_bone_cull_rays(p(ray_list), p(ray_count), p(rm[0]), p(rm[1]), p(rm[2]), p(args[0]), p(args[1]), R, S, G,
                                         p(args[2]), p(eng.align), p(eng.axis_scale), p(near), p(far), p(z), rays_per_wg, p(bits),
                                         p(lst), p(cnt), _hip.stream())
    torch.cuda.synchronize()
    if check:
        assert rc == 0
    return rc, z, bits, lst, cnt


def check_against_reference(world, ref, rays, got, S, coarse):
    """rays: the listed rays (long, no duplicates).  Listed rays: depths and words equal the reference's; every other ray: canaries;
    the rows are the reference's rows of the listed rays, each ray's rows contiguous with ascending sample index"""
    _, z, bits, lst, cnt = got
    R = world["R"]
    listed = torch.zeros(R, dtype=torch.bool, device=DEV)
    listed[rays] = True
    bits, ref_bits = bits.view(R, S), ref["bits"].view(R, S)
    assert torch.equal(bits[listed], ref_bits[listed])
    assert bool((bits[~listed] == CANARY_I).all())
    if coarse:
        assert torch.equal(z[listed].view(torch.int32), ref["z"][listed].view(torch.int32))
        assert bool((z[~listed] == CANARY_F).all())
    else:
        assert torch.equal(z.view(torch.int32), ref["z"].view(torch.int32))        # an input: untouched
    want = ref["rows"][listed[ref["rows"] // S]]
    n = int(cnt.item())
    assert n == want.numel()
    rows = lst[:n].long()
    assert torch.equal(torch.sort(rows).values, torch.sort(want).values)
    assert bool((lst[n:] == CANARY_I).all())
    if n > 1:
        ray, nxt = rows[:-1] // S, rows[1:] // S
        assert bool(((ray != nxt) | (rows[1:] > rows[:-1])).all())                   # ascending inside a ray
        assert int((ray != nxt).sum()) + 1 == int(torch.unique(rows // S).numel())    # one run per ray: contiguous
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("S,Sf", SHAPES)
def test_listed_cull_equals_the_existing_kernels_on_the_listed_rays(world, S, Sf):
    fr, ref = passes_of(world, S, Sf)
    R = world["R"]
    n_list = int(fr["ray_count"].item())
    frame = fr["ray_list"][:n_list].long()
    assert 100 < n_list < R
    every = torch.randperm(R, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(torch.int32)
    all_count = torch.tensor([R], dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    for tag, coarse, s in (("coarse", True, S), ("fine", False, Sf)):
        zz = ref[tag]["z"]
        # the frame's own list, at the library's rays per workgroup and at one that leaves a ragged last workgroup
        for rpw in (0, 7):
            n = check_against_reference(world, ref[tag], frame, cull_rays(world, fr["ray_list"], fr["ray_count"], zz, coarse, rays_per_wg=rpw), s, coarse)
            assert n > 0
        # every ray listed (no ray of constants), in a scrambled order; 1024 rays are no multiple of 24 rays per workgroup
        for rpw in (0, 24):
            n = check_against_reference(world, ref[tag], every.long(), cull_rays(world, every, all_count, zz, coarse, rays_per_wg=rpw), s, coarse)
            assert n == ref[tag]["rows"].numel()
        # an empty list: nothing is written anywhere
        _, z, bits, lst, cnt = cull_rays(world, fr["ray_list"], zero, zz, coarse)
        assert int(cnt.item()) == 0 and bool((bits == CANARY_I).all()) and bool((lst == CANARY_I).all())
        assert bool((z == CANARY_F).all()) if coarse else torch.equal(z, zz)


@pytest.mark.gpu
def test_the_ray_mask_never_changes_the_words_of_the_listed_cull(world):
    """as test_ray_bone_mask_is_conservative_and_never_changes_the_in_volume_mask for k_bone_cull: a tight interval, an interval
    that does not hold the depths (every sample falls back to all bones) and an all-zero mask over such an interval give the words,
    the count and the rows of the correct mask"""
    S, Sf = 48, 16
    fr, ref = passes_of(world, S, Sf)
    ops, eng, args, rm = world["ops"], world["eng"], world["args"], world["rm"]
    frame = fr["ray_list"][:int(fr["ray_count"].item())].long()
    for tag, coarse, s in (("coarse", True, S), ("fine", False, Sf)):
        zz = ref[tag]["z"]
        tight = ops.ray_bone_mask(args[0], args[1], args[2], eng.align, eng.axis_scale, zz.min(1).values, zz.max(1).values)
        wrong = (rm[0], rm[1] + 10.0, rm[2] + 10.0)
        none = (torch.zeros_like(rm[0]), rm[1] + 10.0, rm[2] + 10.0)
        for mask in (tight, wrong, none):
            got = cull_rays(world, fr["ray_list"], fr["ray_count"], zz, coarse, rm=mask)
            check_against_reference(world, ref[tag], frame, got, s, coarse)


@pytest.mark.gpu
@pytest.mark.parametrize("S,Sf", SHAPES)
def test_render_with_the_listed_cull_is_bitwise_the_render_without(world, S, Sf):
    ops, eng, args = world["ops"], world["eng"], world["args"]
    assert eng.cull_listed_rays is True and eng.flat_rays_ok and eng.skip_flat_rays
    calls, real = [], ops.bone_cull_rays
    ops.bone_cull_rays = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        on = eng.render(*args, S, Sf)
    finally:
        ops.bone_cull_rays = real
    assert len(calls) == 2                                     # both passes took the new kernel
    eng.cull_listed_rays = False
    try:
        off = eng.render(*args, S, Sf)
    finally:
        eng.cull_listed_rays = True
    assert set(KEYS) <= set(on) and set(on) == set(off)
    for k in on:
        assert torch.equal(on[k], off[k]), k
    assert float(on["acc_map"].max()) > 0.5
    if (S, Sf) == (48, 16):
        c = eng.render_frame_c(*args, S, Sf)
        assert set(c) == set(on)
        for k in on:
            assert torch.equal(on[k], c[k]), k


@pytest.mark.gpu
def test_more_than_one_pose_is_refused(world):
    fr, ref = passes_of(world, 48, 16)
    rc, z, bits, lst, cnt = cull_rays(world, fr["ray_list"], fr["ray_count"], ref["coarse"]["z"], True, G=2, check=False)
    assert rc == -22
    assert int(cnt.item()) == 0 and bool((bits == CANARY_I).all()) and bool((z == CANARY_F).all())      # before any launch


def test_listed_cull_does_not_spill():
    """both instantiations of k_cull_rays keep everything in registers (the gfx950 ISA of `make build/k_cull_rays.s`)"""
    text = isa.device_asm("k_cull_rays")
    for k in ("k_cull_raysILb1E", "k_cull_raysILb0E"):
        meta = isa.kernel_meta(text, r"\S*" + k + r"\S*", "private_segment_fixed_size")
        assert meta is not None, k
        assert int(meta.group(1)) == 0, (k, meta.group(1))
        body = "\n".join(isa.kernel_body(text, r"_ZN5danbo\S*" + k + r"\S*"))
        assert "scratch_" not in body, k


@pytest.mark.parametrize("kw", [dict(G=2), dict(G=0), dict(R=0), dict(S=0), dict(S=16385), dict(R=1 << 20, S=4096), dict(rpw=-1),
                                dict(ray_list=None), dict(ray_count=None), dict(ray_mask=None), dict(t_lo=None), dict(z=None),
                                dict(bits=None), dict(lst=None), dict(cnt=None), dict(far=None)])
def test_listed_cull_rejects_before_any_launch(kw):
    from core import _hip
    a = dict(ray_list=P, ray_count=P, ray_mask=P, t_lo=P, t_hi=P, o=P, d=P, R=1024, S=48, G=1, skts=P, align=P, scale=P, near=P, far=P,
             z=P, rpw=0, bits=P, lst=P, cnt=P)
    a.update(kw)
    assert _hip.lib().danbo_bone_cull_rays(*a.values(), None) == _hip.C.DANBO_EINVAL
