"""GPU tests of the bone-assignment maps (--render_confd / --render_entropy): the per-sample colouring kernel against
core/networks/misc.py's torch functions and the reference's golden colours, the colour composite against its float64 sum, and the
render -- engine, caster, entry point, two networks -- against a torch restatement built from the very logits the kernels read.

Bounds (none of them taken from what the kernels give):
  * 'confd' colours are exact: an arg-max and a table look-up.
  * 'entropy' colours: 1e-5 against float64 -- 24 terms p log(p + eps) with few-ulp exp / log, sum p = 1, |log| <= 16.2, a division
    by ln 24: 1 - 2e-6, the bound leaves 5 - 8 x.
  * the composite of N terms with sum w c <= 1: products and sums rounded to fp32, N 2^-24 sum |terms|; 2e-5 covers the kernel
    tests' 320 terms (1.9e-5), the 18-sample frames of the end-to-end tests get their own N 2^-24 = 1.1e-6 (+ the colours' 1e-5
    under 'entropy', their weights summing to at most 1)."""
import math
import os

import numpy as np
import pytest
import torch

import danbo_oracle as o
from helpers import ROOT, golden, T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAPS = ("rgb_map", "disp_map", "acc_map", "alpha", "T_i", "rgb0", "disp0", "acc0", "alpha0")
OTHERS = tuple(k for k in MAPS if k not in ("rgb_map", "rgb0"))
ENTROPY_TOL = 1e-5
COMPOSITE_TOL = 2e-5
S_E2E, SF_E2E = 12, 6
E2E_SUM_TOL = (S_E2E + SF_E2E) * 2.0 ** -24 * 1.01          # N 2^-24 sum |terms|, sum w <= 1 up to its own rounding


def clone(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


def mask_of(bits):
    """in-volume words [n] int32 -> bool [n, 24]"""
    return ((bits.reshape(-1, 1).long() >> torch.arange(24, device=bits.device)) & 1).bool()


def colour_ref(logits, mode, mask=None):
    """float64 colours [n,3] of float32 logits [n,24]: get_confidence_rgb itself (an arg-max: exact) / get_entropy_rgb's formula in
    float64; mask (valid_only): -inf in the masked logits, p = 0 there, a row with no bone at all gives 0."""
    from core.networks.misc import get_confidence_rgb
    x = logits.double().clone()
    if mask is not None:
        x[~mask] = -math.inf
    some = torch.ones(len(x), dtype=torch.bool, device=x.device) if mask is None else mask.any(-1)
    if mode == "confd":
        c = get_confidence_rgb(x.float()).double()
    else:
        e = torch.exp(x - x.max(-1, keepdim=True).values)
        p = e / e.sum(-1, keepdim=True)
        t = -(p * (p + 1e-7).log()).sum(-1) / math.log(24)
        c = torch.stack([t, torch.zeros_like(t), 1 - t], -1)
    c[~some] = 0.
    return c


def check_colours(got, want, mode, what):
    err = float((got.double() - want).abs().max()) if len(got) else 0.
    print(f"part_colors {mode} {what}: max |kernel - reference| = {err:.3e}")
    if mode == "confd":
        assert torch.equal(got.double(), want), what
    else:
        assert err <= ENTROPY_TOL, (what, err)


# ----------------------------------------------------------------------------- kernel 1
def random_logits(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0., 3., size=(n, 24)).astype(np.float32)
    for r in range(0, n, 7):                 # exact ties of the largest logit: below and above its index, and a three-way tie
        j = int(x[r].argmax())
        x[r, (j + 5) % 24] = x[r, j]
        if r % 14 == 0:
            x[r, (j + 11) % 24] = x[r, j]
    return x


@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_part_colors_on_the_golden_logits(mode):
    from core import hip_ops as ops
    g = golden("confd_colours")
    x = T(g["confd"].reshape(-1, 24))
    assert len(x) == 30
    rgb = torch.full((30, 3), math.nan, device=DEV)
    ops.part_colors(x, mode, rgb)
    check_colours(rgb, colour_ref(x, mode), mode, "golden rows against the restatement")
    ref = T(g["confidence_rgb" if mode == "confd" else "entropy_rgb"].reshape(-1, 3))
    check_colours(rgb, ref.double(), mode, "golden rows against the reference's colours")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_part_colors_dense_listed_and_masked(mode, n):
    from core import hip_ops as ops
    x = T(random_logits(n, 100 + n))
    rng = np.random.default_rng(n)
    # dense: row i is sample i
    rgb = torch.full((n, 3), math.nan, device=DEV)
    ops.part_colors(x, mode, rgb)
    check_colours(rgb, colour_ref(x, mode), mode, f"n={n} dense")
    # through a permuted list into M > n samples, with a device count below the capacity
    M, cnt = n + 7, (3 * n) // 4
    lst = rng.permutation(M)[:n].astype(np.int32)
    rgb = torch.full((M, 3), math.nan, device=DEV)
    ops.part_colors(x, mode, rgb, T(lst, torch.int32), T([cnt], torch.int32))
    idx = torch.tensor(lst[:cnt].astype(np.int64), device=DEV)
    check_colours(rgb[idx], colour_ref(x[:cnt], mode), mode, f"n={n} listed")
    untouched = torch.ones(M, dtype=torch.bool, device=DEV)
    untouched[idx] = False
    assert int(untouched.sum()) == M - cnt and bool(torch.isnan(rgb[untouched]).all())       # rows beyond the count, unlisted samples
    # valid_only: the words are indexed by SAMPLE; some of them are empty
    words = rng.integers(0, 1 << 24, size=M).astype(np.int64)
    words[rng.random(M) < 0.2] = 0
    words[rng.random(M) < 0.2] &= 0x00F00F
    bits = T(words, torch.int32)
    rgb = torch.full((M, 3), math.nan, device=DEV)
    ops.part_colors(x, mode, rgb, T(lst, torch.int32), T([cnt], torch.int32), bits=bits, valid_only=True)
    m = mask_of(bits)[idx]
    check_colours(rgb[idx], colour_ref(x[:cnt], mode, m), mode, f"n={n} valid_only")
    if cnt:
        empty = ~m.any(-1)
        assert n < 20 or int(empty.sum()) > 0
        assert float(rgb[idx][empty].abs().sum()) == 0.
    assert bool(torch.isnan(rgb[untouched]).all())


# ----------------------------------------------------------------------------- kernel 2
def composite_case(R, S, Sf, seed, identity=False):
    rng = np.random.default_rng(seed)
    N = S + Sf
    ca = rng.random((R, S, 3)).astype(np.float32)
    cb = rng.random((R, max(Sf, 1), 3)).astype(np.float32)[:, :Sf]
    za, zb = np.sort(rng.random((R, S)).astype(np.float32), -1), np.sort(rng.random((R, Sf)).astype(np.float32), -1)
    idx = np.argsort(np.concatenate([za, zb], -1), -1, kind="stable").astype(np.int32)       # the stable merge of two sorted rows
    if identity:
        idx = np.tile(np.arange(N, dtype=np.int32), (R, 1))
    w = rng.random((R, N)).astype(np.float32)
    w[rng.random((R, N)) < 0.5] = 0.
    w = (w / np.maximum(w.sum(-1, keepdims=True), 1e-6) * rng.uniform(0.3, 1.0, size=(R, 1))).astype(np.float32)
    assert float(w.sum(-1).max()) <= 1.0 + 1e-6
    bits = rng.integers(1, 1 << 24, size=(R, N)).astype(np.int64)       # words by SOURCE sample: [coarse | fine]
    none = rng.random((R, N)) < 0.25
    bits[none] = 0
    col = np.concatenate([ca, cb], 1)
    col[none] = np.nan                                                   # no colour row: must not be read
    # the weight of such a sample is +0 (what the render guarantees) for half of them; the others keep theirs and must still
    # contribute nothing
    pos = np.argsort(idx, -1)                                            # position of every source sample in the sorted order
    zero_w = none & (rng.random((R, N)) < 0.5)
    w[np.nonzero(zero_w)[0], pos[zero_w]] = 0.
    src = np.take_along_axis(col, idx[..., None].astype(np.int64), 1).astype(np.float64)
    live = np.take_along_axis(~none, idx.astype(np.int64), 1)
    want = np.where(live[..., None], w[..., None].astype(np.float64) * np.nan_to_num(src), 0.).sum(1)
    return dict(ca=col[:, :S], cb=col[:, S:], idx=idx, w=w, bits_a=bits[:, :S], bits_b=bits[:, S:], want=want)


@pytest.mark.parametrize("S,Sf", [(5, 3), (48, 16), (64, 64), (256, 64), (12, 0)])
@pytest.mark.parametrize("R", [1, 3, 130])
def test_composite_colors_against_the_float64_sum(R, S, Sf):
    from core import hip_ops as ops
    identity = Sf == 0
    c = composite_case(R, S, Sf, 1000 * R + S, identity)
    ca, w = T(c["ca"]), T(c["w"])
    kw = dict(bits_a=T(c["bits_a"].reshape(-1), torch.int32))
    if not identity:
        kw.update(rgb_b=T(c["cb"]), idx=T(c["idx"], torch.int32), bits_b=T(c["bits_b"].reshape(-1), torch.int32))
    out = ops.composite_colors(ca, w, **kw)
    again = ops.composite_colors(ca, w, **kw)
    assert bool(torch.isfinite(out).all())                 # the NaN rows of the samples without a colour were not read
    err = float((out.double().cpu() - torch.tensor(c["want"])).abs().max())
    print(f"composite_colors R={R} S={S} Sf={Sf}: max |kernel - float64 sum| = {err:.3e}")
    assert err <= COMPOSITE_TOL
    assert torch.equal(out, again)
    # a ray list holding a subset: the other rows keep their sentinel
    rng = np.random.default_rng(R + S)
    listed = np.nonzero(rng.random(R) < 0.6)[0].astype(np.int32)
    lst = np.full(R, R + 5, np.int32)                      # (entries beyond the count are never read)
    lst[:len(listed)] = rng.permutation(listed)
    flat = dict(ray_list=T(lst, torch.int32), ray_count=T([len(listed)], torch.int32))
    buf = torch.full((R, 3), -7., device=DEV)
    ops.composite_colors(ca, w, flat=flat, out=buf, **kw)
    on = torch.zeros(R, dtype=torch.bool, device=DEV)
    on[torch.tensor(listed.astype(np.int64), device=DEV)] = True
    assert torch.equal(buf[on], out[on]) and bool((buf[~on] == -7.).all())


# ----------------------------------------------------------------------------- end to end: the engine
def restate(out, mode, valid_only, S, Sf, two_net=False):
    """rgb_map / rgb0 [R,3] float64 from the keep=True internals: the logits K2 left, scattered by their lists, coloured by the
    torch functions, merged through the sorted order, weighted with T_i / weights_coarse, summed in float64"""
    R = out["rgb_map"].shape[0]

    def colours(tag, n, bits):
        confd, lst = out["confd_" + tag], out["list_" + tag]
        logits = torch.zeros(R * n, 24, device=DEV)
        has = torch.zeros(R * n, dtype=torch.bool, device=DEV)
        if lst is None:
            logits[:], has[:] = confd, True
        else:
            cnt = int(out["count_" + tag])
            at = lst[:cnt].long()
            logits[at], has[at] = confd[:cnt], True
        c = colour_ref(logits, mode, mask_of(bits) if valid_only else None)
        c[~has] = 0.                                   # no logits: outside every volume, weight exactly +0 (asserted by the caller)
        return c.reshape(R, n, 3)

    c0 = colours("coarse", S, out["valid_bits"])
    rgb0 = (out["weights_coarse"].double()[..., None] * c0).sum(1)
    if two_net:
        c = colours("fine", S + Sf, out["valid_bits_fine"])
    else:
        both = torch.cat([c0, colours("fine", Sf, out["valid_bits_fine"])], 1)
        c = torch.gather(both, 1, out["sorted_idxs"].long()[..., None].expand(-1, -1, 3))
    return (out["T_i"].double()[..., None] * c).sum(1), rgb0


def map_tol(mode):
    return E2E_SUM_TOL + (ENTROPY_TOL if mode == "entropy" else 0.)


def check_against_restatement(out, mode, valid_only, what, two_net=False):
    want, want0 = restate(out, mode, valid_only, S_E2E, SF_E2E, two_net)
    e, e0 = float((out["rgb_map"].double() - want).abs().max()), float((out["rgb0"].double() - want0).abs().max())
    print(f"part map {mode} valid_only={valid_only} {what}: rgb_map {e:.3e} rgb0 {e0:.3e} (bound {map_tol(mode):.3e})")
    assert e <= map_tol(mode) and e0 <= map_tol(mode), (what, e, e0)


def danbo_engine(seed=3):
    from core.render_engine import DanboEngine
    from core.utils import synthetic as syn
    cfg = syn.model_config("danbo_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd = syn.make_state_dict(cfg, seed=seed, n_framecodes=10, rest=rest)
    orc = o.DanboOracle(cfg, sd, rest)
    return DanboEngine(dict(cfg), {k: T(v) for k, v in sd.items()}, T(orc.align))


@pytest.fixture(scope="module")
def frame():
    from core.utils import synthetic as syn
    eng = danbo_engine()
    scene = syn.make_scene(n_poses=1, H=32, W=32, n_views=1, pose_seed=40)
    ro, rd = scene["rays"][0]
    assert len(ro) == 1024
    args = (T(ro), T(rd), T(scene["skts"]), T(scene["bones"]), T(scene["cyls"]), torch.zeros(1024, dtype=torch.int64, device=DEV))
    plain = clone(eng.render(*args, S_E2E, SF_E2E))
    keep = clone(eng.render(*args, S_E2E, SF_E2E, keep=True))
    return dict(eng=eng, scene=scene, rays=(ro, rd), args=args, plain=plain, keep=keep)


def test_frame_preconditions(frame):
    """what the end-to-end assertions rely on: enough opaque rays, several bones in the picture, no weight outside the volumes"""
    from core.networks.misc import joint_colours
    eng, plain, keep = frame["eng"], frame["plain"], frame["keep"]
    assert eng.empty_density_le0 and eng.flat_rays_ok
    solid = plain["acc_map"] > 0.5
    print("rays with acc > 0:", int((plain["acc_map"] > 0).sum()), " with acc > 0.5:", int(solid.sum()))
    assert int(solid.sum()) >= 50
    out = eng.render(*frame["args"], S_E2E, SF_E2E, part_map="confd")
    # the palette colour nearest to every opaque pixel's (un-premultiplied) colour
    pix = out["rgb_map"][solid] / plain["acc_map"][solid, None]
    near = torch.cdist(pix, joint_colours(DEV)).argmin(-1)
    print("distinct palette colours among the opaque pixels:", len(near.unique()))
    assert len(near.unique()) >= 5
    inside0 = keep["valid_bits"].reshape(1024, S_E2E) != 0
    inside = torch.gather(torch.cat([inside0, (eng.render(*frame["args"], S_E2E, SF_E2E, part_map="confd", keep=True)["valid_bits_fine"]
                                               .reshape(1024, SF_E2E) != 0)], 1), 1, keep["sorted_idxs"].long())
    assert float(keep["weights_coarse"][~inside0].abs().sum()) == 0. and float(keep["T_i"][~inside].abs().sum()) == 0.


@pytest.mark.parametrize("valid_only", [False, True])
@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_engine_part_map(frame, mode, valid_only):
    eng, args, plain = frame["eng"], frame["args"], frame["plain"]
    kw = dict(part_map=mode, part_valid_only=valid_only)
    lazy = clone(eng.render(*args, S_E2E, SF_E2E, **kw))
    kept = eng.render(*args, S_E2E, SF_E2E, keep=True, **kw)
    dense = eng.render(*args, S_E2E, SF_E2E, dense=True, **kw)
    for k in OTHERS:                                    # (i) nothing but the two colour maps moves
        assert torch.equal(lazy[k], plain[k]) and torch.equal(kept[k], plain[k]) and torch.equal(dense[k], plain[k]), k
    assert kept["list_coarse"] is not None and kept["confd_coarse"].shape[1] == 24
    assert torch.equal(kept["sorted_idxs"], frame["keep"]["sorted_idxs"])
    check_against_restatement(kept, mode, valid_only, "culled")          # (ii)
    for k in ("rgb_map", "rgb0"):                       # (iii) lazy, keep and dense: the same bits
        assert torch.equal(lazy[k], kept[k]) and torch.equal(lazy[k], dense[k]), k
    solid = plain["acc_map"] > 0.5                      # (iv) it is a different picture
    diff = (lazy["rgb_map"] - plain["rgb_map"]).abs().amax(-1)[solid]
    print(f"part map {mode} valid_only={valid_only}: |map - colour image| on the opaque rays: min {float(diff.min()):.3e} mean {float(diff.mean()):.3e}")
    assert float(diff.min()) > 1e-3
    assert bool(torch.isfinite(lazy["rgb_map"]).all()) and float(lazy["rgb_map"].min()) >= -1e-6


def test_valid_only_changes_the_map(frame):
    eng, args = frame["eng"], frame["args"]
    a = eng.render(*args, S_E2E, SF_E2E, part_map="confd")["rgb_map"]
    b = eng.render(*args, S_E2E, SF_E2E, part_map="confd", part_valid_only=True)["rgb_map"]
    assert float((a - b).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        eng.render(*args, S_E2E, SF_E2E, part_map="bones")


@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_engine_part_map_softplus_takes_the_dense_path(frame, mode):
    from core import hip_ops as ops
    eng, args = frame["eng"], frame["args"]
    eng.cfg["density_act"] = ("softplus", 1.0)
    try:
        plain = clone(eng.render(*args, S_E2E, SF_E2E))
        out = clone(eng.render(*args, S_E2E, SF_E2E, part_map=mode))
        kept = eng.render(*args, S_E2E, SF_E2E, part_map=mode, keep=True)
    finally:
        eng.cfg["density_act"] = ops.RELU
    assert kept["list_coarse"] is None and kept["list_fine"] is None and len(kept["confd_coarse"]) == 1024 * S_E2E
    assert float(plain["acc_map"].min()) > 0.            # softplus: density on every sample, also outside the volumes
    for k in OTHERS:
        assert torch.equal(out[k], plain[k]) and torch.equal(kept[k], plain[k]), k
    for k in ("rgb_map", "rgb0"):
        assert torch.equal(out[k], kept[k]), k
    check_against_restatement(kept, mode, False, "softplus, dense")
    again = eng.render(*args, S_E2E, SF_E2E)
    assert all(torch.equal(again[k], frame["plain"][k]) for k in MAPS)


@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_engine_part_map_with_and_without_rays_of_constants(frame, mode):
    from core import hip_ops as ops
    eng, args = frame["eng"], frame["args"]
    on = clone(eng.render(*args, S_E2E, SF_E2E, part_map=mode))
    eng.skip_flat_rays = False
    try:
        off = eng.render(*args, S_E2E, SF_E2E, part_map=mode)
    finally:
        eng.skip_flat_rays = True
    for k in MAPS:
        assert torch.equal(on[k], off[k]), k
    near, far = eng.near_far(args[0], args[1], args[4], args[2])
    flat = ops.ray_bone_mask(args[0], args[1], args[2], eng.align, eng.axis_scale, near, far, want_flat=True)[3] != 0
    assert int(flat.sum()) > 100
    for k in ("rgb_map", "rgb0"):
        z = on[k][flat]
        assert float(z.abs().sum()) == 0. and not bool(torch.signbit(z).any()), k


# ----------------------------------------------------------------------------- caster
def danbo_caster(two_net=False, seeds=(3, 4), n_codes=10):
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "danbo_base.txt"))
    args.single_net = not two_net
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=n_codes, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    _, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    assert caster.two_net == two_net
    cfg = syn.model_config("danbo_base")
    sds = [syn.make_state_dict(cfg, seed=s, n_framecodes=n_codes, rest=syn.rest_pose(0.48)) for s in seeds]
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sds[0].items()}, strict=True)
    if two_net:
        caster.network_fine.load_state_dict({k: torch.tensor(v) for k, v in sds[1].items()}, strict=True)
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    return caster, kw


def cast(caster, kw, scene, rb, **extra):
    z = np.zeros(len(rb), np.int64)
    return caster(T(rb), N_samples=S_E2E, kp_batch=T(scene["kps"][z]), skts=T(scene["skts"][z]), cyls=T(scene["cyls"][z]),
                  bones=T(scene["bones"][z]), cams=T(z, torch.int64), N_importance=SF_E2E, N_uniques=1, **dict(kw, **extra))


def test_caster_graph_key_whole_image_and_both_flags(frame):
    from core import trainer
    from core.utils import synthetic as syn
    caster, kw = danbo_caster()
    scene, (ro, rd) = frame["scene"], frame["rays"]
    rb = syn.ray_batch(ro, rd)
    assert len(rb) <= caster.graph_max_rays and caster.use_graphs
    plain = clone(cast(caster, kw, scene, rb))
    part = clone(cast(caster, kw, scene, rb, render_confd=True))          # same chunk shape: another graph
    assert len(caster._graphs.graphs) == 2
    assert not torch.equal(plain["rgb_map"], part["rgb_map"])
    for k in OTHERS:
        assert torch.equal(plain[k], part[k]), k
    replay = cast(caster, kw, scene, rb, render_confd=True)
    caster.use_graphs = False
    try:
        eager = clone(cast(caster, kw, scene, rb, render_confd=True))
        both = cast(caster, kw, scene, rb, render_confd=True, render_entropy=True)       # confd wins
        ent = clone(cast(caster, kw, scene, rb, render_entropy=True))
        masked = cast(caster, kw, scene, rb, render_confd=True, part_valid_only=True)
    finally:
        caster.use_graphs = True
    for k in MAPS:
        assert torch.equal(part[k], eager[k]) and torch.equal(replay[k], eager[k]) and torch.equal(both[k], eager[k]), k
    assert not torch.equal(ent["rgb_map"], eager["rgb_map"]) and not torch.equal(masked["rgb_map"], eager["rgb_map"])
    solid = plain["acc_map"] > 0.5
    assert int(solid.sum()) >= 50 and float((part["rgb_map"] - plain["rgb_map"]).abs().amax(-1)[solid].min()) > 1e-3
    # the whole image in one cast against the chunked loop
    n = len(ro)
    exp = lambda x, dt=torch.float32: T(x, dt)[:1].expand(n, *x.shape[1:])  # noqa: E731
    kwargs = dict(kp_batch=exp(scene["kps"]), skts=exp(scene["skts"]), cyls=exp(scene["cyls"]), bones=exp(scene["bones"]),
                  cams=torch.zeros(1, dtype=torch.int64, device=DEV).expand(n), ray_caster=caster, N_samples=S_E2E,
                  N_importance=SF_E2E, render_entropy=True, **kw)
    whole = trainer.render(32, 32, 80., chunk=256, rays=(T(ro), T(rd)), **kwargs)
    orig = caster.render_rays_whole
    caster.render_rays_whole = lambda *a, **k: None
    try:
        loop = trainer.render(32, 32, 80., chunk=256, rays=(T(ro), T(rd)), **kwargs)
    finally:
        caster.render_rays_whole = orig
    for k in loop:
        assert torch.equal(whole[k], loop[k]), k
    kwargs["render_entropy"] = False
    assert not torch.equal(trainer.render(32, 32, 80., chunk=256, rays=(T(ro), T(rd)), **kwargs)["rgb_map"], whole["rgb_map"])


def test_anerf_caster_ignores_the_flags(frame):
    """A-NeRF has no assignment net: the flags change nothing there"""
    from core.config import parse_args
    from core.raycasters import create_raycaster
    from core.utils import synthetic as syn
    from core.utils.skeleton_utils import SMPLSkeleton
    args = parse_args(["--no_reload"], config=os.path.join(ROOT, "danbo-pytorch_amd", "configs", "h36m_zju", "anerf_base.txt"))
    da = dict(skel_type=SMPLSkeleton, near=0., far=100., n_views=10, rest_pose=syn.rest_pose(0.48), hwf=(64, 64, 80.))
    _, te, *_ = create_raycaster(args, da, device=DEV)
    caster = te["ray_caster"].eval()
    kw = {k: v for k, v in te.items() if k not in ("ray_caster", "use_viewdirs", "N_samples", "N_importance")}
    scene, (ro, rd) = frame["scene"], frame["rays"]
    rb = syn.ray_batch(ro[:256], rd[:256])
    a = clone(cast(caster, kw, scene, rb))
    b = cast(caster, kw, scene, rb, render_confd=True, part_valid_only=True)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ----------------------------------------------------------------------------- two networks
@pytest.mark.parametrize("mode", ["confd", "entropy"])
def test_two_net_part_map(frame, mode):
    eng_c, eng_f, args = frame["eng"], danbo_engine(seed=4), frame["args"]
    plain = clone(eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E))
    for valid_only in (False, True):
        kw = dict(part_map=mode, part_valid_only=valid_only)
        lazy = clone(eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E, **kw))
        kept = eng_c.render_two_net(eng_f, *args, S_E2E, SF_E2E, keep=True, **kw)
        for k in OTHERS:
            assert torch.equal(lazy[k], plain[k]) and torch.equal(kept[k], plain[k]), k
        for k in ("rgb_map", "rgb0"):
            assert torch.equal(lazy[k], kept[k]), k
        inside = kept["valid_bits_fine"].reshape(1024, -1) != 0
        assert float(kept["T_i"][~inside].abs().sum()) == 0.
        assert len(kept["confd_fine"]) == 1024 * (S_E2E + SF_E2E)
        check_against_restatement(kept, mode, valid_only, "two networks", two_net=True)
        solid = plain["acc_map"] > 0.5
        assert int(solid.sum()) >= 50 and float((lazy["rgb_map"] - plain["rgb_map"]).abs().amax(-1)[solid].min()) > 1e-3


# ----------------------------------------------------------------------------- entry point
def test_run_render_writes_the_part_map(tmp_path):
    """train -> checkpoint -> run_render --render_confd on the synthetic source: image.npy holds the map.  A pixel whose ray's
    weighted samples all name one bone is acc x that bone's palette colour over the white background, up to the uint8 rounding."""
    import run_nerf
    import run_render
    from core.networks.misc import joint_colours
    from core.raycasters import RayCaster
    from core.render_engine import DanboEngine
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "1000", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "selected", "--selected_idxs", "0", "--render_res", "32", "32", "--white_bkgd"]
    rec, paths = [], []
    orig_render, orig_path = DanboEngine.render, run_render.render_path

    def spy(self, *a, **k):                      # keep=True gives the same bits (tests above) and shows what the kernels read
        out = orig_render(self, *a, **dict(k, keep=True))
        rec.append((k.get("part_map"), out))
        return {key: out[key] for key in MAPS}

    def path(**k):
        paths.append(orig_path(**k))
        return paths[-1]
    DanboEngine.render, run_render.render_path, RayCaster.use_graphs = spy, path, False      # (eager: the spy reads device counts)
    try:
        rgbs, accs, _, _ = run_render.run_render(base + ["--runname", "parts", "--render_confd"])
    finally:
        DanboEngine.render, run_render.render_path, RayCaster.use_graphs = orig_render, orig_path, True
    plain, _, _, _ = run_render.run_render(base + ["--runname", "plain"])
    img, acc8 = np.load(tmp_path / "out" / "parts" / "image.npy"), np.load(tmp_path / "out" / "parts" / "acc.npy")
    assert img.shape == (1, 32, 32, 3) and img.dtype == np.uint8
    print("run_render part map: acc max", float(accs.max()), " max |map image - colour image|", float(np.abs(rgbs - plain).max()))
    assert np.array_equal(img, (rgbs * 255).astype(np.uint8)) and not np.array_equal(img, np.load(tmp_path / "out" / "plain" / "image.npy"))
    rec = [r for r in rec if r[0] is not None]          # (the synthetic data source renders its teacher images through the engine too)
    assert len(rec) == 1 and rec[0][0] == "confd"
    out, valid_idx = rec[0][1], paths[0][3][0].to(DEV)
    R = out["rgb_map"].shape[0]
    S, N = out["weights_coarse"].shape[1], out["T_i"].shape[1]
    # the arg-max bone of every sample of the sorted order, from the logits the colouring read
    def bones(tag, n):
        b = torch.full((R * n,), -1, dtype=torch.long, device=DEV)
        cnt = int(out["count_" + tag])
        b[out["list_" + tag][:cnt].long()] = out["confd_" + tag][:cnt].argmax(-1)
        return b.reshape(R, n)
    bone = torch.gather(torch.cat([bones("coarse", S), bones("fine", N - S)], 1), 1, out["sorted_idxs"].long())
    w = out["T_i"] > 0
    assert bool((bone[w] >= 0).all())
    first = torch.where(w, bone, torch.full_like(bone, 99)).amin(-1)
    one = w.any(-1) & ((bone == first[:, None]) | ~w).all(-1)
    print("rays whose weighted samples all name one bone:", int(one.sum()), "of", int(w.any(-1).sum()), "with weight; acc == 255 pixels:",
          int((acc8 == 255).sum()))
    assert int(one.sum()) >= 1
    acc = out["acc_map"][one, None].double()
    want = acc * joint_colours(DEV)[first[one]].double()
    # sum w c against (sum w) c: the rounding of either fp32 sum of N terms, N 2^-24 each
    assert float((out["rgb_map"][one].double() - want).abs().max()) <= 2 * N * 2.0 ** -24 * 1.01
    pix = torch.tensor(img[0].reshape(-1, 3), device=DEV)[valid_idx][one].double()
    assert float((pix - (want + (1 - acc)) * 255).abs().max()) <= 1.0 + 1e-2          # (x * 255).astype(uint8) truncates
