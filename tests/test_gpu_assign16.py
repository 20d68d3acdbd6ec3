"""K2's fast kernel (csrc/k_assign16.hip: factorised gather + assignment GNN on fp16 hi/lo-split MFMAs + masked sigmoid + blend,
danbo_gather_assign_blend16_fwd) against the float64 arbiter (helpers.assignment_f64 / blend_f64 on the oracle's fp32 gather)
and against the exact-fp32 kernel (ops.assign_blend) on the same inputs, on synthetic scenes that reach the paths the stage
fixture does not: tails and the persistent tile loop, tiles that straddle poses (the L1/L2 route), crowded volumes, the
neighbour-pair skip, and checkpoints whose assignment net or features leave fp16's range.

Bounds are those of test_gpu_kernels.test_assign_blend_unfused_and_fused: h within 5e-6, logits within 2e-5, both relative to
max(1, the reference's largest |value|)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import danbo_oracle as o
from helpers import ROOT, assignment_f64, blend_f64, synthetic, T, N

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
J = 24
H_BOUND, LOGIT_BOUND = 5e-6, 2e-5
SENTINEL = 12345.0


def _ops():
    from core import hip_ops
    return hip_ops


def _prob_edit(sd, f0, f1):
    """layer 0 of the assignment net times f0, layer 1 times f1, w2 divided by f0 f1: the same function (ReLU commutes with a
    positive factor) at another scale -- in float64, rounded once to fp32"""
    a = "prob_linears.layers."
    sd = dict(sd)
    for k, f in (("0.lin.weight", f0), ("0.bias", f0), ("1.weight", f1), ("1.bias", f0 * f1), ("2.weight", 1.0 / (f0 * f1))):
        sd[a + k] = (sd[a + k].astype(np.float64) * f).astype(np.float32)
    return sd


def make_case(G=1, rays_per_pose=64, S=16, seed=0, axis_mult=1.0, vol_mult=1.0, prob=(1.0, 1.0)):
    """G poses x rays_per_pose rays x S samples (rows = R S), rays aimed at a random joint of their pose so that the samples
    straddle the bone volumes; engine, volumes, in-volume bits and the float64 reference of every row."""
    from core.render_engine import DanboEngine
    ops = _ops()
    syn = synthetic()
    cfg = syn.model_config("danbo_base")
    rest = syn.rest_pose(cfg["rest_scale"])
    sd = {k: np.array(v, dtype=np.float32) for k, v in syn.make_state_dict(cfg, seed=1, n_framecodes=8, rest=rest).items()}
    sd["graph_net.axis_scale"] = (sd["graph_net.axis_scale"] * np.float32(axis_mult)).astype(np.float32)
    if prob != (1.0, 1.0):
        sd = _prob_edit(sd, *prob)
    assert all(np.isfinite(v).all() for v in sd.values())
    bones = syn.random_bones(G, seed=seed).astype(np.float32)
    _, skts, kps = syn.forward_kinematics(bones, rest)
    skts = skts.astype(np.float32)
    align = o.bone_align_transforms(rest)
    rng = np.random.default_rng(seed + 100)
    R = G * rays_per_pose
    pose = np.arange(R) // rays_per_pose
    target = kps[pose, rng.integers(0, J, R)] + rng.normal(0.0, 0.05, (R, 3))
    d = rng.normal(size=(R, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays_o = (target - 2.0 * d).astype(np.float32)
    rays_d = d.astype(np.float32)
    z = np.sort(rng.uniform(1.6, 2.4, (R, S)), -1).astype(np.float32)
    eng = DanboEngine(cfg, {k: T(v) for k, v in sd.items()}, T(align))
    eng.refresh()
    vols = eng.volumes(T(bones))
    if vol_mult != 1.0:
        vols = (vols * vol_mult).contiguous()
    geo = ops.Geometry(T(rays_o), T(rays_d), T(skts), eng.align, eng.axis_scale, z=T(z))
    bits = ops.bone_cull(geo, compact=False)[0]
    # the reference, on the oracle's fp32 gather of the same inputs
    vols_np = N(vols)
    pts = o.sample_points(rays_o, rays_d, z)
    pts_t = o.bone_local(pts, skts[pose], align)
    x, _ = o.in_volume(pts_t, sd["graph_net.axis_scale"])
    pf = (o.factorised_gather(vols_np, x, pose, cfg["voxel_feat"], cfg["voxel_res"]) * o.window(x)[..., None]).astype(np.float32)
    pf = pf.reshape(-1, J, pf.shape[-1])
    valid = ((N(bits).astype(np.uint32)[:, None] >> np.arange(J, dtype=np.uint32)) & 1).astype(bool)
    logits = assignment_f64(sd, pf)
    _, h = blend_f64(pf, logits, valid)
    return dict(eng=eng, geo=geo, vols=vols, bits=bits, pf=pf, valid=valid, logits=logits, h=h, G=G, S=S, R=R,
                rays_per_pose=rays_per_pose, vols_np=vols_np, x=x, sd=sd)


def run16(c, lst=None, cnt=None, want_confd=True):
    """danbo_gather_assign_blend16_fwd into outputs pre-filled with a sentinel (rows the launch must not touch keep it); the
    tile-ticket word must be back at 0 when the launch has finished"""
    ops = _ops()
    geo, eng = c["geo"], c["eng"]
    n = geo.M
    h = torch.full((n, ops.H_STRIDE), SENTINEL, device=DEV)
    confd = torch.full((n, J), SENTINEL, device=DEV) if want_confd else None
    aw = eng.aw
    ops._call("danbo_gather_assign_blend16_fwd", *geo.head(), ops._p(c["vols"]), ops._p(c["bits"]), ops._p(lst), ops._p(cnt), n,
              ops._p(eng.assign16), ops._p(aw["b0"]), ops._p(aw["b1"]), ops._p(aw["w2"]), ops._p(aw["b2"]), ops._p(h),
              ops._p(confd), ops._p(ops._ticket(geo.device)), ops._stream())
    torch.cuda.synchronize()
    assert int(ops._ticket(geo.device).item()) == 0
    return N(h), (N(confd) if want_confd else None)


def _bound_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(1.0, float(np.abs(ref).max())))


def check(c, rows, h, confd, label="", h_on_own_logits=False):
    """rows: the input row of each output row; h / confd of the kernel against the arbiter and the exact-fp32 kernel.
    h_on_own_logits: h against the float64 blend of the kernel's OWN logits (the logits against float64 separately) -- for logits
    of ~400, whose fp32 round-off (relative, ~1e-7 of 400) the sigmoid's slope near 0 turns into ~1e-5 of h in ANY fp32
    evaluation (measured: the exact-fp32 kernel too)"""
    ops = _ops()
    assert np.isfinite(h).all() and (confd is None or np.isfinite(confd).all())
    h32, confd32 = ops.assign_blend(T(c["pf"]), c["bits"], c["eng"].aw, want_confd=True)
    h32, confd32 = N(h32)[rows], N(confd32)[rows]
    h_ref = blend_f64(c["pf"][rows], confd, c["valid"][rows])[1] if h_on_own_logits else c["h"][rows]
    eh, e32, e32_64 = _bound_err(h[:, :15], h_ref), _bound_err(h[:, :15], h32[:, :15]), _bound_err(h32[:, :15], c["h"][rows])
    print(f"{label}: h vs float64 {eh:.2e} (vs the fp32 kernel {e32:.2e}; fp32 kernel vs float64 {e32_64:.2e})", end="")
    if confd is not None:
        el, el32, el32_64 = _bound_err(confd, c["logits"][rows]), _bound_err(confd, confd32), _bound_err(confd32, c["logits"][rows])
        print(f", logits vs float64 {el:.2e} (vs the fp32 kernel {el32:.2e}; fp32 kernel vs float64 {el32_64:.2e}; |logit| <= "
              f"{np.abs(c['logits']).max():.3g})", end="")
    print()
    assert eh <= H_BOUND, (label, "h", eh)
    assert float(np.abs(h[:, 15]).max()) == 0.0
    if not h_on_own_logits:
        assert e32 <= H_BOUND, (label, "h vs fp32 kernel", e32)
        assert e32_64 <= H_BOUND
    if confd is not None:
        assert el <= LOGIT_BOUND, (label, "logits", el)
        assert el32 <= LOGIT_BOUND, (label, "logits vs fp32 kernel", el32)
        assert el32_64 <= LOGIT_BOUND


def run_and_check(c, seed=0, frac=0.85):
    """dense, then a compacted and permuted list (frac of the rows, count on the device); confd on and off: h bitwise the same"""
    M = c["geo"].M
    h, confd = run16(c)
    check(c, np.arange(M), h, confd, "dense")
    h2, _ = run16(c, want_confd=False)
    assert np.array_equal(h2, h)
    rng = np.random.default_rng(seed)
    k = max(1, int(round(frac * M)))
    rows = rng.permutation(M)[:k].astype(np.int32)
    lst = T(np.concatenate([rows, np.zeros(M - k, np.int32)]), torch.int32)      # (entries past the count are never read)
    cnt = T(np.array([k]), torch.int32)
    hl, confdl = run16(c, lst, cnt)
    check(c, rows, hl[:k], confdl[:k], "list")
    assert (hl[k:] == SENTINEL).all() and (confdl[k:] == SENTINEL).all()
    hl2, _ = run16(c, lst, cnt, want_confd=False)
    assert np.array_equal(hl2, hl)
    return rows


@pytest.mark.parametrize("n", [1, 31, 33, 127, 129, 4133, 81920])
def test_k2_row_counts_tails_and_the_persistent_tile_loop(n):
    """tails around the 32-row wavefront and 128-row tile, and a launch of more than 2 x 256 tiles (> 65 536 rows): the tiles
    beyond the first workgroup's are handed out by the ticket counter"""
    S = 32 if n > 65536 else 1
    c = make_case(G=1, rays_per_pose=n // S, S=S, seed=n)
    assert c["geo"].M == n
    rows = run_and_check(c, seed=n)
    if n > 65536:
        assert len(rows) > 2 * 256 * 128               # the list launch also runs the persistent loop
    if n >= 31:
        assert c["valid"].any(-1).sum() >= n // 4


@pytest.mark.parametrize("G,rays_per_pose", [(48, 4), (2, 97)])
def test_k2_tiles_that_straddle_poses(G, rays_per_pose):
    """rows of a tile whose pose is not the tile's first row's read transforms and volumes through L1/L2, not the staged LDS copy"""
    c = make_case(G=G, rays_per_pose=rays_per_pose, S=16, seed=3)
    spp = rays_per_pose * 16
    M = c["geo"].M
    rows = run_and_check(c, seed=G)
    for order in (np.arange(M), rows):
        pose = order // spp
        ntile = (len(order) + 127) // 128
        first = pose[np.arange(ntile) * 128]
        other = pose != np.repeat(first, 128)[: len(order)]
        assert (other & c["valid"][order].any(-1)).sum() > 0              # in-volume rows on the L2 route
    if G == 48:
        assert all(len(np.unique(np.arange(M)[t * 128:(t + 1) * 128] // spp)) == 2 for t in range(M // 128))


@pytest.mark.parametrize("mult", [4.0, 12.0])
def test_k2_crowded_volumes(mult):
    """bone volumes grown 4x / 12x (axis_scale is trainable): rows valid in many bones walk the longest bone loop"""
    c = make_case(G=2, rays_per_pose=64, S=16, seed=5, axis_mult=mult)
    assert (c["valid"].sum(-1) >= 8).sum() > 0
    run_and_check(c, seed=int(mult))


# ---------------------------------------------------------------------------------------------------------------------------
# the neighbour-pair skip: exact, bit for bit (a fresh process with DANBO_A16_NOSKIP=1 evaluates every pair)
SKIP_CASE = dict(G=2, rays_per_pose=128, S=16, seed=7)


def _skip_share(c, want_confd):
    """(skipped, evaluated) neighbour pairs t >= 1 of the wavefronts of the dense launch, as the kernel decides them: a pair is
    skipped where window x largest |volume entry| < 2^-26 for both of its bones on every row that uses the bone's logit"""
    G, spp = c["G"], c["rays_per_pose"] * c["S"]
    x = c["x"].reshape(-1, J, 3)
    win = o.window(x.reshape(-1, 3)).reshape(-1, J).astype(np.float32)
    vmax = np.abs(c["vols_np"]).max(-1)                                            # [G, 24]
    pose = np.arange(x.shape[0]) // spp
    small = (win * vmax[pose]).astype(np.float32) < np.float32(2.0 ** -26)          # [M, 24]
    nb = {j: [j] + [i for i in range(J) if i != j and (o.adjacency()[j, i] != 0)] for j in range(J)}
    skipped = evaluated = 0
    M = x.shape[0]
    for w0 in range(0, M, 32):
        sl = slice(w0, min(w0 + 32, M))
        v = c["valid"][sl]
        todo = range(J) if want_confd else [j for j in range(J) if v[:, j].any()]
        for j in todo:
            used = np.ones(v.shape[0], bool) if want_confd else v[:, j]
            q = nb[j]
            for t in range(1, (len(q) + 1) // 2):
                pair = q[2 * t: 2 * t + 2]
                if all(small[sl][used][:, b].all() for b in pair):
                    skipped += 1
                else:
                    evaluated += 1
    return skipped, evaluated


def _child_main(out_dir):
    """(run in a fresh process) the skip case's launches, outputs as .npy"""
    c = make_case(**SKIP_CASE)
    h, confd = run16(c)
    h2, _ = run16(c, want_confd=False)
    np.save(os.path.join(out_dir, "h.npy"), h)
    np.save(os.path.join(out_dir, "confd.npy"), confd)
    np.save(os.path.join(out_dir, "h_noconfd.npy"), h2)


def test_k2_neighbour_pair_skip_is_exact(tmp_path):
    c = make_case(**SKIP_CASE)
    for want_confd in (True, False):
        skipped, evaluated = _skip_share(c, want_confd)
        print(f"confd={want_confd}: neighbour pairs skipped {skipped}, evaluated {evaluated}")
        assert skipped >= 0.1 * (skipped + evaluated) and evaluated >= 0.1 * (skipped + evaluated)
    h, confd = run16(c)
    check(c, np.arange(c["geo"].M), h, confd, "skip case")
    h2, _ = run16(c, want_confd=False)
    env = dict(os.environ, DANBO_A16_NOSKIP="1")
    code = ("import sys; sys.path[:0] = %r; import test_gpu_assign16 as t; t._child_main(%r)"
            % ([os.path.join(ROOT, "tests"), os.path.join(ROOT, "danbo-pytorch_amd"), os.path.join(ROOT, "oracle")], str(tmp_path)))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.array_equal(np.load(tmp_path / "h.npy"), h)
    assert np.array_equal(np.load(tmp_path / "confd.npy"), confd)
    assert np.array_equal(np.load(tmp_path / "h_noconfd.npy"), h2)


# ---------------------------------------------------------------------------------------------------------------------------
RANGE_CASES = {
    "layers_x1e-3": dict(prob=(1e-3, 1e-3)),
    "layers_x1e3": dict(prob=(1e3, 1e3)),
    "alternating": dict(prob=(1e3, 1e-3)),
    "layer0_x6e4": dict(prob=(6e4, 1.0 / 6e4)),
    "layer0_x2e5": dict(prob=(2e5, 1.0 / 2e5)),
    "volumes_x1e3": dict(vol_mult=1e3),
}


@pytest.mark.parametrize("case", list(RANGE_CASES))
def test_k2_on_checkpoints_outside_fp16_range(case):
    """The split puts every operand into two fp16 halves (normal from 6e-5, finite to 65504).  A checkpoint's assignment net is not
    bound to the seeded generator's scale: 1000x smaller / larger layers, alternating, a layer-0 output of ~1e5 (weights and
    bias x 6e4 or 2e5, the next layer scaled back) -- the same function at another scale, which K2 has to evaluate within the
    bounds (csrc/k_assign16.hip: k_assign16_pack's range factors; before them the kernel measured 1.6e-5, 1.1e-5, 4.5e-4 and
    0.14 of h on the x1e-3, alternating, x6e4 and x2e5 cases).  volumes x 1e3 makes the features and logits large (|logit| ~
    400): the bounds are relative there, and h is held to the float64 blend of the kernel's own logits (see check())."""
    c = make_case(G=2, rays_per_pose=64, S=16, seed=11, **RANGE_CASES[case])
    assert c["valid"].any(-1).sum() > 200
    assert np.abs(c["logits"][c["valid"]]).max() > 0.1
    if case == "volumes_x1e3":
        assert np.abs(c["logits"]).max() > 100.0
    h, confd = run16(c)
    check(c, np.arange(c["geo"].M), h, confd, case, h_on_own_logits=case == "volumes_x1e3")
    h2, _ = run16(c, want_confd=False)
    assert np.array_equal(h2, h)
