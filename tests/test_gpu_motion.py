"""The motion set-up on the GPU (danbo_pose_rotations / danbo_pose_chain / danbo_box_rays, core.motion, run_render --render_type
retarget / animate): the rotations against float64 Rodrigues within the bound derived in tests/motion_ref.py, everything after them
against the serial restatement of csrc/motion_math.hpp bit for bit -- every size, pose case, NULL output, a NaN joint, a second
call, odd addresses --, guard words around every output, frame_rays against kp_to_valid_rays, and the entry point."""
import os

import numpy as np
import pytest
import torch

import motion_ref as mr
from helpers import DEV, ROOT, entry
from motion_ref import E, F32, F64, J

pytestmark = pytest.mark.gpu
N_GUARD = 64          # guard words on either side of an output: 256 bytes, so an unshifted output keeps the allocation's alignment
FILL = -7.25
OUTPUTS = dict(l2ws=16 * J, skts=16 * J, kps=3 * J, cyls=5)      # floats per pose


def raw(name):
    import core.motion as cm
    cm.lib()
    return entry(name)


def stream_ptr():
    from core import _hip
    return _hip.stream()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def guarded(n, dtype=torch.float32, fill=FILL, shift=0):
    """-> (whole device buffer, the view of n payload elements that starts N_GUARD + shift elements in)"""
    buf = torch.full((n + 2 * N_GUARD + shift,), fill, dtype=dtype, device=DEV)
    return buf, buf[N_GUARD + shift:N_GUARD + shift + n]


def intact(buf, n, fill=FILL, shift=0):
    return bool((buf[:N_GUARD + shift] == fill).all()) and bool((buf[N_GUARD + shift + n:] == fill).all())


def gpu_rotations(bones):
    """the raw C call with guard words around rots -> [N,24,3,3] (numpy)"""
    N = len(bones)
    b = dev(bones)
    buf, rots = guarded(N * J * 9)
    rc = raw("danbo_pose_rotations")(b.data_ptr(), N, rots.data_ptr(), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(buf, N * J * 9), "a guard word was overwritten"
    return rots.reshape(N, J, 3, 3).cpu().numpy()


def gpu_chain(rots, rest, roots=None, want=tuple(OUTPUTS), shift=0, ext=None):
    """the raw C call with guard words around every wanted output (the others NULL) -> dict of numpy arrays"""
    N = len(rots)
    r, p, t = dev(rots), dev(rest), None if roots is None else dev(roots)
    bufs = {k: guarded(N * OUTPUTS[k], shift=shift) for k in want}
    ptrs = [bufs[k][1].data_ptr() if k in want else None for k in OUTPUTS]
    e = mr.extensions() if ext is None else ext
    rc = raw("danbo_pose_chain")(r.data_ptr(), p.data_ptr(), None if t is None else t.data_ptr(), N, *ptrs, *(float(x) for x in e),
                                 stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    shapes = dict(l2ws=(N, J, 4, 4), skts=(N, J, 4, 4), kps=(N, J, 3), cyls=(N, 5))
    out = {}
    for k in want:
        assert intact(bufs[k][0], N * OUTPUTS[k], shift=shift), f"a guard word of {k} was overwritten"
        out[k] = bufs[k][1].reshape(shapes[k]).cpu().numpy()
    return out


def gpu_box_rays(c2w, fx, fy, cx, cy, W, x0, y0, x1, y1):
    n = (x1 - x0) * (y1 - y0)
    c = dev(c2w)
    (bo, o), (bd, d), (bi, idx) = guarded(3 * n), guarded(3 * n), guarded(n, torch.int64, -5)
    # (the payload's address from the buffer's: the data_ptr() of a view without elements is null, and a null pointer is refused)
    at = lambda buf: buf.data_ptr() + N_GUARD * buf.element_size()      # noqa: E731
    rc = raw("danbo_box_rays")(c.data_ptr(), fx, fy, cx, cy, W, x0, y0, x1, y1, at(bo), at(bd), at(bi), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(bo, 3 * n) and intact(bd, 3 * n) and intact(bi, n, -5), "a guard word was overwritten"
    return o.reshape(n, 3).cpu().numpy(), d.reshape(n, 3).cpu().numpy(), idx.cpu().numpy()


def check_rotations(bones, rots):
    """rots against float64 Rodrigues and R^T R - I, both within the bounds of motion_ref's docstring; prints the share used"""
    want, bound = mr.rodrigues64(bones), mr.rodrigues_bound(bones)
    err = np.abs(rots.astype(F64) - want)
    r64 = rots.astype(F64)
    orth = np.abs(r64.swapaxes(-1, -2) @ r64 - np.eye(3))
    print(f"rotations: error {np.max(err / bound):.4f}, orthogonality {np.max(orth / (4 * bound)):.4f} of their bounds")
    assert np.all(err <= bound) and np.all(orth <= 4 * bound)


def check_chain(rots, rest, roots, got, ext=None):
    want = mr.host_chain(rots, rest, roots, ext=ext, want=tuple(got))
    for k in got:
        assert mr.same_bits(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


# ----------------------------------------------------------------------------- rotations and chain
@pytest.mark.parametrize("N", mr.SIZES)
def test_random_poses_at_every_size(N):
    """sizes that put an odd pose into a wavefront's second half (1, 3, 65) and cross a workgroup (65, 130: 8 poses each)"""
    bones, rest = mr.random_bones(N, seed=N), mr.rest_pose()
    rots = gpu_rotations(bones)
    check_rotations(bones, rots)
    for roots in (None, mr.random_roots(N, seed=N)):
        check_chain(rots, rest, roots, gpu_chain(rots, rest, roots))


@pytest.mark.parametrize("theta", mr.THETAS, ids=[f"{t:g}" for t in mr.THETAS])
def test_one_joint_at_an_angle(theta):
    bones, rest, roots = mr.one_joint_bones(3, theta), mr.rest_pose(), mr.random_roots(3)
    rots = gpu_rotations(bones)
    check_rotations(bones, rots)
    eye = np.eye(3, dtype=F32)
    assert np.all(np.delete(rots, 4, axis=1) == eye)                    # every joint at zero: the identity, exactly
    if theta == 0:
        assert np.all(rots == eye)
    if theta == 1e-7:
        assert np.all(rots[:, 4][:, [0, 1, 2], [0, 1, 2]] == 1) and np.all(rots[:, 4, 0, 1] != 0)      # I + K to first order
    for r in (None, roots):
        check_chain(rots, rest, r, gpu_chain(rots, rest, r))


def test_identity_pose():
    N, rest, roots = 3, mr.rest_pose(), mr.random_roots(3)
    rots = gpu_rotations(np.zeros((N, J, 3), F32))
    assert mr.same_bits(rots, np.tile(np.eye(3, dtype=F32), (N, J, 1, 1)))
    got = gpu_chain(rots, rest, None)
    check_chain(rots, rest, None, got)
    assert mr.same_bits(got["l2ws"][..., :3, :3], rots)
    _, trans, _, _ = mr.chain_bounds(rest, None, N)
    assert np.all(np.abs(got["kps"].astype(F64) - rest.astype(F64)) <= trans[..., None])       # the rest pose, up to the sums' rounding
    check_chain(rots, rest, roots, gpu_chain(rots, rest, roots))


def test_each_output_null_in_turn():
    N = 65
    rots, rest, roots = mr.rodrigues64(mr.random_bones(N, seed=2)).astype(F32), mr.rest_pose(), mr.random_roots(N)
    full = gpu_chain(rots, rest, roots)
    for left_out in OUTPUTS:
        want = tuple(k for k in OUTPUTS if k != left_out)
        got = gpu_chain(rots, rest, roots, want=want)
        assert all(mr.same_bits(got[k], full[k]) for k in want), left_out
    for only in OUTPUTS:
        assert mr.same_bits(gpu_chain(rots, rest, roots, want=(only,))[only], full[only]), only
    check_chain(rots, rest, roots, full)


def test_a_nan_joint_stays_in_its_subtree_and_its_pose():
    N, rest, roots = 3, mr.rest_pose(), mr.random_roots(3)
    clean = mr.random_bones(N, seed=8)
    bones = clean.copy()
    bones[1, 4, 1] = np.nan                 # joint 4 of pose 1: its descendants are 7 and 10
    bones[2, 13, 0] = np.inf                # joint 13 of pose 2: 16, 18, 20, 22
    rots, rots_clean = gpu_rotations(bones), gpu_rotations(clean)
    bad = np.isnan(rots).any((-1, -2))
    assert np.array_equal(np.argwhere(bad), [[1, 4], [2, 13]]) and np.isnan(rots[1, 4]).all() and np.isnan(rots[2, 13]).all()
    assert mr.same_bits(rots[~bad], rots_clean[~bad])
    got, ok = gpu_chain(rots, rest, roots), gpu_chain(rots_clean, rest, roots)
    want = mr.host_chain(rots, rest, roots)
    tainted = np.zeros((N, J), bool)
    tainted[1, [4, 7, 10]] = tainted[2, [13, 16, 18, 20, 22]] = True
    below = tainted.copy()                  # a joint's own position comes from its parent's matrix: only the joints below are lost
    below[1, 4] = below[2, 13] = False
    for k, lost in (("l2ws", tainted), ("skts", tainted), ("kps", below)):
        assert mr.same_bits_or_nan(got[k], want[k]), k
        flat = got[k].reshape(N, J, -1)
        assert np.array_equal(np.isnan(flat).any(-1), lost), k
        assert mr.same_bits(got[k][~lost], ok[k][~lost]), k
    assert mr.same_bits_or_nan(got["cyls"], want["cyls"]) and mr.same_bits(got["cyls"][0], ok["cyls"][0])
    assert np.isnan(got["cyls"][1:, 2:]).all() and not np.isnan(got["cyls"][:, :2]).any()


def test_a_second_call_and_odd_addresses():
    N = 65
    rots, rest, roots = mr.rodrigues64(mr.random_bones(N, seed=4)).astype(F32), mr.rest_pose(), mr.random_roots(N)
    first, second = gpu_chain(rots, rest, roots), gpu_chain(rots, rest, roots)          # one repeat, not a stress loop
    check_chain(rots, rest, roots, first)
    assert all(mr.same_bits(first[k], second[k]) for k in OUTPUTS)
    bones = mr.random_bones(N, seed=4)
    assert mr.same_bits(gpu_rotations(bones), gpu_rotations(bones))
    # outputs that start 1 .. 3 floats past an aligned address: the 16-byte stores must not be taken
    for shift in (1, 2, 3):
        got = gpu_chain(rots, rest, roots, shift=shift)
        assert all(mr.same_bits(got[k], first[k]) for k in OUTPUTS), shift
    # and inputs at such addresses
    room = torch.zeros(rots.size + 8, device=DEV)
    src = room[3:3 + rots.size]
    src.copy_(dev(rots).reshape(-1))
    out = torch.empty(N, J, 3, device=DEV)
    rc = raw("danbo_pose_chain")(src.data_ptr(), dev(rest).data_ptr(), None, N, None, None, out.data_ptr(), None, 0., 0., 0., stream_ptr())
    assert rc == 0
    assert mr.same_bits(out.cpu().numpy(), mr.host_chain(rots, rest, None, want=("kps",))["kps"])


# ----------------------------------------------------------------------------- box rays
@pytest.mark.parametrize("name", sorted(mr.BOXES))
def test_box_rays_equal_the_restatement_bitwise(name):
    c2w = mr.camera(seed=len(name))
    o, d, idx = gpu_box_rays(c2w, *mr.box_scalars(name))
    wo, wd, widx = mr.host_box_rays(c2w, *mr.box_scalars(name))
    assert mr.same_bits(o, wo) and mr.same_bits(d, wd) and mr.same_bits(idx, widx)
    if name.startswith("empty"):            # nothing was launched: the guards were checked with no payload between them
        assert len(idx) == 0
        return
    H, W, focal, center, tl, br = mr.BOXES[name]
    assert idx[0] == tl[1] * W + tl[0] and idx[-1] == (br[1] - 1) * W + br[0] - 1 and len(idx) == (br[0] - tl[0]) * (br[1] - tl[1])
    # the Python entry on the same case
    import core.motion as cm
    po, pd, pidx = cm.box_rays(dev(c2w), focal, center, H, W, tl, br)
    assert pidx.dtype == torch.int64 and pidx.is_cuda and mr.same_bits(po.cpu().numpy(), wo) and mr.same_bits(pd.cpu().numpy(), wd)
    assert mr.same_bits(pidx.cpu().numpy(), widx)


def test_an_empty_box_leaves_its_outputs_untouched():
    c = dev(mr.camera())
    o, d = torch.full((12,), FILL, device=DEV), torch.full((12,), FILL, device=DEV)
    idx = torch.full((4,), -5, dtype=torch.int64, device=DEV)
    for box in ((3, 2, 3, 5), (3, 2, 6, 2), (0, 0, 0, 0)):
        assert raw("danbo_box_rays")(c.data_ptr(), 10., 10., 4., 4., 8, *box, o.data_ptr(), d.data_ptr(), idx.data_ptr(), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((o == FILL).all()) and bool((d == FILL).all()) and bool((idx == -5).all())
    import core.motion as cm
    po, pd, pidx = cm.box_rays(c, 10., None, 8, 8, (3, 2), (3, 5))
    assert po.shape == (0, 3) and pd.shape == (0, 3) and pidx.shape == (0,)


# ----------------------------------------------------------------------------- the Python entries
def test_python_entries_and_frame_rays_against_kp_to_valid_rays():
    import core.motion as cm
    from core.load_data import synthetic_arrays
    from core.utils.ray_utils import kp_to_valid_rays
    H, W = 48, 40
    a = synthetic_arrays(n_poses=3, n_cams=2, H=H, W=W, pose_seed=2)          # three poses, two cameras each: six frames
    rest, bones, roots = a["rest_pose"].astype(F32), a["bones"].astype(F32), a["kp3d"][:, 0].astype(F32)
    chain = cm.pose_chain(bones=dev(bones), rest_pose=dev(rest), roots=dev(roots), ext_scale=mr.EXT_SCALE)
    rots = cm.rotations(dev(bones))
    assert rots.is_cuda and rots.shape == (6, J, 3, 3)
    want = mr.host_chain(rots.cpu().numpy(), rest, roots)
    assert all(mr.same_bits(chain[k].cpu().numpy(), want[k]) for k in OUTPUTS)
    by_rots = cm.pose_chain(rots=rots, rest_pose=dev(rest), roots=dev(roots)[:, None], cylinders=False)
    assert by_rots["cyls"] is None and all(torch.equal(by_rots[k], chain[k]) for k in ("l2ws", "skts", "kps"))
    with pytest.raises(ValueError, match="2\\^20 poses"):
        cm.rotations(dev(bones)[0])
    with pytest.raises(ValueError, match="one position per pose"):
        cm.pose_chain(rots=rots, rest_pose=dev(rest), roots=dev(roots)[:2])
    with pytest.raises(ValueError, match="does not lie in"):
        cm.box_rays(dev(a["c2ws"][0].astype(F32)), 10., None, H, W, (0, 0), (W + 1, 4))

    poses = a["c2ws"].astype(F32)
    two = np.stack([a["focals"], a["focals"] * F32(1.03125)], -1).astype(F32)
    centers = (np.array([W * 0.5, H * 0.5], F32) + np.random.default_rng(0).uniform(-3, 3, (6, 2))).astype(F32)
    for focal, cen in ((a["focals"].astype(F32), None), (two, centers)):
        rays, idxs, cyls, boxes = cm.frame_rays(poses, H, W, focal, chain["kps"], chain["cyls"], centers=cen)
        h_rays, h_idxs, h_cyls, h_boxes = kp_to_valid_rays(dev(poses), H, W, focal, kps=chain["kps"], centers=cen, ext_scale=mr.EXT_SCALE)
        assert mr.same_bits(cyls.cpu().numpy(), h_cyls.cpu().numpy())                  # the device's cylinders are numpy's
        assert len(rays) == len(h_rays) == 6 and cyls is chain["cyls"]
        bitwise = True
        for i in range(6):
            assert np.array_equal(boxes[i][0], h_boxes[i][0]) and np.array_equal(boxes[i][1], h_boxes[i][1])
            assert idxs[i].is_cuda and rays[i][0].is_cuda and np.array_equal(idxs[i].cpu().numpy(), h_idxs[i].numpy())
            n = len(h_idxs[i])
            assert n > 0 and rays[i][0].shape == rays[i][1].shape == (n, 3)
            o, d, ho, hd = (t.cpu().numpy() for t in (*rays[i], *h_rays[i]))
            assert mr.same_bits(o, ho)
            fx, fy = (float(focal[i]),) * 2 if focal.ndim == 1 else (float(f) for f in focal[i])
            cx, cy = (W * 0.5, H * 0.5) if cen is None else (float(c) for c in cen[i])
            x, y = (h_idxs[i].numpy() % W).astype(F64), (h_idxs[i].numpy() // W).astype(F64)
            dirs = np.abs(np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(n)], -1))
            bound = 4 * E * (dirs[:, None, :] * np.abs(poses[i, :3, :3].astype(F64))[None]).sum(-1) * (1 + 4 * E)
            assert np.all(np.abs(d.astype(F64) - hd) <= bound), i
            bitwise &= mr.same_bits(d, hd)
        print("frame_rays: directions bitwise equal to kp_to_valid_rays':", bitwise)
    # a device tensor of cameras gives the same as the host array
    again = cm.frame_rays(dev(poses), H, W, two, chain["kps"], chain["cyls"], centers=centers)
    assert all(torch.equal(x[1], y[1]) for x, y in zip(again[0], rays)) and all(torch.equal(x, y) for x, y in zip(again[1], idxs))


# ----------------------------------------------------------------------------- the entry point
def test_run_render_retarget_and_animate(tmp_path):
    import run_nerf
    import run_render
    from core.config import config_parser as nerf_config_parser, txt_to_argstring
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "20", "--render_factor", "0", "--n_iters", "20"])
    log, out = tmp_path / "demo", tmp_path / "out"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(out), "--render_res", "32", "32", "--selected_idxs", "1", "2"]
    args = run_render.config_parser().parse_args(base + ["--runname", "x"])
    nerf_args, _ = nerf_config_parser().parse_known_args(txt_to_argstring(args.nerf_args))
    dataset = run_render.get_render_dataset(args, nerf_args, DEV)
    np.savez(tmp_path / "own.npz", bones=dataset.bones[[1, 2]], kp3d=dataset.kp3d[[1, 2]])
    retarget = ["--render_type", "retarget", "--retarget_len", "1"]
    run_render.run_render(base + ["--runname", "selected", "--render_type", "selected"])
    run_render.run_render(base + ["--runname", "host"] + retarget + ["--motion_chain", "host"])
    run_render.run_render(base + ["--runname", "device", "--render_skel"] + retarget + ["--motion_chain", "device"])
    run_render.run_render(base + ["--runname", "motion", "--render_type", "retarget", "--motion", str(tmp_path / "own.npz"), "--motion_cam", "1"])
    run_render.run_render(base + ["--runname", "animate", "--render_type", "animate", "--n_step", "3", "--animate_joints", "16", "18"])
    load = lambda run, name: np.load(out / run / name, allow_pickle=True)      # noqa: E731
    image, acc, boxes = (load("selected", n) for n in ("image.npy", "acc.npy", "bboxes.npy"))
    assert image.shape == (2, 32, 32, 3) and boxes.shape == (2, 2, 2)
    # the host statement of the new type is the selected run, bit for bit
    assert mr.same_bits(load("host", "image.npy"), image) and mr.same_bits(load("host", "acc.npy"), acc)
    assert np.array_equal(load("host", "bboxes.npy"), boxes)

    def check(run, want_boxes, host_image, host_acc):
        img, a, bx = (load(run, n) for n in ("image.npy", "acc.npy", "bboxes.npy"))
        assert np.array_equal(bx, want_boxes), run
        inside = np.zeros(img.shape[:3], bool)
        for i, (tl, br) in enumerate(bx):
            inside[i, tl[1]:br[1], tl[0]:br[0]] = True
        assert inside.any() and np.all(img[~inside] == 0) and np.all(a[~inside] == 0), run       # (no --white_bkgd: black, acc 0)
        assert np.isfinite(img.astype(F64)).all() and img.dtype == np.uint8 and a.dtype == np.uint8
        print(f"run_render {run}: largest difference to the host chain's frames: image "
              f"{np.abs(img.astype(int) - host_image.astype(int)).max()} / 255, acc {np.abs(a.astype(int) - host_acc.astype(int)).max()} / 255")
        return img

    check("device", boxes, image, acc)
    assert load("device", "skel.npy").shape == image.shape and not (out / "host" / "skel.npy").exists()
    # the motion file holds the data's own bones, seen from frame 1's camera at frame 1's root: its first frame is the retarget
    # run's first frame, its second the other pose in that place
    m_boxes = load("motion", "bboxes.npy")
    assert m_boxes.shape == (2, 2, 2) and np.array_equal(m_boxes[0], boxes[0])
    check("motion", m_boxes, image[[0, 0]], acc[[0, 0]])
    assert load("animate", "image.npy").shape == (3 + 1, 32, 32, 3) and np.isfinite(load("animate", "acc.npy").astype(F64)).all()
