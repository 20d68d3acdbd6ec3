"""The motion set-up without a GPU: the serial restatement of csrc/motion_math.hpp (the code the kernels inline, built by g++)
against the numpy float32 restatement of tests/motion_ref.py bit for bit, against the project's own host path in float64 and
against get_kp_bounding_cylinder / get_rays, the sequence builders of core/motion.py, the argument rules of the three entries, and
the binding of include/danbo_motion.h as a satellite.  The bounds are derived in motion_ref's docstring."""
import ctypes

import numpy as np
import pytest

import motion_ref as mr
from helpers import ADDR, EINVAL, entry
from motion_ref import E, F32, F64, J

ENTRIES = ("danbo_pose_rotations", "danbo_pose_chain", "danbo_box_rays")


def rots32(bones):
    return mr.rodrigues64(bones).astype(F32)


# ----------------------------------------------------------------------------- the chain
def test_the_tree_tables_are_the_python_tree():
    from core.utils.skeleton_utils import SMPLSkeleton
    lib = mr.host_lib()
    assert [lib.ref_parent(j) for j in range(J)] == list(SMPLSkeleton.joint_trees) == list(mr.PARENT)
    assert [lib.ref_depth(j) for j in range(J)] == list(mr.DEPTH) and lib.ref_levels() == mr.DEPTH.max() + 1 == 9
    assert list(np.flatnonzero(mr.DEPTH == 8)) == [22, 23]


@pytest.mark.parametrize("with_roots", [False, True], ids=["no-roots", "roots"])
@pytest.mark.parametrize("N", mr.SIZES)
def test_restatement_equals_numpy_float32_bitwise(N, with_roots):
    rots, rest = rots32(mr.random_bones(N, seed=N)), mr.rest_pose()
    roots = mr.random_roots(N, seed=N) if with_roots else None
    got, want = mr.host_chain(rots, rest, roots), mr.chain32(rots, rest, roots)
    for k in ("l2ws", "skts", "kps", "cyls"):
        assert mr.same_bits(got[k], want[k]), k
    assert np.all(got["l2ws"][..., 3, :] == [0, 0, 0, 1]) and np.all(got["skts"][..., 3, :] == [0, 0, 0, 1])
    assert mr.same_bits(got["kps"], np.ascontiguousarray(got["l2ws"][..., :3, 3]))


def test_every_output_may_be_left_out():
    rots, rest, roots = rots32(mr.random_bones(3, seed=9)), mr.rest_pose(), mr.random_roots(3)
    full = mr.host_chain(rots, rest, roots)
    for k in full:
        one = mr.host_chain(rots, rest, roots, want=(k,))
        assert mr.same_bits(one[k], full[k]) and all(v is None for n, v in one.items() if n != k)


def test_cylinders_equal_the_host_function_bitwise():
    from core.utils.skeleton_utils import get_kp_bounding_cylinder
    for ext_scale in (0.00035, 0.001):
        ext = mr.extensions(ext_scale)
        out = mr.host_chain(rots32(mr.random_bones(2000, seed=3)), mr.rest_pose(), mr.random_roots(2000), ext=ext)
        want = get_kp_bounding_cylinder(out["kps"], ext_scale=ext_scale, extend_mm=250, top_expand_ratio=1.60, bot_expand_ratio=1.10,
                                        head='-y')
        assert want.dtype == F32 and mr.same_bits(out["cyls"], want)


def test_max_and_min_do_not_depend_on_the_order():
    """-0 orders below +0 and a NaN wins from either side: the serial sweep and a tree reduction then give the same bits"""
    lib = mr.host_lib()
    for a, b in ((0.0, -0.0), (-0.0, 0.0)):
        assert not np.signbit(lib.ref_max(a, b)) and np.signbit(lib.ref_min(a, b))
    for a, b in ((1.5, -2.0), (-2.0, 1.5)):
        assert lib.ref_max(a, b) == 1.5 and lib.ref_min(a, b) == -2.0
    for a, b in ((float("nan"), 1.0), (1.0, float("nan")), (float("nan"), float("inf"))):
        assert np.isnan(lib.ref_max(a, b)) and np.isnan(lib.ref_min(a, b))
    # a NaN joint: the pose's radius, top and bottom are NaN as numpy's max and min make them, the root columns are not
    rots = np.tile(np.eye(3, dtype=F32), (1, J, 1, 1))
    rots[0, 7, 1, 1] = np.nan
    out = mr.host_chain(rots, mr.rest_pose(), None)
    assert np.isnan(out["cyls"][0, 2:]).all() and not np.isnan(out["cyls"][0, :2]).any()


@pytest.mark.parametrize("case", ["random", "identity"] + [f"theta={t:g}" for t in mr.THETAS])
def test_chain_against_float64(case):
    N = 130 if case == "random" else 3
    bones = mr.random_bones(N, seed=5) if case == "random" else np.zeros((N, J, 3), F32) if case == "identity" else \
        mr.one_joint_bones(N, float(case.split("=")[1]))
    rest, roots = mr.rest_pose(), mr.random_roots(N, seed=6)
    got = mr.host_chain(rots32(bones), rest, roots)
    l2w64, skt64 = mr.chain64(bones, rest, roots)
    rot, trans, inv, reach = mr.chain_bounds(rest, roots, N)
    err = lambda a, b: np.abs(a.astype(F64) - b)      # noqa: E731
    e_rot, e_t = err(got["l2ws"][..., :3, :3], l2w64[..., :3, :3]).max((-1, -2)), err(got["l2ws"][..., :3, 3], l2w64[..., :3, 3]).max(-1)
    e_irot, e_it = err(got["skts"][..., :3, :3], skt64[..., :3, :3]).max((-1, -2)), err(got["skts"][..., :3, 3], skt64[..., :3, 3]).max(-1)
    print(f"{case}: rotation {(e_rot / rot).max():.3f}, translation {(e_t / trans).max():.3f}, inverse rotation "
          f"{(e_irot / rot).max():.3f}, inverse translation {(e_it / inv).max():.3f} of their bounds")
    assert np.all(e_rot <= rot) and np.all(e_t <= trans) and np.all(e_irot <= rot) and np.all(e_it <= inv)
    # skt . l2w - I, formed in float64 from the float32 outputs
    prod = got["skts"].astype(F64) @ got["l2ws"].astype(F64) - np.eye(4)
    t_len = np.linalg.norm(got["l2ws"][..., :3, 3].astype(F64), axis=-1)
    assert np.all(np.abs(prod[..., :3, :3]).max((-1, -2)) <= 2.01 * rot) and np.all(np.abs(prod[..., :3, 3]).max(-1) <= 3.1 * E * t_len)
    assert np.all(prod[..., 3, :] == 0)
    if case == "identity":
        assert mr.same_bits(got["l2ws"][..., :3, :3], np.tile(np.eye(3, dtype=F32), (N, J, 1, 1)))
        assert np.all(np.abs(got["kps"].astype(F64) - (rest.astype(F64) + roots[:, None].astype(F64))) <= trans[..., None])


# ----------------------------------------------------------------------------- box rays
@pytest.mark.parametrize("name", sorted(mr.BOXES))
def test_box_rays_restatement_numpy_and_get_rays(name):
    import torch
    from core.utils.ray_utils import get_rays
    H, W, focal, center, tl, br = mr.BOXES[name]
    c2w = mr.camera(seed=len(name))
    o, d, idx = mr.host_box_rays(c2w, *mr.box_scalars(name))
    o32, d32, idx32 = mr.box_rays32(c2w, *mr.box_scalars(name))
    assert mr.same_bits(o, o32) and mr.same_bits(d, d32) and mr.same_bits(idx, idx32)
    n = (br[0] - tl[0]) * (br[1] - tl[1])
    assert len(idx) == n
    if name.startswith("empty"):
        assert n == 0
        return
    # get_rays of the whole image, indexed by the box as kp_to_valid_rays indexes it
    ray_o, ray_d = get_rays(H, W, focal, torch.tensor(c2w), center=center)
    vh, vw = torch.meshgrid(torch.arange(tl[1], br[1]), torch.arange(tl[0], br[0]), indexing='ij')
    want_idx = (vh * W + vw).reshape(-1)
    assert np.array_equal(idx, want_idx.numpy())
    want_o, want_d = ray_o.reshape(-1, 3)[want_idx].numpy(), ray_d.reshape(-1, 3)[want_idx].numpy()
    fx, fy, cx, cy = mr.box_scalars(name)[:4]
    x, y = (idx % W).astype(F64), (idx // W).astype(F64)
    dirs = np.abs(np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(n)], -1))
    bound = 4 * E * (dirs[:, None, :] * np.abs(c2w[:3, :3].astype(F64))[None]).sum(-1) * (1 + 4 * E)      # (the p_i carry 2 roundings)
    print(f"{name}: rays_d bitwise equal to get_rays: {mr.same_bits(d, want_d)}; max |diff| / bound {np.max(np.abs(d - want_d) / bound):.3f}")
    assert mr.same_bits(o, want_o) and np.all(np.abs(d.astype(F64) - want_d) <= bound)


# ----------------------------------------------------------------------------- the sequence builders
@pytest.fixture(scope="module")
def data():
    from core.load_data import synthetic_arrays
    return synthetic_arrays(n_poses=5, n_cams=2, H=32, W=32, pose_seed=3)


def test_retarget_of_length_one_is_selected(data):
    import run_render as rr
    from core import motion
    sel, centers = [7, 2, 4], np.arange(20, dtype=F32).reshape(10, 2)
    src = (data["kp3d"], data["bones"], data["c2ws"], data["focals"], data["rest_pose"], sel)
    kps, skts, c2ws, idxs, focals, bones, cen = rr.load_selected(*src, centers=centers)
    seq = motion.load_retarget(*src, length=1, skip=1, centers=centers)
    assert np.array_equal(seq["bones"], bones) and seq["bones"].dtype == bones.dtype and np.array_equal(seq["c2ws"], c2ws)
    assert np.array_equal(seq["cam_idxs"], idxs) and np.array_equal(seq["focals"], focals) and np.array_equal(seq["centers"], cen)
    assert seq["rotmats"] is None
    k2, s2 = rr._pose_chain(seq["bones"], data["rest_pose"], seq["roots"][:, None])
    assert mr.same_bits(k2, kps) and mr.same_bits(s2, skts)
    # runs: length 3 from 7 and 8 of 10 frames, every second frame; the run that starts at 8 ends with the data
    seq = motion.load_retarget(*src[:5], [7, 8], length=3, skip=2, centers=centers, center_kps=True, undo_rot=True)
    assert list(seq["cam_idxs"]) == [7, 9, 8] and np.all(seq["roots"] == 0) and np.array_equal(seq["c2ws"], data["c2ws"][[7, 9, 8]])
    assert np.all(seq["bones"][:, 0] == F32([1.5708, 0, 0])) and np.array_equal(seq["bones"][:, 1:], data["bones"][[7, 9, 8], 1:])
    assert np.all(data["bones"][7, 0] != F32(1.5708))                              # the data was copied, not written


def test_animate_of_all_joints_is_interpolate(data):
    import run_render as rr
    from core import motion
    bones = data["bones"].copy()
    bones[:, [12, 15]] = 0                      # the joints that animate takes from the last pose agree (and blend exactly)
    sel = [1, 6, 4]
    src = (data["kp3d"], bones, data["c2ws"], data["focals"], data["rest_pose"], sel)
    kps, skts, c2ws, idxs, focals, want = rr.load_interpolate(*src, n_step=4)
    seq = motion.load_animate(*src, list(range(J)), n_step=4)
    assert len(want) == 2 * 4 + 1 and mr.same_bits(np.ascontiguousarray(seq["bones"]), np.ascontiguousarray(want))
    assert np.array_equal(seq["c2ws"], c2ws) and np.array_equal(seq["cam_idxs"], idxs) and np.array_equal(seq["focals"], focals)
    k2, s2 = rr._pose_chain(seq["bones"], data["rest_pose"], seq["roots"][:, None])
    assert mr.same_bits(k2, kps) and mr.same_bits(s2, skts)
    # a subset: the other joints are the first pose's, 12 and 15 the last pose's; from_rest zeroes the first pose's joints
    b = data["bones"]
    seq = motion.load_animate(data["kp3d"], b, *src[2:5], [1, 6], [16, 18], n_step=3, from_rest=True)["bones"]
    assert seq.shape == (4, J, 3) and np.all(seq[:, [12, 15]] == b[6][[12, 15]])
    rest_of = [j for j in range(1, J) if j not in (12, 15, 16, 18)]
    assert np.all(seq[:, rest_of] == 0) and np.all(seq[:, 0] == b[1, 0]) and np.all(seq[0, [16, 18]] == 0)
    assert np.array_equal(seq[3, [16, 18]], b[6][[16, 18]])
    assert np.allclose(seq[1, [16, 18]], b[6][[16, 18]] / 3, rtol=1e-6, atol=0)
    with pytest.raises(ValueError, match="0 .. 23"):
        motion.load_animate(*src, [24])


def test_load_motion_start_len_skip_travel(data, tmp_path):
    from scipy.spatial.transform import Rotation
    from core import motion
    file_bones = mr.random_bones(6, seed=11)
    root = np.cumsum(np.full((6, 3), 0.25, F32), 0) * F32([1, 0.5, -2])
    np.savez(tmp_path / "m.npz", bones=file_bones, root=root)
    centers = np.arange(20, dtype=F32).reshape(10, 2)
    args = (data["kp3d"], data["c2ws"], data["focals"])
    seq = motion.load_motion(tmp_path / "m.npz", *args, cam=3, centers=centers)
    anchor = data["kp3d"][3, 0].astype(F32)
    assert np.array_equal(seq["bones"], file_bones) and seq["roots"].shape == (6, 3) and np.all(seq["roots"] == anchor)
    assert np.all(seq["cam_idxs"] == 3) and np.all(seq["c2ws"] == data["c2ws"][3]) and np.all(seq["focals"] == data["focals"][3])
    assert np.all(seq["centers"] == centers[3]) and seq["rotmats"] is None
    seq = motion.load_motion(tmp_path / "m.npz", *args, cam=3, start=1, length=4, skip=2, travel=True)
    assert np.array_equal(seq["bones"], file_bones[[1, 3]]) and seq["centers"] is None
    assert np.array_equal(seq["roots"], (anchor + (root[[1, 3]] - root[1])).astype(F32)) and np.all(seq["roots"][0] == anchor)
    assert np.all(seq["roots"][1] != anchor)
    assert len(motion.load_motion(tmp_path / "m.npz", *args, start=4)["bones"]) == 2
    # kp3d in place of root; rotation matrices in place of axis-angles
    kp = np.zeros((6, J, 3), F32)
    kp[:, 0] = root
    mats = mr.rodrigues64(file_bones).astype(F32)
    np.savez(tmp_path / "r.npz", rotmats=mats, kp3d=kp)
    seq2 = motion.load_motion(tmp_path / "r.npz", *args, cam=3, start=1, length=4, skip=2, travel=True)
    assert np.array_equal(seq2["roots"], seq["roots"]) and mr.same_bits(seq2["rotmats"], mats[[1, 3]])
    back = Rotation.from_rotvec(seq2["bones"].reshape(-1, 3)).as_matrix().reshape(2, J, 3, 3)
    assert np.abs(back - mats[[1, 3]]).max() < 1e-6
    np.savez(tmp_path / "bad.npz", bones=file_bones, rotmats=mats)
    for call in (lambda: motion.load_motion(tmp_path / "bad.npz", *args), lambda: motion.load_motion(tmp_path / "m.npz", *args, start=6),
                 lambda: motion.load_motion(tmp_path / "m.npz", *args, skip=0)):
        with pytest.raises(ValueError):
            call()
    np.savez(tmp_path / "still.npz", bones=file_bones)
    with pytest.raises(ValueError, match="travel"):
        motion.load_motion(tmp_path / "still.npz", *args, travel=True)


def test_the_entry_point_knows_the_new_types():
    import run_render as rr
    base = ["--nerf_args", "a", "--ckptpath", "c", "--dataset", "synthetic", "--entry", "val", "--runname", "r"]
    a = rr.config_parser().parse_args(base)
    assert a.motion_chain == "device" and a.retarget_len == 1 and a.retarget_skip == 1 and a.motion is None and a.render_type == "bullet"
    a = rr.config_parser().parse_args(base + ["--render_type", "animate", "--animate_joints", "16", "18", "--motion_chain", "host"])
    assert a.animate_joints == [16, 18] and a.motion_chain == "host" and set(rr.MOTION_TYPES) == {"retarget", "animate"}


# ----------------------------------------------------------------------------- arguments
def test_the_restatement_rejects_bad_arguments():
    lib = mr.host_lib()
    buf = np.full(64, 7, F32)
    p, f = buf.ctypes.data, (0.0, 0.0, 0.0)
    assert lib.ref_chain(None, p, p, 1, p, p, p, p, *f) == EINVAL and lib.ref_chain(p, None, p, 1, p, p, p, p, *f) == EINVAL
    assert lib.ref_chain(p, p, p, 1, None, None, None, None, *f) == EINVAL
    assert lib.ref_chain(p, p, p, 0, p, p, p, p, *f) == EINVAL and lib.ref_chain(p, p, p, -1, p, p, p, p, *f) == EINVAL
    assert lib.ref_chain(p, p, p, (1 << 20) + 1, p, p, p, p, *f) == EINVAL
    cam = (1.0, 1.0, 0.0, 0.0)
    for W, x0, y0, x1, y1 in ((0, 0, 0, 0, 0), (8, 3, 0, 2, 4), (8, 0, 3, 4, 2), (8, -1, 0, 4, 4), (8, 0, -1, 4, 4), (8, 0, 0, 9, 4),
                              ((1 << 15) + 1, 0, 0, 1, 1), (8, 0, 0, 4, (1 << 15) + 1)):
        assert lib.ref_box_rays(p, *cam, W, x0, y0, x1, y1, p, p, p) == EINVAL, (W, x0, y0, x1, y1)
    assert lib.ref_box_rays(None, *cam, 8, 0, 0, 1, 1, p, p, p) == EINVAL and lib.ref_box_rays(p, *cam, 8, 0, 0, 1, 1, p, p, None) == EINVAL
    assert np.all(buf == 7)


def test_the_entry_points_reject_the_same_before_any_launch():
    """the library's own entries (no GPU: each returns before a launch; ADDR is a host address no check follows)"""
    import core.motion as cm
    cm.lib()
    p, f = ctypes.c_void_p(ADDR), (0.0, 0.0, 0.0)
    rotations, chain, rays = (entry(n) for n in ENTRIES)
    assert rotations(None, 1, p, None) == EINVAL and rotations(p, 1, None, None) == EINVAL
    assert rotations(p, 0, p, None) == EINVAL and rotations(p, -1, p, None) == EINVAL and rotations(p, (1 << 20) + 1, p, None) == EINVAL
    assert chain(None, p, p, 1, p, p, p, p, *f, None) == EINVAL and chain(p, None, p, 1, p, p, p, p, *f, None) == EINVAL
    assert chain(p, p, p, 1, None, None, None, None, *f, None) == EINVAL and chain(p, p, None, 1, None, None, None, None, *f, None) == EINVAL
    assert chain(p, p, p, 0, p, p, p, p, *f, None) == EINVAL and chain(p, p, p, -1, p, p, p, p, *f, None) == EINVAL
    assert chain(p, p, p, (1 << 20) + 1, p, p, p, p, *f, None) == EINVAL
    cam = (1.0, 1.0, 0.0, 0.0)
    for W, x0, y0, x1, y1 in ((0, 0, 0, 0, 0), (8, 3, 0, 2, 4), (8, 0, 3, 4, 2), (8, -1, 0, 4, 4), (8, 0, -1, 4, 4), (8, 0, 0, 9, 4),
                              ((1 << 15) + 1, 0, 0, 1, 1), (8, 0, 0, 4, (1 << 15) + 1)):
        assert rays(p, *cam, W, x0, y0, x1, y1, p, p, p, None) == EINVAL, (W, x0, y0, x1, y1)
    for null in range(4):
        ptrs = [p, p, p, p]
        ptrs[null] = None
        assert rays(ptrs[0], *cam, 8, 0, 0, 1, 1, *ptrs[1:], None) == EINVAL
    # an empty box is accepted and launches nothing (there is no device here to launch on)
    assert rays(p, *cam, 8, 3, 2, 3, 5, p, p, p, None) == 0 and rays(p, *cam, 8, 3, 2, 6, 2, p, p, p, None) == 0


# ----------------------------------------------------------------------------- the header
def test_the_header_binds_as_a_satellite_and_the_library_exports_it():
    import os
    from core import _hip
    import core.mesh_score as cms
    import core.motion as cm
    path = os.path.join(os.path.dirname(_hip.HEADER_PATH), "danbo_motion.h")
    bound = _hip.bind_headers([_hip.header(n).path for n in _hip.HEADERS] + [cms.header().path, path])      # raises on a clash or a struct
    assert len(bound) == len(_hip.HEADERS) + 2 and bound[-1].path == path and not bound[-1].structs
    assert bound[-2].path.endswith("danbo_mesh_score.h") and "danbo_motion.h" not in _hip.HEADERS
    assert tuple(bound[-1].signatures) == ENTRIES
    assert vars(bound[-1].C) == dict(DANBO_MOTION_MAX_POSES=1 << 20, DANBO_MOTION_MAX_DIM=1 << 15)
    assert cm.header().signatures == bound[-1].signatures and cm.MAX_POSES == 1 << 20
    floats = [i for i, t in enumerate(bound[-1].signatures["danbo_pose_chain"]) if t is ctypes.c_float]
    assert floats == [8, 9, 10] and len(bound[-1].signatures["danbo_pose_chain"]) == 12
    l = cm.lib()
    assert l is _hip.lib() and l.danbo_abi_version() == 9
    for name, argtypes in bound[-1].signatures.items():
        fn = getattr(l, name)                                                             # AttributeError: not exported
        assert fn.argtypes == argtypes and fn.restype is ctypes.c_int


def test_tensors_off_the_device_raise():
    import torch
    import core.motion as cm
    b, r = torch.zeros(2, J, 3), torch.zeros(J, 3)
    for call in (lambda: cm.rotations(b), lambda: cm.pose_chain(bones=b, rest_pose=r), lambda: cm.pose_chain(rots=torch.zeros(2, J, 3, 3), rest_pose=r),
                 lambda: cm.box_rays(torch.eye(4), 10.0, None, 8, 8, (0, 0), (4, 4)),
                 lambda: cm.frame_rays(np.eye(4)[None], 8, 8, 10.0, b, torch.zeros(2, 5))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="not both"):
        cm.pose_chain(rest_pose=r)
