"""The set-up of a rendered motion on the device (include/danbo_motion.h, csrc/k_motion.hip; the arithmetic of the chain and of the
rays is stated once in csrc/motion_math.hpp): axis-angle poses to rotation matrices, the kinematic chain of the SMPL tree with its
inverses, joints and bounding cylinders, and the rays of every frame's image box -- what run_render._pose_chain,
get_kp_bounding_cylinder and kp_to_valid_rays do on the host, pose by pose and image by image.  The sequence builders at the end
(load_retarget, load_motion, load_animate) work on small numpy arrays; their output is what gets uploaded.

The header is a satellite that _hip.HEADERS does not list: it is bound here, once, with the public call that binds the table,
after the mesh-score header (so the rule "no struct, no name an earlier header declares" covers both), and the types of its entries
are set on the handle of _hip.lib()."""
import os

import numpy as np
import torch

from . import _hip
from . import mesh_score

HEADER = "danbo_motion.h"
J = 24
_bound = None
_typed = False


def header():
    """what include/danbo_motion.h declares: .path, .signatures, .restypes, .C -- bound beside every header of _hip.HEADERS and the
    mesh-score header"""
    global _bound
    if _bound is None:
        path = os.path.join(os.path.dirname(_hip.HEADER_PATH), HEADER)
        _bound = _hip.bind_headers([_hip.header(n).path for n in _hip.HEADERS] + [mesh_score.header().path, path])[-1]
    return _bound


def lib():
    """_hip.lib() with the types of this header's entries set (a library that lacks one is stale)"""
    global _typed
    l = _hip.lib()
    if not _typed:
        h = header()
        for name, argtypes in h.signatures.items():
            fn = getattr(l, name, None)
            if fn is None:
                raise RuntimeError(f"{_hip.LIB_PATH} has no {name}, which {h.path} declares: "
                                   "the library is stale, rebuild it with `make -C danbo-pytorch_amd/csrc`")
            fn.argtypes = argtypes
            fn.restype = h.restypes[name]
        _typed = True
    return l


MAX_POSES = header().C.DANBO_MOTION_MAX_POSES
MAX_DIM = header().C.DANBO_MOTION_MAX_DIM
# the cylinder of the render path (core/utils/ray_utils.kp_to_valid_rays): 250 mm, grown 1.6 x above and 1.1 x below
EXTEND_MM, TOP_RATIO, BOT_RATIO = 250, 1.60, 1.10


def _call(name, *args):
    _hip.check(getattr(lib(), name)(*args), name)


def _device(t, name, who, shape):
    """t as the kernels read it: a contiguous float32 device tensor whose trailing dimensions are `shape`"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a CUDA/HIP tensor -- libdanbo_hip has no CPU fallback")
    if t.dtype != torch.float32 or t.dim() < len(shape) or tuple(t.shape[t.dim() - len(shape):]) != tuple(shape):
        raise ValueError(f"{who}: {name} must be a float32 tensor of shape [..., {', '.join(map(str, shape))}]")
    return t.contiguous()


def _poses(t, name, who, shape):
    t = _device(t, name, who, shape)
    if t.dim() != len(shape) + 1 or not 1 <= t.shape[0] <= MAX_POSES:
        raise ValueError(f"{who}: {name} must hold 1 .. 2^20 poses as [N, {', '.join(map(str, shape))}], not {tuple(t.shape)}")
    return t


def rotations(bones):
    """danbo_pose_rotations: bones [N,24,3] axis-angles, float32 on the device -> rots [N,24,3,3]"""
    bones = _poses(bones, "bones", "rotations", (J, 3))
    rots = torch.empty(bones.shape[0], J, 3, 3, device=bones.device, dtype=torch.float32)
    with torch.cuda.device(bones.device):
        _call("danbo_pose_rotations", _hip.ptr(bones), bones.shape[0], _hip.ptr(rots), _hip.stream())
    return rots


def cylinder_extensions(ext_scale):
    """(ext, ext_top, ext_bot) of the render path's cylinder as get_kp_bounding_cylinder adds them to float32 joints: Python floats
    that the call rounds to float32"""
    ext = EXTEND_MM * ext_scale
    return ext, ext * TOP_RATIO, ext * BOT_RATIO


def pose_chain(bones=None, rots=None, *, rest_pose, roots=None, ext_scale=0.00035, cylinders=True):
    """danbo_pose_chain on N poses given as axis-angles `bones` [N,24,3] (through rotations()) or as matrices `rots` [N,24,3,3];
    rest_pose [24,3]; roots [N,3] or [N,1,3] or None -- all float32 on the device.  -> dict(l2ws [N,24,4,4], skts [N,24,4,4],
    kps [N,24,3], cyls [N,5] or None without `cylinders`): what run_render._pose_chain and get_kp_bounding_cylinder(kps,
    ext_scale=ext_scale, extend_mm=250, top_expand_ratio=1.6, bot_expand_ratio=1.1, head='-y') compute on the host."""
    who = "pose_chain"
    if (bones is None) == (rots is None):
        raise ValueError(f"{who}: bones or rots, not both")
    rots = rotations(bones) if rots is None else _poses(rots, "rots", who, (J, 3, 3))
    N, dev = rots.shape[0], rots.device
    rest_pose = _device(rest_pose, "rest_pose", who, (J, 3))
    if rest_pose.dim() != 2 or rest_pose.device != dev:
        raise ValueError(f"{who}: rest_pose must be [24, 3] on {dev}")
    if roots is not None:
        roots = _device(roots, "roots", who, (3,)).reshape(-1, 3)
        if roots.shape[0] != N or roots.device != dev:
            raise ValueError(f"{who}: roots must hold one position per pose, on {dev}")
    out = dict(l2ws=torch.empty(N, J, 4, 4, device=dev), skts=torch.empty(N, J, 4, 4, device=dev), kps=torch.empty(N, J, 3, device=dev),
               cyls=torch.empty(N, 5, device=dev) if cylinders else None)
    with torch.cuda.device(dev):
        _call("danbo_pose_chain", _hip.ptr(rots), _hip.ptr(rest_pose), _hip.ptr(roots), N, _hip.ptr(out["l2ws"]), _hip.ptr(out["skts"]),
              _hip.ptr(out["kps"]), _hip.ptr(out["cyls"]), *cylinder_extensions(ext_scale), _hip.stream())
    return out


def _focals(focal):
    """(fx, fy) as core.utils.ray_utils.get_rays reads a focal"""
    if isinstance(focal, float) or len(np.reshape(focal, -1)) < 2:
        fx = fy = float(np.reshape(focal, -1)[0])
    else:
        fx, fy = (float(f) for f in focal)
    return fx, fy


def box_rays(c2w, focal, center, H, W, tl, br):
    """danbo_box_rays: the rays of the pixels tl[0] <= x < br[0], tl[1] <= y < br[1] of the H x W image of camera c2w ([4,4] or
    [3,4] float32 on the device; focal a number or (fx, fy); center (cx, cy) or None: the image's middle) -> rays_o [n,3],
    rays_d [n,3], idx [n] int64 (y W + x), all on the device, in row-major order of the box: get_rays(H, W, focal, c2w, center)
    indexed by the box."""
    who = "box_rays"
    c2w = _device(c2w, "c2w", who, (4,))
    if c2w.dim() != 2 or c2w.shape[0] < 3:
        raise ValueError(f"{who}: c2w must be [4, 4] or [3, 4]")
    fx, fy = _focals(focal)
    cx, cy = (W * 0.5, H * 0.5) if center is None else (float(center[0]), float(center[1]))
    x0, y0, x1, y1 = int(tl[0]), int(tl[1]), int(br[0]), int(br[1])
    if not (0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H):
        raise ValueError(f"{who}: the box ({x0}, {y0}) .. ({x1}, {y1}) does not lie in the {H} x {W} image")
    n = (x1 - x0) * (y1 - y0)
    rays_o = torch.empty(n, 3, device=c2w.device, dtype=torch.float32)
    rays_d = torch.empty(n, 3, device=c2w.device, dtype=torch.float32)
    idx = torch.empty(n, device=c2w.device, dtype=torch.int64)
    if n == 0:      # (tensors without elements have no address to hand over)
        return rays_o, rays_d, idx
    with torch.cuda.device(c2w.device):
        _call("danbo_box_rays", _hip.ptr(c2w), fx, fy, cx, cy, int(W), x0, y0, x1, y1, _hip.ptr(rays_o), _hip.ptr(rays_d), _hip.ptr(idx),
              _hip.stream())
    return rays_o, rays_d, idx


def frame_rays(render_poses, H, W, focal, kps, cyls, centers=None):
    """The device form of core.utils.ray_utils.kp_to_valid_rays: render_poses [F,4,4] (numpy: uploaded once; or a device tensor:
    read back once), kps [N,24,3] and cyls [N,5] device tensors (pose_chain's), focal a float or one entry per frame, centers None
    or one (cx, cy) per frame.  The boxes come from cylinder_to_box_2d on the host, from ONE device-to-host copy of cyls for the
    whole sequence; the rays of every frame from one danbo_box_rays launch.  -> rays [(o, d)], flat pixel indices, cylinders, boxes
    as kp_to_valid_rays returns them, rays and indices on the device."""
    from .utils.skeleton_utils import cylinder_to_box_2d, nerf_c2w_to_extrinsic
    who = "frame_rays"
    cyls = _device(cyls, "cyls", who, (5,))
    if isinstance(render_poses, torch.Tensor):
        poses_dev = render_poses.to(device=cyls.device, dtype=torch.float32).contiguous()
        poses = render_poses.cpu().numpy()
    else:
        poses = np.asarray(render_poses)
        poses_dev = torch.tensor(np.ascontiguousarray(poses), dtype=torch.float32, device=cyls.device)
    cyl_host = cyls.cpu().numpy()
    rays, valid_idxs, bboxes = [], [], []
    for i, c2w in enumerate(poses):
        cyl = cyl_host[i % kps.shape[0]]
        f = focal if isinstance(focal, float) else focal[i]
        center = None if centers is None else centers[i]
        h = H if isinstance(H, int) else int(H[i])
        w = W if isinstance(W, int) else int(W[i])
        tl, br, _ = cylinder_to_box_2d(cyl, [h, w, f], nerf_c2w_to_extrinsic(c2w), center=center)
        ray_o, ray_d, idx = box_rays(poses_dev[i], f, center, h, w, tl, br)
        rays.append((ray_o, ray_d))
        valid_idxs.append(idx)
        bboxes.append((tl, br))
    return rays, valid_idxs, cyls, bboxes


# ---------------------------------------------------------------------------------------------------- sequences (host, numpy)
def _sequence(bones, roots, c2ws, cam_idxs, focals, centers=None, rotmats=None):
    # (bones and roots keep the data's type: the host chain then computes what the other loaders compute; an upload rounds them)
    return dict(bones=np.asarray(bones), roots=np.asarray(roots), c2ws=c2ws, cam_idxs=np.asarray(cam_idxs), focals=focals, centers=centers,
                rotmats=None if rotmats is None else np.ascontiguousarray(rotmats, dtype=np.float32))


def _camera_focals(focals, idxs):
    return np.array([focals] * len(idxs)) if isinstance(focals, float) else focals[idxs]


def load_retarget(kps, bones, c2ws, focals, rest_pose, selected_idxs, length=1, skip=1, centers=None, center_kps=False, undo_rot=False):
    """Runs of `length` consecutive frames from every selected index, every `skip`-th of them, each with its own camera (reference
    run_render.py:660-724, without its stray breakpoint).  center_kps moves every pose's root to the origin, undo_rot replaces the
    root rotation by a quarter turn about x.  -> the sequence: dict(bones [F,24,3], roots [F,3], c2ws, cam_idxs, focals, centers,
    rotmats=None); the chain (pose_chain here, run_render._pose_chain on the host) makes kps and skts from bones, rest_pose and
    roots.  rest_pose is not read: it is an argument so that every loader takes the same tuple."""
    idxs = np.asarray(selected_idxs)
    if skip > 1 or length > 1:
        idxs = np.concatenate([np.arange(s, min(s + length, len(c2ws)))[::skip] for s in idxs])
    seq_bones = bones[idxs].copy()
    roots = kps[idxs][:, 0].copy()
    if center_kps:
        roots -= roots.copy()
    if undo_rot:
        seq_bones[..., 0, :] = np.array([1.5708, 0., 0.], dtype=np.float32)
    return _sequence(seq_bones, roots, c2ws[idxs].copy(), idxs, _camera_focals(focals, idxs),
                     centers[idxs] if centers is not None else None)


def load_motion(file, kps, c2ws, focals, cam=0, start=0, length=None, skip=1, travel=False, centers=None):
    """Poses from an .npz driven through the model's own skeleton: `bones` [F,24,3] axis-angles, or `rotmats` [F,24,3,3] (they go
    straight into pose_chain(rots=); the axis-angles the network is conditioned on are scipy's as_rotvec of them); optional `root`
    [F,3], or `kp3d` [F,24,3] whose joint 0 is the root.  Frames start, start + skip, ... below start + length (length None: to the
    end of the file).  Every frame is seen from the one dataset camera `cam` (its c2w, focal and centre) and the motion's first
    frame is anchored at that dataset frame's root kps[cam, 0]; with `travel` the file's root displacement relative to its first
    frame is added.  -> the sequence of load_retarget (rotmats set when the file holds them)."""
    with np.load(file) as d:
        if ("bones" in d) == ("rotmats" in d):
            raise ValueError(f"{file}: one of bones [F,24,3] and rotmats [F,24,3,3]")
        pose = np.asarray(d["bones"] if "bones" in d else d["rotmats"], dtype=np.float32)
        is_mat = "rotmats" in d
        root = np.asarray(d["root"], np.float32) if "root" in d else np.asarray(d["kp3d"], np.float32)[:, 0] if "kp3d" in d else None
    if pose.shape[1:] != ((J, 3, 3) if is_mat else (J, 3)):
        raise ValueError(f"{file}: poses of shape {pose.shape}, expected [F, 24, 3{', 3' if is_mat else ''}]")
    if start < 0 or skip < 1 or (length is not None and length < 1) or start >= len(pose):
        raise ValueError(f"{file}: start {start}, length {length}, skip {skip} select nothing of {len(pose)} frames")
    pick = slice(start, None if length is None else start + length, skip)
    pose = pose[pick]
    n = len(pose)
    anchor = np.asarray(kps[cam, 0], dtype=np.float32)
    roots = np.repeat(anchor[None], n, 0)
    if travel:
        if root is None or len(root) < start + 1:
            raise ValueError(f"{file}: travel needs root [F,3] or kp3d [F,24,3]")
        roots = roots + (root[pick] - root[start])
    if is_mat:
        from scipy.spatial.transform import Rotation
        seq_bones = Rotation.from_matrix(pose.reshape(-1, 3, 3).astype(np.float64)).as_rotvec().reshape(n, J, 3)
    else:
        seq_bones = pose
    cams = np.full(n, cam)
    return _sequence(seq_bones, roots, c2ws[cams].copy(), cams, _camera_focals(focals, cams), centers[cams] if centers is not None else None,
                     rotmats=pose if is_mat else None)


def load_animate(kps, bones, c2ws, focals, rest_pose, selected_idxs, joints, n_step=10, from_rest=False, undo_rot=False,
                 center_cam=False, center_kps=False):
    """`n_step` linear blends of the axis-angles of the listed `joints` between consecutive selected poses, laid over the FIRST
    selected pose's other joints, placed at the first pose's root and seen from the first selected camera (reference
    run_render.py:726-798).  from_rest zeroes the first pose's non-root joints.  As the reference does, joints 12 and 15 (neck and
    head) of every frame are taken from the LAST selected pose, whether or not they are listed.  center_cam / center_kps as in
    the reference: the camera is moved onto the z axis and the pose by the same shift, or the pose onto the origin.  The
    reference's camera ring (generate_bullet_time, of which it keeps the first camera) and its halved x offset are not reproduced:
    the first selected camera is used as it is.  -> the sequence of load_retarget."""
    idxs = np.asarray(selected_idxs)
    joints = np.asarray(joints, dtype=np.int64)
    if joints.size == 0 or joints.min() < 0 or joints.max() >= J:
        raise ValueError("animate: --animate_joints takes joint indices 0 .. 23")
    cams = c2ws[idxs].copy()
    if center_cam:
        shift = cams[..., :2, -1].copy()
        cams[..., :2, -1] = 0.
    sel_kps, sel_bones = kps[idxs].copy(), bones[idxs].copy()
    if center_kps:
        sel_kps -= sel_kps[..., :1, :].copy()
    elif center_cam:
        sel_kps[..., :2] -= shift[:, None]
    if from_rest:
        sel_bones[:1, 1:] = 0
    if undo_rot:
        sel_bones[..., 0, :] = np.array([0., 0., 1.5708 * 2], dtype=np.float32)
    w = np.linspace(0, 1.0, n_step, endpoint=False).reshape(-1, 1, 1)
    blends = [sel_bones[i:i + 1, joints] * (1 - w) + sel_bones[i + 1:i + 2, joints] * w for i in range(len(sel_bones) - 1)]
    blends = np.concatenate(blends + [sel_bones[-1:, joints]], axis=0)
    n = len(blends)
    seq = sel_bones[:1].repeat(n, 0).astype(blends.dtype)
    seq[:, joints] = blends
    seq[:, [12, 15]] = sel_bones[-1, [12, 15], :]
    return _sequence(seq, sel_kps[:1, 0].repeat(n, 0), cams[:1].repeat(n, 0), idxs[:1].repeat(n, 0), _camera_focals(focals, idxs)[:1].repeat(n, 0))
