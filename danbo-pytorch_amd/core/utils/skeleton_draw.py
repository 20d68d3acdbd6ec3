"""The skeleton overlay on the device: the posed skeleton projected into every frame and drawn over it (reference
core/utils/skeleton_utils.py: skeleton3d_to_2d :478-491, draw_skeletons_3d / draw_skeletons / draw_skeleton2d :1577-1612, which go
through cv2.line on the host) -- include/danbo_skel.h, csrc/k_skel.hip; the definitions are stated once in csrc/skel_math.hpp.  The
coverage rule is this project's own and exact (a pixel is covered iff its centre lies within width / 2 of the segment), not
cv2.line's.  The frames stay where they are; nothing here reads a result on the host."""
import numpy as np
import torch

from .. import _hip
from .skeleton_utils import SMPLSkeleton, nerf_c2w_to_extrinsic

N_JOINTS = len(SMPLSkeleton.joint_names)
# the reference's colours by the joint's name: (plain, with flip)
_COLOURS = {"left": ((100, 149, 237), (0, 128, 128)), "right": ((255, 0, 0), (128, 128, 0)), None: ((46, 204, 13), (128, 0, 128))}


def _entries():
    """{name: function} of the entries of include/danbo_skel.h on _hip.lib(), which has bound them"""
    return {name: getattr(_hip.lib(), name) for name in _hip.header("danbo_skel.h").signatures}


def bone_colours(flip=False, skel_type=SMPLSkeleton):
    """[24,3] uint8: the colour of every bone by its joint's name, as draw_skeleton2d picks it"""
    side = lambda name: "left" if "left" in name else ("right" if "right" in name else None)      # noqa: E731
    return np.array([_COLOURS[side(name)][1 if flip else 0] for name in skel_type.joint_names], dtype=np.uint8)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _frames(imgs, who):
    """imgs as a contiguous [N,H,W,3] float32 or uint8 device tensor; a numpy array is uploaded"""
    if isinstance(imgs, np.ndarray):
        if imgs.dtype not in (np.float32, np.uint8):
            raise ValueError(f"{who}: imgs must be float32 or uint8, not {imgs.dtype}")
        imgs = torch.tensor(np.ascontiguousarray(imgs), device=_device())
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise RuntimeError(f"{who}: imgs: expected a CUDA/HIP tensor or a numpy array -- libdanbo_hip has no CPU fallback")
    if imgs.dtype not in (torch.float32, torch.uint8) or imgs.dim() != 4 or imgs.shape[-1] != 3:
        raise ValueError(f"{who}: imgs must be an [N, H, W, 3] float32 or uint8 tensor")
    if not imgs.is_contiguous():
        raise ValueError(f"{who}: imgs must be contiguous")
    return imgs


def skeleton3d_to_2d(kps, c2ws, H, W, focals, centers=None):
    """The integer segment ends of every bone (danbo_skel_project).  kps [N,24,3] (a device tensor or an array), c2ws [N,4,4] and
    focals (a float, [N] or [N,2]) and centers ([N,2] or None) as the reference takes them; the world-to-camera matrices are made on
    the host with nerf_c2w_to_extrinsic, exactly the reference's path.
    -> ends [N,24,4] int32 on the device: per bone {ax, ay, bx, by} from the joint to its parent; ax = INT32_MIN: not drawn."""
    dev = kps.device if isinstance(kps, torch.Tensor) else _device()
    if dev.type != "cuda":
        raise RuntimeError("skeleton3d_to_2d: kps: expected a CUDA/HIP tensor or a numpy array -- libdanbo_hip has no CPU fallback")
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)      # noqa: E731
    if not isinstance(kps, torch.Tensor):
        kps = torch.tensor(np.asarray(kps, dtype=np.float32), device=dev)
    kps = kps.to(torch.float32).contiguous()
    N = kps.shape[0]
    if kps.dim() != 3 or tuple(kps.shape[1:]) != (N_JOINTS, 3) or N < 1:
        raise ValueError(f"skeleton3d_to_2d: kps must be [N, {N_JOINTS}, 3]")
    c2ws = host(c2ws)
    if c2ws.shape != (N, 4, 4):
        raise ValueError(f"skeleton3d_to_2d: c2ws must be [{N}, 4, 4]")
    w2c = np.array([nerf_c2w_to_extrinsic(c2w) for c2w in c2ws]).astype(np.float32)[:, :3, :]
    focals = host(focals).astype(np.float32)
    focals = np.full((N, 1), focals, np.float32) if focals.ndim == 0 else focals.reshape(N, -1)
    if focals.shape[1] not in (1, 2):
        raise ValueError("skeleton3d_to_2d: focals must hold one or two values per frame")
    up = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)      # noqa: E731
    if centers is not None:
        centers = host(centers)
        if centers.shape != (N, 2):
            raise ValueError(f"skeleton3d_to_2d: centers must be [{N}, 2]")
        centers = up(centers)
    w2c, focals_d = up(w2c), up(focals)
    ends = torch.empty(N, N_JOINTS, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("danbo_skel_project", _hip.ptr(kps), _hip.ptr(w2c), _hip.ptr(focals_d), focals.shape[1], _hip.ptr(centers), N, int(H),
                  int(W), _hip.ptr(ends), _hip.stream())
    return ends


def draw_skeletons(imgs, ends, width=3, flip=False, skel_type=SMPLSkeleton):
    """The overlay of callers that already hold 2-D ends (danbo_skel_draw).  imgs [N,H,W,3] float32 or uint8, a device tensor or a
    numpy array (uploaded); ends [N,24,4] int32 on the device (skeleton3d_to_2d's).  -> [N,H,W,3] uint8 on the device: the frame --
    a float32 one quantised as (rgb * 255).astype(uint8) -- with bones 0 .. 23 painted in order at `width` pixels."""
    imgs = _frames(imgs, "draw_skeletons")
    N, H, W, _ = imgs.shape
    if not isinstance(ends, torch.Tensor) or ends.device != imgs.device:
        raise RuntimeError(f"draw_skeletons: ends: expected a tensor on {imgs.device} -- libdanbo_hip has no CPU fallback")
    if ends.dtype != torch.int32 or tuple(ends.shape) != (N, N_JOINTS, 4) or not ends.is_contiguous():
        raise ValueError(f"draw_skeletons: ends must be a contiguous int32 tensor of shape {(N, N_JOINTS, 4)}")
    colours = torch.tensor(bone_colours(flip, skel_type), device=imgs.device)
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=imgs.device)
    with torch.cuda.device(imgs.device):
        _hip.call("danbo_skel_draw", _hip.ptr(imgs), 1 if imgs.dtype == torch.float32 else 0, _hip.ptr(ends), _hip.ptr(colours), int(width),
                  N, H, W, _hip.ptr(out), _hip.stream())
    return out


def draw_skeletons_3d(imgs, skels, c2ws, H, W, focals, centers=None, width=3, flip=False, skel_type=SMPLSkeleton):
    """The reference's draw_skeletons_3d: `imgs` with the skeletons `skels` [N,24,3] seen through c2ws drawn over them.
    -> [N,H,W,3] uint8 on the device (two launches on the current stream, no host read)."""
    imgs = _frames(imgs, "draw_skeletons_3d")
    kps = skels if isinstance(skels, torch.Tensor) else torch.tensor(np.asarray(skels, dtype=np.float32), device=imgs.device)
    return draw_skeletons(imgs, skeleton3d_to_2d(kps, c2ws, H, W, focals, centers), width, flip, skel_type)
