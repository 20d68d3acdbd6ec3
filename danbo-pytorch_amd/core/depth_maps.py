"""Depth and normal maps of the volume renderer on the device (include/danbo_depth.h, csrc/k_depth.hip; the definitions are stated
once in csrc/depth_math.hpp).  The reference forms depth_map = sum(weights * z_vals) in raw2outputs (core/networks/nerf.py:337) and
drops it; here the expected depth and a level (median) depth come from the final composite's weights and sorted depths, and the
normal map from the assembled depth and acc frames of the rendered camera itself.  Nothing here reads a result on the host."""
import numpy as np
import torch

from . import _hip

SPACES = {"camera": 0, "world": 1}


def _entries():
    """{name: function} of the entries of include/danbo_depth.h on _hip.lib(), which has bound them"""
    return {name: getattr(_hip.lib(), name) for name in _hip.header("danbo_depth.h").signatures}


def _device_f32(t, name, who, shape=None):
    """t as the kernels read it: a contiguous float32 device tensor (of `shape`, where given)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a CUDA/HIP tensor -- libdanbo_hip has no CPU fallback")
    if t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{who}: {name} must be a float32 tensor" + (f" of shape {tuple(shape)}" if shape is not None else ""))
    return t.contiguous()


def composite_depth(weights, z_sorted, level=0.5, flat=None):
    """danbo_depth_composite_fwd: weights, z_sorted [R,n] (the final composite's T_i and its sorted depths, n = S + Sf <= 320) ->
    (depth [R] = sum_k w_k z_k, depth_level [R] = z of the first position whose prefix of w reaches `level`; +0 where none does).
    flat: hip_ops.flat_rays()'s result -- only its listed rays are read and written; the rays of constants, whose z_sorted rows
    were never made, keep the +0 the outputs start from, which is their exact result."""
    who = "composite_depth"
    weights = _device_f32(weights, "weights", who)
    if weights.dim() != 2:
        raise ValueError(f"{who}: weights must be [R, n]")
    z_sorted = _device_f32(z_sorted, "z_sorted", who, weights.shape)
    if z_sorted.device != weights.device:
        raise RuntimeError(f"{who}: z_sorted: expected a tensor on {weights.device}")
    R, n = weights.shape
    if not 1 <= n <= 320:
        raise ValueError(f"{who}: 1 <= n <= 320 positions per ray, not {n}")
    if not 0. < float(level) <= 1.:
        raise ValueError(f"{who}: level must lie in (0, 1], not {level}")
    lst = cnt = None
    if flat is not None:
        lst, cnt = flat["ray_list"], flat["ray_count"]
        if lst.dtype != torch.int32 or cnt.dtype != torch.int32 or lst.numel() < R or not lst.is_cuda or not cnt.is_cuda:
            raise ValueError(f"{who}: flat must hold flat_rays()'s int32 ray_list [R] and ray_count [1]")
    alloc = torch.zeros if flat is not None else torch.empty
    out = alloc(2, R, device=weights.device, dtype=torch.float32)
    with torch.cuda.device(weights.device):
        _hip.call("danbo_depth_composite_fwd", _hip.ptr(weights), _hip.ptr(z_sorted), R, n, float(level), _hip.ptr(lst), _hip.ptr(cnt),
                  _hip.ptr(out[0]), _hip.ptr(out[1]), _hip.stream())
    return out[0], out[1]


def camera_rows(c2ws, focals, centers, N, H, W, device):
    """(c2w [N,3,4], intr [N,4] = (fx, fy, cx, cy)) float32 on `device` from what render_path takes: c2ws [N,4,4] or [N,3,4], focals
    (a float, [N] or [N,2]), centers ([N,2] or None: (W / 2, H / 2), get_rays' default).  Host arrays are uploaded."""
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)      # noqa: E731
    c2w = host(c2ws).astype(np.float32)
    if c2w.shape not in ((N, 4, 4), (N, 3, 4)):
        raise ValueError(f"normal_maps: c2ws must be [{N}, 4, 4] or [{N}, 3, 4]")
    f = host(focals).astype(np.float32)
    f = np.full((N, 1), f, np.float32) if f.ndim == 0 else f.reshape(N, -1)
    if f.shape[1] not in (1, 2):
        raise ValueError("normal_maps: focals must hold one or two values per frame")
    intr = np.empty((N, 4), np.float32)
    intr[:, 0], intr[:, 1] = f[:, 0], f[:, -1]
    if centers is None:
        intr[:, 2], intr[:, 3] = np.float32(W) * np.float32(0.5), np.float32(H) * np.float32(0.5)
    else:
        c = host(centers).astype(np.float32)
        if c.shape != (N, 2):
            raise ValueError(f"normal_maps: centers must be [{N}, 2]")
        intr[:, 2:] = c
    up = lambda a: torch.tensor(np.ascontiguousarray(a), device=device)      # noqa: E731
    return up(c2w[:, :3, :]), up(intr)


def normal_maps(depth, acc, c2ws, focals, centers=None, cast_mask=None, acc_min=0.5, jump=0., space='camera', background=1.,
                return_valid=False):
    """danbo_depth_normals: the normal map of N assembled frames.  depth, acc [N,H,W] float32 on the device (render_path's depth and
    acc frames: 0 outside the cast box), cast_mask [N,H,W] bool / uint8 on the device or None; c2ws, focals, centers as render_path
    takes them (camera_rows).  A pixel is usable iff cast, acc >= acc_min and depth / acc > 0; jump > 0 leaves out neighbours whose
    depth differs by more; space 'camera' (x right, y up, z towards the camera) or 'world' (rotated by c2w[:3,:3]: comparable with
    the mesh turntable's normals).  -> [N,H,W,3] float32 on the device: 0.5 n + 0.5, `background` where a pixel has no normal
    (return_valid: also the [N,H,W] uint8 mask of the pixels that have one)."""
    who = "normal_maps"
    depth = _device_f32(depth, "depth", who)
    if depth.dim() != 3:
        raise ValueError(f"{who}: depth must be [N, H, W]")
    N, H, W = depth.shape
    acc = _device_f32(acc, "acc", who, depth.shape)
    if space not in SPACES:
        raise ValueError(f"{who}: space must be one of {sorted(SPACES)}, not {space!r}")
    if not float(jump) >= 0.:
        raise ValueError(f"{who}: jump must be >= 0, not {jump}")
    if N < 1 or not (1 <= H <= 4096 and 1 <= W <= 4096):
        raise ValueError(f"{who}: N >= 1 frames of 1 .. 4096 pixels a side, not {tuple(depth.shape)}")
    if cast_mask is not None:
        if not isinstance(cast_mask, torch.Tensor) or cast_mask.device != depth.device:
            raise RuntimeError(f"{who}: cast_mask: expected a tensor on {depth.device} -- libdanbo_hip has no CPU fallback")
        if cast_mask.dtype not in (torch.bool, torch.uint8) or tuple(cast_mask.shape) != (N, H, W):
            raise ValueError(f"{who}: cast_mask must be a bool or uint8 tensor of shape {(N, H, W)}")
        cast_mask = cast_mask.contiguous().view(torch.uint8)
    c2w, intr = camera_rows(c2ws, focals, centers, N, H, W, depth.device)
    out = torch.empty(N, H, W, 3, device=depth.device, dtype=torch.float32)
    valid = torch.empty(N, H, W, device=depth.device, dtype=torch.uint8) if return_valid else None
    with torch.cuda.device(depth.device):
        _hip.call("danbo_depth_normals", _hip.ptr(depth), _hip.ptr(acc), _hip.ptr(cast_mask), _hip.ptr(c2w), _hip.ptr(intr), N, H, W,
                  float(acc_min), float(jump), SPACES[space], float(background), _hip.ptr(out), _hip.ptr(valid), _hip.stream())
    return (out, valid) if return_valid else out
