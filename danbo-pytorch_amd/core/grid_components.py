"""Connected components of a density grid's inside set on the device, and the filter that drops the components a caller does not
want -- the floaters of an extracted mesh -- before marching cubes (include/danbo_grid_cc.h, csrc/k_grid_cc.hip; the definitions
are stated once in csrc/grid_cc_math.hpp).  The grid never leaves the GPU and nothing here reads a result on the host."""
import torch

from . import _hip

_NEG_INF = float("-inf")


def _entries():
    """{name: function} of the entries of include/danbo_grid_cc.h on _hip.lib(), which has bound them"""
    return {name: getattr(_hip.lib(), name) for name in _hip.header("danbo_grid_cc.h").signatures}


def _grid(sigma, iso, floor, who):
    if not isinstance(sigma, torch.Tensor) or not sigma.is_cuda:
        raise RuntimeError(f"{who}: sigma: expected a CUDA/HIP tensor -- libdanbo_hip has no CPU fallback")
    if sigma.dtype != torch.float32 or sigma.dim() != 3:
        raise ValueError(f"{who}: sigma must be a [nx, ny, nz] float32 grid")
    if sigma.stride(2) != 1:
        raise ValueError(f"{who}: the innermost stride of sigma must be 1")
    nx, ny, nz = sigma.shape
    return (_hip.ptr(sigma), nx, ny, nz, sigma.stride(0), sigma.stride(1), float(floor), float(iso))


def _int32(t, name, shape, device, who):
    if not isinstance(t, torch.Tensor) or t.device != device:
        raise RuntimeError(f"{who}: {name}: expected a tensor on {device} -- libdanbo_hip has no CPU fallback")
    if t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous int32 tensor of shape {tuple(shape)}")
    return t


def grid_components(sigma, iso, floor=_NEG_INF):
    """6-connected components of the inside set of a density grid in device memory (danbo_grid_cc_label).  sigma [nx,ny,nz] float32
    with innermost stride 1 -- a transposed view is taken as it is; every value is read as max(sigma, floor), a NaN as -inf; inside
    = value >= iso (the definitions of ops.marching_cubes).
    -> labels [nx,ny,nz] int32: the smallest logical linear index (i * ny + j) * nz + k of the point's component, -1 outside;
       sizes  [nx,ny,nz] int32: at the index of every label the number of points of its component, 0 elsewhere;
       stats  [4] int32: points inside, components, size of the largest component, its label (ties: the smallest; none: -1).
    All three are contiguous device tensors; five launches on the current stream, no host read, the same bits on every call."""
    grid = _grid(sigma, iso, floor, "grid_components")
    nx, ny, nz = sigma.shape
    n_bytes = _hip.lib().danbo_grid_cc_workspace_bytes(nx, ny, nz)
    if n_bytes == 0:
        raise _hip.HipError(f"grid_components: unsupported grid {nx} x {ny} x {nz} (each dimension 2 .. 1024, fewer than 2^31 points)")
    ws = torch.empty(n_bytes, device=sigma.device, dtype=torch.uint8)
    labels = torch.empty(nx, ny, nz, device=sigma.device, dtype=torch.int32)
    sizes = torch.empty(nx, ny, nz, device=sigma.device, dtype=torch.int32)
    stats = torch.empty(4, device=sigma.device, dtype=torch.int32)
    _hip.call("danbo_grid_cc_label", *grid, _hip.ptr(ws), _hip.ptr(labels), _hip.ptr(sizes), _hip.ptr(stats), _hip.stream())
    return labels, sizes, stats


def keep_components(sigma, iso, floor, labels, sizes, stats, keep_largest=False, min_points=0, fill=None, out=None):
    """The grid without the components that are not kept (danbo_grid_cc_keep).  labels, sizes, stats: grid_components' of the same
    sigma, iso and floor.  A component is kept iff its size >= min_points and (not keep_largest or it is the largest one, stats[3]
    -- read on the device).  out[p] = sigma[p], bit for bit, where p is outside or its component is kept, `fill` elsewhere; fill must
    read as outside (default: floor where floor < iso, else -inf).  out: default torch.empty_strided with sigma's size and strides;
    `sigma` itself filters in place; any other tensor must not overlap sigma.
    -> out, kept [2] int32 (components kept, points kept; a device tensor).  Two launches on the current stream, no host read."""
    grid = _grid(sigma, iso, floor, "keep_components")
    shape, dev = tuple(sigma.shape), sigma.device
    labels = _int32(labels, "labels", shape, dev, "keep_components")
    sizes = _int32(sizes, "sizes", shape, dev, "keep_components")
    stats = _int32(stats, "stats", (4,), dev, "keep_components")
    min_points = int(min_points)
    if min_points < 0:
        raise ValueError("keep_components: min_points must not be negative")
    if fill is None:
        fill = float(floor) if float(floor) < float(iso) else _NEG_INF
    fill = float(fill)
    if not (fill != fill or max(fill, float(floor)) < float(iso)):
        raise ValueError(f"keep_components: fill = {fill} is not outside (max(fill, floor) must lie below iso = {float(iso)})")
    if out is None:
        out = torch.empty_strided(shape, sigma.stride(), device=dev, dtype=torch.float32)
    elif not isinstance(out, torch.Tensor) or out.device != dev:
        raise RuntimeError(f"keep_components: out: expected a tensor on {dev} -- libdanbo_hip has no CPU fallback")
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.stride(2) != 1:
        raise ValueError(f"keep_components: out must be a float32 tensor of shape {shape} with innermost stride 1")
    kept = torch.empty(2, device=dev, dtype=torch.int32)
    _hip.call("danbo_grid_cc_keep", *grid, _hip.ptr(labels), _hip.ptr(sizes), _hip.ptr(stats), 1 if keep_largest else 0, min_points, fill,
              _hip.ptr(out), out.stride(0), out.stride(1), _hip.ptr(kept), _hip.stream())
    return out, kept
