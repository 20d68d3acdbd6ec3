"""Turntable normal maps of a mesh (the reference's separate render_mesh.py: every mesh turned through 360 degrees in front of an
orthographic camera, colour 0.5 * normal + 0.5, white background): the reference's views in closed form and the frames drawn by the
library's rasteriser (hip_ops.rasterize_mesh), from device tensors to a uint8 stack on the device."""
import math

import numpy as np
import torch

HALF_EXTENT = 0.6          # the reference's camera: width 1, ortho_ratio 1.2 -> ortho(-0.6, 0.6, ...)
N_FRAMES = 91              # range(0, 361, 4)
STEP_DEG = 4.0


def make_rotate(rx, ry, rz):
    """Rz(rz) Ry(ry) Rx(rx), float64 (angles in radians)"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1., 0., 0.], [0., cx, -sx], [0., sx, cx]])
    Ry = np.array([[cy, 0., sy], [0., 1., 0.], [-sy, 0., cy]])
    Rz = np.array([[cz, -sz, 0.], [sz, cz, 0.], [0., 0., 1.]])
    return Rz @ Ry @ Rx


def base_rotation():
    """what the reference applies to every mesh before it turns it: rot = [[0,1,0],[-1,0,0],[0,0,1]], then
    make_rotate(270, 180, 90 degrees)"""
    rot = np.array([[0., 1., 0.], [-1., 0., 0.], [0., 0., 1.]])
    return make_rotate(math.radians(270.), math.radians(180.), math.radians(90.)) @ rot


def turntable_views(verts, n_frames=N_FRAMES, step_deg=STEP_DEG):
    """The reference's model -> view matrices for the mesh with the vertices `verts` [V,3] (a device tensor), [n_frames,3,4]
    float32 on its device: frame j is  Ry(-(90 + step_deg (j + 1)) degrees) * s * base_rotation(), s = 1 / (y_max - y_min) of the
    rotated vertices -- the mesh is scaled to unit height and NOT centred, as in the reference -- with no translation.  Float64
    in closed form, rounded once to float32; the two extrema are one reduction on the device (one host read)."""
    from core import hip_ops
    hip_ops._on_device((verts, "verts"))
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] == 0:
        raise ValueError("turntable_views: verts must be a non-empty [V, 3] tensor")
    B = base_rotation()
    y = verts.double() @ torch.tensor(B[1], dtype=torch.float64, device=verts.device)
    lo, hi = torch.aminmax(y)
    lo, hi = torch.stack([lo, hi]).tolist()
    if not (hi > lo) or not math.isfinite(hi - lo):
        raise ValueError("turntable_views: the mesh has no finite height")
    views = np.zeros((n_frames, 3, 4))
    for j in range(n_frames):
        views[j, :, :3] = make_rotate(0., math.radians(-(90. + step_deg * (j + 1))), 0.) @ B / (hi - lo)
    return torch.tensor(views.astype(np.float32), device=verts.device)


@torch.no_grad()
def render_turntable(verts, faces, normals=None, colors=None, size=(512, 512), shade="normal", n_frames=N_FRAMES, step_deg=STEP_DEG,
                     background=(1., 1., 1.), flip=False, chunk=16):
    """-> uint8 [n_frames,H,W,3] on the device: the turntable of the mesh, to8b of the rasteriser's float image.  shade 'normal'
    (normals [V,3] float32), 'color' (colors [V,3], uint8 0 .. 255 or float 0 .. 1) or 'flat' (face normals: a bare mesh).  The views
    are drawn `chunk` frames at a time, so that the float images stay bounded.  flip: left to right, the reference's --flip."""
    from core import hip_ops
    if shade == "normal":
        if normals is None:
            raise ValueError("render_turntable: shade 'normal' needs vertex normals")
        attr = normals.float()
    elif shade == "color":
        if colors is None:
            raise ValueError("render_turntable: shade 'color' needs vertex colours")
        attr = colors.float() / 255. if colors.dtype == torch.uint8 else colors.float()
    elif shade == "flat":
        attr = None
    else:
        raise ValueError(f"render_turntable: shade must be normal, color or flat, not {shade!r}")
    H, W = (int(x) for x in size)
    views = turntable_views(verts, n_frames, step_deg)
    out = torch.empty(n_frames, H, W, 3, device=verts.device, dtype=torch.uint8)
    for j in range(0, n_frames, chunk):
        rgb = hip_ops.rasterize_mesh(verts, faces, attr, mode=shade, views=views[j:j + chunk], half_extent=HALF_EXTENT, size=(H, W),
                                     background=background)["rgb"]
        out[j:j + chunk] = (255. * rgb.clamp(0., 1.)).to(torch.uint8)
    return out.flip(2) if flip else out
