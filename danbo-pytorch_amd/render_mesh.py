"""Turntable normal maps of the meshes of a run (the reference's render_mesh.py, which needs an OpenGL / EGL context, PyOpenGL,
trimesh and cv2; here the library's own rasteriser draws them on the GPU).

Reads `<basedir>/<expname>/meshes/*.ply` (what `run_render.py --render_mesh` writes) and writes, per mesh, the 91 frames of the
reference's turntable as one uint8 stack `<basedir>/<expname>/mesh_render/NNN.npy` of shape [91, H, W, 3] (an `.npy` stack like
run_render's `image.npy`: there is no image encoder here).  --shade normal (default) draws 0.5 * normal + 0.5 of the vertex normals
in the file (`--mesh_normals`); a file without normals is drawn with its face normals (flat) and the tool says so.  --shade color
draws the vertex colours (`--mesh_colors`), --shade flat the face normals."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from core.utils.mesh_io import read_ply_attrs  # noqa: E402
from core.utils.mesh_render import render_turntable  # noqa: E402


def config_parser():
    p = argparse.ArgumentParser()
    p.add_argument('-ww', '--width', type=int, default=512)
    p.add_argument('-hh', '--height', type=int, default=512)
    p.add_argument('--expname', type=str, default=None)
    p.add_argument('--basedir', type=str, default='render_output/')
    p.add_argument('--mesh_ind', type=int, default=None)
    p.add_argument('--skip', type=int, default=1)
    p.add_argument('--flip', action='store_true', help='flip the rendered geometry left to right')
    p.add_argument('--shade', type=str, default='normal', choices=['normal', 'color', 'flat'])
    return p


def pick_shade(shade, attrs, path):
    """the shading a file can be drawn with: normal falls back to flat (and says so), color without colours is an error"""
    if shade == 'normal' and 'normals' not in attrs:
        print(f'{path}: no vertex normals in the file, drawing face normals (--shade flat)')
        return 'flat'
    if shade == 'color' and 'colors' not in attrs:
        raise ValueError(f'{path}: --shade color, but the file has no vertex colours (run_render.py --render_mesh --mesh_colors)')
    return shade


def render_meshes(argv=None):
    args = config_parser().parse_args(argv)
    if args.expname is None:
        raise ValueError('render_mesh.py: --expname is required')
    if not torch.cuda.is_available():
        raise RuntimeError("render_mesh.py drives the HIP rasteriser: no GPU visible")
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    root = os.path.join(args.basedir, args.expname)
    out_dir = os.path.join(root, 'mesh_render')
    os.makedirs(out_dir, exist_ok=True)
    files = sorted(glob.glob(os.path.join(root, 'meshes', '*.ply')))
    files = files[::args.skip] if args.mesh_ind is None else files[args.mesh_ind:args.mesh_ind + 1]
    print(f'the results are saved at {out_dir}')
    written = []
    for i, path in enumerate(files):
        verts, faces, attrs = read_ply_attrs(path)
        print(f'{os.path.basename(path)}: {verts.shape}')
        shade = pick_shade(args.shade, attrs, path)
        to = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), device=device)      # noqa: E731
        frames = render_turntable(to(verts), to(faces), normals=to(attrs.get('normals')), colors=to(attrs.get('colors')),
                                  size=(args.height, args.width), shade=shade, flip=args.flip)
        written.append(os.path.join(out_dir, f'{i:03d}.npy'))
        np.save(written[-1], frames.cpu().numpy())
    return written


if __name__ == '__main__':
    render_meshes()
