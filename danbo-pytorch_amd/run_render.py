"""Rendering entry point (reference: run_render.py -- parser :31-97, `load_nerf` :99-134, sequence loaders :838-999,
`evaluate_metric` :1178-1263, `render_mesh` :1266-1281, `run_render` :1283-1347).

    python danbo-pytorch_amd/run_render.py --nerf_args logs/demo/args.txt --ckptpath logs/demo/001000.tar \
        --dataset synthetic --entry val --render_type bullet --runname demo_bullet --render_res 256 256 [--eval]

A trained model (the reference's `args.txt` + `.tar` checkpoint formats) is rendered along a generated camera / pose
sequence -- `bullet` (camera ring around selected poses), `interpolate` (axis-angle blend between selected poses), `bubble`
(camera wobbling around its position), `val` /
`selected` (the data's own cameras), `retarget` (runs of the data's frames, or with `--motion FILE` a motion of one's own driven
through the trained skeleton), `animate` (listed joints blended between selected poses; for these two the chain, the cylinders and
the rays of every frame are made on the device, core/motion.py, unless `--motion_chain host`) -- or sampled on a density grid
(`--render_mesh`).  The sequence generators take arrays instead of the reference's HDF5 paths (no h5py / deepdish here);
`--dataset synthetic` builds them from seeded poses, `--dataset npz --entry file.npz` reads them.  Outputs: `image/`, `acc/` as .npy stacks (no imageio here), `bboxes.npy`, with
`--eval` `scores.npy` + `score_final.txt` like the reference, and with `--render_skel` the reference's `skel/` as `skel.npy`:
every frame with its posed skeleton drawn over it on the device (core/utils/skeleton_draw.py).  `--render_depth` adds `depth.npy`
(the expected depth sum w z of every pixel of the rendered camera, float32 [N,H,W], 0 outside the cast box) and `depth_med.npy`
(the depth at which the accumulated weight reaches `--depth_level`), `--render_normal` adds `normal.npy` (uint8 [N,H,W,3]): the
normal map of the depth frames, made on the device (core/depth_maps.py).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from core.config import config_parser as nerf_config_parser, txt_to_argstring  # noqa: E402
from core import motion  # noqa: E402
from core.depth_maps import normal_maps  # noqa: E402
from core.load_data import PoseImageDataset, generate_bullet_time, get_dataset  # noqa: E402
from core.raycasters import create_raycaster  # noqa: E402
from core.utils.evaluation_helpers import evaluate_in_boxes, evaluate_in_boxes_device  # noqa: E402
from core.utils.mesh_io import write_ply  # noqa: E402
from core.utils.mesh_render import render_turntable  # noqa: E402
from core.utils.skeleton_draw import draw_skeletons_3d  # noqa: E402
from core.utils.skeleton_utils import get_smpl_l2ws  # noqa: E402
from run_nerf import render_path  # noqa: E402


def config_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--nerf_args', type=str, required=True, help='args.txt in the training log directory')
    p.add_argument('--ckptpath', type=str, required=True, help='checkpoint (.tar)')
    p.add_argument('--render_res', nargs='+', type=int, default=[1000, 1000], help='(H, W) of the rendered images')
    p.add_argument('--dataset', type=str, required=True, help="'synthetic' or 'npz'")
    p.add_argument('--entry', type=str, required=True, help='catalog entry: a split name (synthetic) or an .npz path')
    p.add_argument('--white_bkgd', action='store_true')
    p.add_argument('--render_type', type=str, default='bullet', help='bullet | interpolate | bubble | pose_rotate | selected | val | '
                   'retarget | animate')
    p.add_argument('--render_mesh', action='store_true', help='sample the density grid instead of rendering images')
    p.add_argument('--mesh_res', type=int, default=255)
    p.add_argument('--mesh_radius', type=float, default=1.8)
    p.add_argument('--mesh_threshold', type=float, default=10.0, help='density of the extracted isosurface')
    p.add_argument('--mesh_normals', action='store_true', help='with --render_mesh: per-vertex normals in the .ply')
    p.add_argument('--mesh_colors', action='store_true', help='with --render_mesh: per-vertex colours (seen head-on) in the .ply')
    p.add_argument('--mesh_keep_largest', action='store_true', help='with --render_mesh: drop the floaters -- keep only the largest '
                   '6-connected component of the grid above the threshold (labelled and filtered on the device, before the extraction)')
    p.add_argument('--mesh_min_points', type=int, default=0, help='with --render_mesh: drop every component of fewer grid points')
    p.add_argument('--mesh_render', nargs='?', const='normal', default=None, choices=['normal', 'color', 'flat'],
                   help='with --render_mesh: the turntable of every mesh (render_mesh.py) straight from the device tensors')
    p.add_argument('--mesh_render_res', nargs=2, type=int, default=[512, 512], help='(H, W) of the turntable frames')
    p.add_argument('--mesh_score', type=str, default=None, metavar='DIR', help='with --render_mesh: score every extracted mesh NNN '
                   'against DIR/NNN.ply while it is on the device (core/mesh_score.py).  mesh_scores.npy holds one row per mesh: '
                   'chamfer_l1, chamfer_l2, normal_consistency, n_points, then precision, recall, fscore of every threshold in the '
                   'order given; mesh_score_final.txt the column means')
    p.add_argument('--mesh_score_points', type=int, default=100_000, help='surface samples per mesh of --mesh_score')
    p.add_argument('--mesh_score_tau', nargs='+', type=float, default=[0.01, 0.02], help='distance thresholds of --mesh_score')
    p.add_argument('--render_confd', action='store_true', help='image.npy holds the part map: every sample coloured by the bone '
                   'with the largest assignment logit')
    p.add_argument('--render_entropy', action='store_true', help='image.npy holds the entropy of the bone assignment, blue (one '
                   'bone) to red (uniform); --render_confd wins when both are given')
    p.add_argument('--part_valid_only', action='store_true', help='with --render_confd / --render_entropy: only the bones whose '
                   'volume holds the sample take part')
    p.add_argument('--render_skel', action='store_true', help='also save skel.npy: every frame with its posed skeleton drawn over it '
                   '(the reference\'s skel/ output), made on the device')
    p.add_argument('--skel_width', type=int, default=3, help='with --render_skel: width of the bones in pixels (1 .. 64)')
    p.add_argument('--skel_flip', action='store_true', help='with --render_skel: the reference\'s second set of colours')
    p.add_argument('--render_depth', action='store_true', help='also save depth.npy (float32 [N,H,W]: the expected depth sum w z of '
                   'every pixel, 0 outside the cast box) and depth_med.npy (the depth where the accumulated weight reaches --depth_level)')
    p.add_argument('--depth_level', type=float, default=0.5, help='with --render_depth: the level of depth_med.npy in (0, 1]; 0.5 is '
                   'the median depth')
    p.add_argument('--render_normal', action='store_true', help='also save normal.npy (uint8 [N,H,W,3]): the normal map of the '
                   'rendered depth, 0.5 n + 0.5, white where a pixel has no normal; made on the device')
    p.add_argument('--normal_space', type=str, default='camera', choices=['camera', 'world'], help='with --render_normal: camera '
                   'space (x right, y up, z towards the camera) or world space (comparable with the mesh turntable)')
    p.add_argument('--normal_acc_min', type=float, default=0.5, help='with --render_normal: a pixel below this opacity has no normal')
    p.add_argument('--normal_jump', type=float, default=0., help='with --render_normal: > 0 leaves out neighbours whose depth differs '
                   'by more (no normals across depth edges)')
    p.add_argument('--retarget_len', type=int, default=1, help='retarget: frames of the run that starts at every selected index')
    p.add_argument('--retarget_skip', type=int, default=1, help='retarget: every k-th frame of a run')
    p.add_argument('--motion', type=str, default=None, metavar='FILE', help='retarget: drive the model with the poses of an .npz '
                   '(bones [F,24,3] axis-angles or rotmats [F,24,3,3]; optional root [F,3] or kp3d [F,24,3]) instead of the data\'s own')
    p.add_argument('--motion_start', type=int, default=0, help='with --motion: the first frame of the file')
    p.add_argument('--motion_len', type=int, default=None, help='with --motion: frames of the file from --motion_start (default: all)')
    p.add_argument('--motion_skip', type=int, default=1, help='with --motion: every k-th of them')
    p.add_argument('--motion_cam', type=int, default=0, help='with --motion: the data frame whose camera sees the motion and at whose '
                   'root its first frame stands')
    p.add_argument('--motion_travel', action='store_true', help='with --motion: add the file\'s root displacement relative to its '
                   'first frame')
    p.add_argument('--animate_joints', nargs='+', type=int, default=None, help='animate: the joints that are blended between the '
                   'selected poses (0 .. 23)')
    p.add_argument('--from_rest', action='store_true', help='animate: the first pose\'s joints other than the root start at zero')
    p.add_argument('--center_kps', action='store_true', help='retarget / animate: every pose\'s root at the origin')
    p.add_argument('--undo_rot', action='store_true', help='retarget / animate: the reference\'s fixed root rotation')
    p.add_argument('--motion_chain', type=str, default='device', choices=['device', 'host'], help='retarget / animate: where the '
                   'kinematic chain, the bounding cylinders and the rays of every frame are made: on the device (core/motion.py) or '
                   'by the host path of the other render types')
    p.add_argument('--selected_idxs', nargs='+', type=int, default=None)
    p.add_argument('--selected_framecode', type=int, default=None)
    p.add_argument('--n_bullet', type=int, default=10)
    p.add_argument('--n_step', type=int, default=10)
    p.add_argument('--outputdir', type=str, default='render_output/')
    p.add_argument('--runname', type=str, required=True)
    p.add_argument('--eval', action='store_true', help='PSNR / SSIM inside the bounding boxes against the data images')
    p.add_argument('--eval_device', action='store_true', help='with --eval: the frames stay on the device and are scored there '
                   '(with --no_save only the sums of the scores cross to the host)')
    p.add_argument('--no_save', action='store_true')
    return p


# ---------------------------------------------------------------------------------------------------- sequences
def _select_cameras(c2ws, focals, selected_idxs):
    focals = np.array([focals] * len(selected_idxs)) if isinstance(focals, float) else focals[selected_idxs]
    return c2ws[selected_idxs].copy(), focals


def _pose_chain(bones, rest_pose, root_locs):
    """axis-angle poses + root positions -> joint positions, world-to-bone matrices"""
    l2ws = np.array([get_smpl_l2ws(b, rest_pose, 1.0) for b in bones])
    l2ws[..., :3, -1] += root_locs
    return l2ws[..., :3, -1], np.linalg.inv(l2ws)


def load_bullettime(kps, bones, c2ws, focals, rest_pose, selected_idxs, n_bullet=30, centers=None, undo_rot=False,
                    center_cam=True, center_kps=True):
    """Every selected pose seen from `n_bullet` cameras on a ring about the world y axis (reference :895-968).  The camera is
    first moved onto the axis (`center_cam`) and the pose onto the origin (`center_kps`), so the ring orbits the subject.
    -> kps, skts, c2ws, cam_idxs, focals, bones, centers, one entry per (pose, view)"""
    selected_idxs = np.asarray(selected_idxs)
    c2ws, focals = _select_cameras(c2ws, focals, selected_idxs)
    if center_cam:
        shift = c2ws[..., :2, -1].copy()
        c2ws[..., :2, -1] = 0.
    c2ws = np.array([generate_bullet_time(c, n_bullet) for c in c2ws]).reshape(-1, 4, 4)
    rep = lambda x: np.repeat(x, n_bullet, axis=0)  # noqa: E731
    kps, bones = kps[selected_idxs].copy(), bones[selected_idxs].copy()
    if center_kps:
        kps -= kps[..., :1, :].copy()
    elif center_cam:
        kps[..., :2] -= shift[:, None]
    if undo_rot:
        bones[..., 0, :] = np.array([1.5708, 0., 0.], dtype=np.float32)
    kps, skts = _pose_chain(bones, rest_pose, kps[..., :1, :])
    centers = rep(centers[selected_idxs]) if centers is not None else None
    return rep(kps), rep(skts), c2ws, rep(selected_idxs), rep(focals), rep(bones), centers


def load_interpolate(kps, bones, c2ws, focals, rest_pose, selected_idxs, n_step=10, undo_rot=False, center_cam=False,
                     center_kps=False):
    """`n_step` linear blends of the axis-angle parameters between consecutive selected poses, all placed at the first pose's
    root and seen from the first selected camera (reference :838-893).  -> kps, skts, c2ws, cam_idxs, focals, bones"""
    selected_idxs = np.asarray(selected_idxs)
    c2ws, focals = _select_cameras(c2ws, focals, selected_idxs)
    if center_cam:
        shift = c2ws[..., :2, -1].copy()
        c2ws[..., :2, -1] = 0.
    kps, bones = kps[selected_idxs].copy(), bones[selected_idxs].copy()
    if center_kps:
        kps -= kps[..., :1, :].copy()
    elif center_cam:
        kps[..., :2] -= shift[:, None]
    if undo_rot:
        bones[..., 0, :] = np.array([1.5708, 0., 0.], dtype=np.float32)
    w = np.linspace(0, 1.0, n_step, endpoint=False).reshape(-1, 1, 1)
    seq = [bones[i:i + 1] * (1 - w) + bones[i + 1:i + 2] * w for i in range(len(bones) - 1)] + [bones[-1:]]
    seq = np.concatenate(seq, axis=0)
    kps, skts = _pose_chain(seq, rest_pose, kps[:1, :1, :])
    n = len(kps)
    return kps, skts, c2ws[:1].repeat(n, 0), selected_idxs[:1].repeat(n, 0), focals[:1].repeat(n, 0), seq


def load_selected(kps, bones, c2ws, focals, rest_pose, selected_idxs, centers=None):
    """The selected frames with their own cameras (reference :971-999)."""
    selected_idxs = np.asarray(selected_idxs)
    c2ws, focals = _select_cameras(c2ws, focals, selected_idxs)
    kps, bones = kps[selected_idxs], bones[selected_idxs]
    kps, skts = _pose_chain(bones, rest_pose, kps[..., :1, :])
    return kps, skts, c2ws, selected_idxs, focals, bones, (centers[selected_idxs] if centers is not None else None)


def load_bubble(kps, bones, c2ws, focals, rest_pose, selected_idxs, x_deg=15., y_deg=25., z_t=0.1, centers=None, n_step=5):
    """Every selected pose seen from a camera that wobbles around its own position: `n_step` points of a closed curve, rotation
    about x by (cos t - 1) x_deg and about y by sin t y_deg, pushed back along z by (sin t + 1) z_t x (distance of the first
    camera) (reference :1001-1073).  Poses are centred on their root.  Like the reference, `bones` comes back once per selected
    pose (NOT repeated per step; `render_path` cycles shorter tensors), everything else once per (pose, step)."""
    from core.utils.skeleton_utils import rotate_x, rotate_y
    selected_idxs = np.asarray(selected_idxs)
    c2ws, focals = _select_cameras(c2ws, focals, selected_idxs)
    z_t = z_t * c2ws[0, 2, -1]
    t = np.linspace(0., 2 * np.pi, n_step, endpoint=True)
    motions = [rotate_x(xm) @ rotate_y(ym) for xm, ym in zip((np.cos(t) - 1.) * np.deg2rad(x_deg), np.sin(t) * np.deg2rad(y_deg))]
    z_trans = (np.sin(t) + 1.) * z_t
    out = []
    for c2w in c2ws:
        for m, dz in zip(motions, z_trans):
            c = c2w.copy()
            c[2, -1] += dz
            out.append(m @ c)
    rep = lambda x: np.repeat(x, n_step, axis=0)  # noqa: E731
    kps, bones = kps[selected_idxs].copy(), bones[selected_idxs].copy()
    kps -= kps[..., :1, :].copy()
    kps, skts = _pose_chain(bones, rest_pose, kps[..., :1, :])
    centers = rep(centers[selected_idxs]) if centers is not None else None
    return rep(kps), rep(skts), np.array(out).reshape(-1, 4, 4), rep(selected_idxs), rep(focals), bones, centers


def load_pose_rotate(kps, bones, c2ws, focals, rest_pose, selected_idxs, n_bullet=30):
    """ONE selected pose whose root joint is turned through full circles about the world y, x and z axes (`n_bullet // 3` steps
    each) in front of its fixed camera (reference :800-836; axis-angle <-> matrix there is pytorch3d, here scipy's Rotation).
    -> kps, skts, bones, c2ws, cam_idxs, focals (the reference's order for this loader)"""
    from scipy.spatial.transform import Rotation
    selected_idxs = np.asarray(selected_idxs)
    if len(selected_idxs) != 1:
        raise ValueError("pose_rotate renders one selected pose (the reference's array shapes only fit one)")
    kps, bones = kps[selected_idxs], bones[selected_idxs].copy()
    root = np.eye(4, dtype=np.float32)
    root[:3, :3] = Rotation.from_rotvec(bones[0, 0].astype(np.float64)).as_matrix()
    rots = np.concatenate([generate_bullet_time(root, n_bullet // 3, axis) for axis in 'yxz'], 0)
    n = len(rots)
    bones = bones.repeat(n, 0)
    bones[:, 0, :] = Rotation.from_matrix(rots[:, :3, :3].astype(np.float64)).as_rotvec().astype(bones.dtype)
    c2ws, focals = _select_cameras(c2ws, focals, selected_idxs)
    kps_out, skts = _pose_chain(bones, rest_pose, kps[..., :1, :])
    return kps_out, skts, bones, c2ws.repeat(n, 0), selected_idxs.repeat(n, 0), focals.repeat(n, 0)


# ---------------------------------------------------------------------------------------------------- model / data
def load_nerf(args, nerf_args, device):
    """Network of `nerf_args` with the checkpoint's weights, frozen, in eval mode; the frame-code table takes its size from the
    checkpoint (reference :99-134)."""
    nerf_args.ft_path, nerf_args.finetune = args.ckptpath, True
    ckpt = torch.load(args.ckptpath, map_location='cpu')
    dataset = get_render_dataset(args, nerf_args, device)
    attrs = dataset.get_meta()
    codes = ckpt['network_fn_state_dict'].get('framecodes.codes.weight')
    if codes is not None:
        attrs['n_views'] = codes.shape[0]
    kw_train, kw_test, _, grad_vars, _, _ = create_raycaster(nerf_args, attrs, device=device)
    for p in grad_vars:
        p.requires_grad = False
    kw_test['ray_caster'] = kw_train['ray_caster'].eval()
    return kw_test, dataset


def get_render_dataset(args, nerf_args, device):
    if args.dataset == 'npz':
        d = np.load(args.entry)
        opt = {k: d[k] for k in ('cam_idxs', 'centers', 'sampling_masks') if k in d}
        return PoseImageDataset(*[d[k] for k in PoseImageDataset.KEYS], ext_scale=nerf_args.ext_scale, **opt)
    if args.dataset != 'synthetic':
        raise NotImplementedError(f"dataset '{args.dataset}': HDF5 catalogs are not readable here; export to .npz")
    nerf_args.dataset_type = 'synthetic'
    return get_dataset(nerf_args, device=device)


MOTION_TYPES = ('retarget', 'animate')


def load_motion_sequence(args, dataset, focals, centers, sel):
    """the sequence (core.motion: bones, roots, cameras) of --render_type retarget / animate"""
    if args.render_type == 'animate':
        if args.animate_joints is None:
            raise ValueError("--render_type animate needs --animate_joints")
        return motion.load_animate(dataset.kp3d, dataset.bones, dataset.c2ws, focals, dataset.rest_pose, sel, args.animate_joints,
                                   n_step=args.n_step, from_rest=args.from_rest, undo_rot=args.undo_rot, center_kps=args.center_kps)
    if args.motion is not None:
        return motion.load_motion(args.motion, dataset.kp3d, dataset.c2ws, focals, cam=args.motion_cam, start=args.motion_start,
                                  length=args.motion_len, skip=args.motion_skip, travel=args.motion_travel, centers=centers)
    return motion.load_retarget(dataset.kp3d, dataset.bones, dataset.c2ws, focals, dataset.rest_pose, sel, length=args.retarget_len,
                                skip=args.retarget_skip, centers=centers, center_kps=args.center_kps, undo_rot=args.undo_rot)


def load_render_data(args, nerf_args, dataset, device=None):
    """-> (render_data for `render_path`, gt_dict for evaluation).  retarget / animate with --motion_chain device: kp, skts and cyls
    are tensors on `device` (default: the current one), made there from the sequence's bones and roots by core.motion.pose_chain."""
    H0, W0 = dataset.H, dataset.W
    H, W = args.render_res if args.render_res is not None else (H0, W0)
    scale = float(H) / float(H0)
    focals = dataset.focals * scale
    centers = dataset.centers * scale if dataset.centers is not None else None
    sel = np.asarray(args.selected_idxs if args.selected_idxs is not None else np.arange(len(dataset))[:dataset.N_render])
    src = (dataset.kp3d, dataset.bones, dataset.c2ws, focals, dataset.rest_pose, sel)
    gt = dict(gt_paths=None, gt_mask_paths=None, is_gt_paths=False, bg_imgs=None, bg_indices=None)
    if args.render_type == 'bullet':
        kps, skts, c2ws, cam_idxs, focals, bones, centers = load_bullettime(*src, n_bullet=args.n_bullet, centers=centers)
    elif args.render_type == 'interpolate':
        kps, skts, c2ws, cam_idxs, focals, bones = load_interpolate(*src, n_step=args.n_step)
        centers = None
    elif args.render_type == 'pose_rotate':
        kps, skts, bones, c2ws, cam_idxs, focals = load_pose_rotate(*src, n_bullet=args.n_bullet)
        centers = None
    elif args.render_type == 'bubble':
        kps, skts, c2ws, cam_idxs, focals, bones, centers = load_bubble(*src, centers=centers, n_step=args.n_step)
        bones = np.repeat(bones, args.n_step, axis=0)     # the pose GNN needs the bones of every frame, in frame order
    elif args.render_type in ('selected', 'val'):
        kps, skts, c2ws, cam_idxs, focals, bones, centers = load_selected(*src, centers=centers)
        if scale == 1.0:
            gt.update(gt_paths=dataset.imgs[sel], gt_mask_paths=dataset.fgs[sel], bg_imgs=dataset.bgs, bg_indices=dataset.bg_idxs[sel])
    elif args.render_type in MOTION_TYPES:
        seq = load_motion_sequence(args, dataset, focals, centers, sel)
        c2ws, cam_idxs, focals, bones, centers = seq['c2ws'], seq['cam_idxs'], seq['focals'], seq['bones'], seq['centers']
        if args.motion_chain == 'host':
            kps, skts = _pose_chain(bones, dataset.rest_pose, seq['roots'][:, None])
        else:
            dev = device if device is not None else torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
            up = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=dev)      # noqa: E731
            pose = dict(rots=up(seq['rotmats'])) if seq['rotmats'] is not None else dict(bones=up(bones))
            chain = motion.pose_chain(**pose, rest_pose=up(dataset.rest_pose), roots=up(seq['roots']), ext_scale=nerf_args.ext_scale)
            kps, skts, cyls = chain['kps'], chain['skts'], chain['cyls']
    else:
        raise NotImplementedError(f"render_type '{args.render_type}'")
    if args.selected_framecode is not None:
        cam_idxs = np.full_like(cam_idxs, args.selected_framecode)
    data = dict(render_poses=c2ws, hwf=(int(H), int(W), focals.astype(np.float32)), centers=centers, kp=kps, skts=skts,
                bones=bones, cams=cam_idxs if nerf_args.opt_framecode else None)
    if args.render_type in MOTION_TYPES and args.motion_chain == 'device':
        data['cyls'] = cyls
    return data, gt


def to_tensors(data, device):
    out = {}
    for k, v in data.items():
        if isinstance(v, np.ndarray) and k != 'centers':
            out[k] = torch.tensor(v, dtype=torch.int64 if k == 'cams' else torch.float32, device=device)
        else:
            out[k] = v
    return out


def evaluate_metric(rgbs, accs, bboxes, gt_dict, basedir, on_device=False):
    score = evaluate_in_boxes_device if on_device else evaluate_in_boxes
    scores = score(rgbs, accs, bboxes, gt_dict['gt_paths'], gt_dict['gt_mask_paths'], gt_dict['bg_imgs'], gt_dict['bg_indices'])
    np.save(os.path.join(basedir, 'scores.npy'), scores, allow_pickle=True)
    with open(os.path.join(basedir, 'score_final.txt'), 'w') as f:
        for k, v in scores.items():
            f.write(f'{k}: {np.mean(v)}\n')
    return scores


@torch.no_grad()
def render_mesh(basedir, render_kwargs, tensor_data, chunk=4096, radius=1.80, res=255, threshold=10., normals=False, colors=False,
                turntable=None, turntable_res=(512, 512), keep_largest=False, min_points=0, score_dir=None, score_points=100_000,
                score_tau=(0.01, 0.02)):
    """Density on a (res+1)^3 grid around every pose and its isosurface at `threshold` (reference :1266-1281: PyMCubes and trimesh
    there, the library's own extraction kernels and core/utils/mesh_io.py here): `meshes/NNN.ply`, vertices in [-0.5, 0.5]^3, and
    the clamped grid as `meshes/NNN_sigma.npy`.  normals / colors (--mesh_normals / --mesh_colors) add per-vertex unit normals --
    the gradient of the grid, where the reference's separate render_mesh.py sums face normals (compute_normal) -- and per-vertex
    colours of the network seen along -normal (with the frame's frame code, where the network has them) to the vertex records.
    turntable ('normal' | 'color' | 'flat', --mesh_render): the 91 frames of the reference's render_mesh.py of every mesh, drawn
    from the device tensors (core/utils/mesh_render.py) into `mesh_render/NNN.npy`, uint8 [91,H,W,3]; it computes the normals or
    colours it needs whether or not the .ply is asked to hold them.
    keep_largest / min_points (--mesh_keep_largest / --mesh_min_points): the grid's connected components above the threshold are
    labelled on the device and the floaters set to 0 before the extraction (RayCaster.render_mesh_surface); the .ply, the
    turntable and `NNN_sigma.npy` are the filtered grid's, and one line per mesh reports what was found and kept -- the one host
    read of the filter, after the .ply is written.
    score_dir (--mesh_score): every mesh is scored against score_dir/NNN.ply from the device tensors (the prediction sampled with
    seed 0, the file with seed 1, so a mesh against itself shows the sampling floor, not 0): one line per mesh, `mesh_scores.npy`
    and `mesh_score_final.txt` (core.mesh_score.save_scores).  A missing file is an error before anything is extracted."""
    caster = render_kwargs['ray_caster']
    os.makedirs(os.path.join(basedir, 'meshes'), exist_ok=True)
    want_n, want_c = normals or turntable == 'normal', colors or turntable == 'color'
    if turntable:
        os.makedirs(os.path.join(basedir, 'mesh_render'), exist_ok=True)
    kps, skts, bones, cams = tensor_data['kp'], tensor_data['skts'], tensor_data['bones'], tensor_data.get('cams')
    filter_kw = dict(keep_largest=bool(keep_largest), min_component=int(min_points), return_components=True) \
        if keep_largest or min_points else {}
    score_rows, score_tau = [], tuple(float(t) for t in score_tau)
    if score_dir is not None:
        from core import mesh_score
        for i in range(len(kps)):
            if not os.path.isfile(os.path.join(score_dir, f'{i:03d}.ply')):
                raise FileNotFoundError(f"--mesh_score: {os.path.join(score_dir, f'{i:03d}.ply')} not found")
    for i in range(len(kps)):
        cam = None if cams is None else cams[i % cams.shape[0]:i % cams.shape[0] + 1]
        verts, faces, *attrs, raw = caster(kps=kps[i:i + 1], skts=skts[i:i + 1], bones=bones[i:i + 1], radius=radius,
                                           render_kwargs=render_kwargs['preproc_kwargs'], res=res, netchunk=chunk, threshold=threshold,
                                           return_density=True, normals=want_n, colors=want_c, cams=cam, fwd_type='mesh_surface',
                                           **filter_kw)
        if filter_kw:
            components, raw = raw, attrs.pop()
        np.save(os.path.join(basedir, 'meshes', f'{i:03d}_sigma.npy'), np.maximum(raw.cpu().numpy(), 0))
        write_ply(os.path.join(basedir, 'meshes', f'{i:03d}.ply'), verts, faces, normals=attrs[0] if normals else None,
                  colors=attrs[-1] if colors else None)
        if filter_kw:
            (n_in, n_comp, biggest, label), (k_comp, k_pts) = (t.tolist() for t in components)
            print(f'mesh {i:03d}: {n_in} grid points above the threshold in {n_comp} components (largest: {biggest} points, label '
                  f'{label}); kept {k_comp} components, {k_pts} points')
        if turntable and len(verts) and len(faces):
            frames = render_turntable(verts, faces, normals=attrs[0] if want_n else None, colors=attrs[-1] if want_c else None,
                                      size=turntable_res, shade=turntable)
            np.save(os.path.join(basedir, 'mesh_render', f'{i:03d}.npy'), frames.cpu().numpy())
        if score_dir is not None:
            if not (len(verts) and len(faces)):
                raise ValueError(f'--mesh_score: mesh {i:03d} is empty at threshold {threshold}')
            s = mesh_score.score_meshes((verts, faces), os.path.join(score_dir, f'{i:03d}.ply'), n_points=score_points,
                                        thresholds=score_tau, seed=(0, 1))
            score_rows.append(mesh_score.score_row(s, score_points, score_tau))
            print(mesh_score.score_line(f'{i:03d}', s, score_tau))
    if score_dir is not None:
        mesh_score.save_scores(basedir, score_rows, score_tau)


def save_depth_maps(args, basedir, geo, accs, render_data, device):
    """depth.npy / depth_med.npy (--render_depth) and normal.npy (--render_normal) from render_path's depth frames `geo` and acc
    frames `accs` [N,H,W,1], wherever those lie: the normals are made on the device (host frames are uploaded) with every frame's
    c2w, focal and centre, and only the finished uint8 map crosses back."""
    host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x      # noqa: E731
    if args.render_depth:
        np.save(os.path.join(basedir, 'depth.npy'), host(geo['depth']).astype(np.float32))
        np.save(os.path.join(basedir, 'depth_med.npy'), host(geo['depth_med']).astype(np.float32))
    if args.render_normal:
        dev = lambda x: torch.as_tensor(x).to(device)      # noqa: E731
        H, W, focals = render_data['hwf']
        rgb = normal_maps(dev(geo['depth']).float(), dev(accs).float()[..., 0], render_data['render_poses'], focals,
                          centers=render_data['centers'], cast_mask=dev(geo['cast']), acc_min=args.normal_acc_min,
                          jump=args.normal_jump, space=args.normal_space)
        np.save(os.path.join(basedir, 'normal.npy'), (rgb * 255).to(torch.uint8).cpu().numpy())


def run_render(argv=None):
    args = config_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("run_render.py drives the HIP render path: no GPU visible")
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    nerf_args, unknown = nerf_config_parser().parse_known_args(txt_to_argstring(args.nerf_args))
    print(f'UNKNOWN ARGS: {unknown}')
    render_kwargs, dataset = load_nerf(args, nerf_args, device)
    render_data, gt_dict = load_render_data(args, nerf_args, dataset, device)
    tensor_data = to_tensors(render_data, device)
    basedir = os.path.join(args.outputdir, args.runname)
    os.makedirs(basedir, exist_ok=True)
    if args.render_mesh:
        render_mesh(basedir, render_kwargs, tensor_data, res=args.mesh_res, radius=args.mesh_radius, threshold=args.mesh_threshold,
                    normals=args.mesh_normals, colors=args.mesh_colors, turntable=args.mesh_render,
                    turntable_res=tuple(args.mesh_render_res), keep_largest=args.mesh_keep_largest, min_points=args.mesh_min_points,
                    score_dir=args.mesh_score, score_points=args.mesh_score_points, score_tau=args.mesh_score_tau)
        return None
    render_kwargs = dict(render_kwargs, render_confd=args.render_confd, render_entropy=args.render_entropy,
                         part_valid_only=args.part_valid_only)
    want_depth = args.render_depth or args.render_normal
    if want_depth:
        render_kwargs['depth_level'] = args.depth_level
    frame_rays = None
    if args.render_type in MOTION_TYPES and args.motion_chain == 'device':
        # the boxes from one read of the cylinders, the rays of every frame made where they are cast
        frame_rays = motion.frame_rays(render_data['render_poses'], *render_data['hwf'], tensor_data['kp'], tensor_data['cyls'],
                                       centers=render_data['centers'])
    rgbs, _, accs, _, bboxes, *geo = render_path(render_kwargs=render_kwargs, chunk=nerf_args.chunk, ext_scale=nerf_args.ext_scale,
                                                 ret_acc=True, white_bkgd=args.white_bkgd, device_out=args.eval_device,
                                                 ret_depth=want_depth, frame_rays=frame_rays, **tensor_data)
    if want_depth and not args.no_save:
        save_depth_maps(args, basedir, geo[0], accs, render_data, device)
    scores = None
    if gt_dict['gt_paths'] is not None and args.eval:
        scores = evaluate_metric(rgbs, accs, bboxes, gt_dict, basedir, on_device=args.eval_device)
    if args.render_skel and not args.no_save:
        # the overlay from the frames where they are: device frames as they are (quantised in the draw), host frames as the uint8
        # image.npy holds; only the finished uint8 overlay crosses to the host
        frames = rgbs if args.eval_device else (rgbs * 255).astype(np.uint8)
        skel = draw_skeletons_3d(frames, render_data['kp'], render_data['render_poses'], *render_data['hwf'],
                                 centers=render_data['centers'], width=args.skel_width, flip=args.skel_flip)
        np.save(os.path.join(basedir, 'skel.npy'), skel.cpu().numpy())
    if args.eval_device and not args.no_save:          # the frames leave the device only to be saved
        rgbs, accs = rgbs.cpu().numpy(), accs.cpu().numpy()
    if not args.no_save:
        np.save(os.path.join(basedir, 'image.npy'), (rgbs * 255).astype(np.uint8))
        np.save(os.path.join(basedir, 'acc.npy'), (accs * 255).astype(np.uint8))
        np.save(os.path.join(basedir, 'bboxes.npy'), np.array(bboxes), allow_pickle=True)
    return rgbs, accs, bboxes, scores


if __name__ == '__main__':
    run_render()
