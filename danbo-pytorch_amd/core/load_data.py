"""Ray batches and camera sequences for the entry points (reference: core/load_data.py, core/dataset.py).

The reference reads its images and poses from per-dataset HDF5 files (h5py / deepdish -- neither is in this image, nor
are the licensed datasets).  What the render path needs from that layer is small and is kept here with the reference's
names and dictionary keys:

  * `generate_bullet_time`                 camera ring around the subject            (reference load_data.py:56-71)
  * `PoseImageDataset.get_meta()`          -> `data_attrs` of `create_raycaster`     (reference dataset.py:469-525)
  * `PoseImageDataset.get_render_data()`   -> validation set of `render_testset`     (reference dataset.py:527-597)
  * `PoseImageDataset.sample_batch()`      -> the per-step ray batch: `N_sample_images` images x `N_rand / N_sample_images`
                                              pixels each, pose tensors replicated per ray, `N_uniques` = number of images
                                              (reference dataset.py:61-125 + `RayImageSampler` / `ray_collate_fn`)
                                              `mask_image` / `perturb_bg` / `sampling_masks`: reference dataset.py:283-323
  * `PoseImageDataset.to_device()`         the tables on the GPU once; `sample_batch(on_device=True)` then draws on the host as
                                              before and gathers the batch there in one launch (include/danbo_batch.h)
  * `load_data(args)`                      -> (train_iterator, render_data, data_attrs)   (reference load_data.py:82-110)

Two array sources: `--dataset_type npz` (a file with the arrays listed in `PoseImageDataset.KEYS`, the layout of the
reference's h5 files) and `--dataset_type synthetic` (seeded poses and cameras of `core/utils/synthetic.py`; the target images
are rendered once by a *teacher* network through the same HIP path, so a training run has a ground truth to converge to).
Under `torch.distributed` every rank draws the same images and keeps its contiguous share of them (whole images, so
`N_uniques` stays an integer per rank -- SURVEY.md §8e).
"""
import math

import numpy as np
import torch

from .utils import synthetic as syn
from .utils.skeleton_utils import SMPLSkeleton, get_kp_bounding_cylinder, rotate_x, rotate_y, rotate_z


def generate_bullet_time(c2w, n_views=20, axis='y'):
    """[4,4] -> [n_views,4,4]: the camera rotated about a world axis in n_views equal steps of a full turn"""
    if axis not in 'xyz':
        raise NotImplementedError(f'rotate axis {axis} is not defined')
    rot = {'x': rotate_x, 'y': rotate_y, 'z': rotate_z}[axis]
    return np.array([rot(a) @ c2w for a in np.linspace(0, math.radians(360), n_views + 1)[:-1]])


class PoseImageDataset:
    """In-memory image / pose / camera arrays, one entry per image."""
    KEYS = ('imgs', 'fgs', 'bgs', 'bg_idxs', 'c2ws', 'focals', 'kp3d', 'bones', 'skts', 'rest_pose')
    BATCH_KEYS = ('rays_o', 'rays_d', 'target_s', 'fgs', 'bgs', 'kp3d', 'bones', 'skts', 'cyls', 'cam_idxs', 'kp_idx')  # of sample_batch
    TABLE_KEYS = ('imgs', 'fgs', 'bgs', 'bg_idxs', 'cam_idxs', 'c2ws', 'focals', 'centers', 'kp3d', 'bones', 'skts', 'cyls')  # of to_device

    def __init__(self, imgs, fgs, bgs, bg_idxs, c2ws, focals, kp3d, bones, skts, rest_pose, cam_idxs=None, centers=None,
                 ext_scale=0.001, skel_type=SMPLSkeleton, N_render=15, render_skip=1, seed=0, mask_image=False, perturb_bg=False,
                 sampling_masks=None):
        self.imgs = np.asarray(imgs, dtype=np.float32)                      # [N,H,W,3] in [0,1]
        self.fgs = np.asarray(fgs, dtype=np.float32).reshape(*self.imgs.shape[:3], 1)
        self.bgs = np.asarray(bgs, dtype=np.float32).reshape(-1, *self.imgs.shape[1:])
        self.bg_idxs = np.asarray(bg_idxs, dtype=np.int64)
        self.c2ws = np.asarray(c2ws, dtype=np.float32)
        N, self.H, self.W = self.imgs.shape[:3]
        self.focals = np.full(N, focals, dtype=np.float32) if np.isscalar(focals) else np.asarray(focals, dtype=np.float32)
        self.kp3d, self.bones, self.skts = (np.asarray(x, dtype=np.float32) for x in (kp3d, bones, skts))
        self.rest_pose = np.asarray(rest_pose, dtype=np.float64)
        self.cam_idxs = np.arange(N) if cam_idxs is None else np.asarray(cam_idxs, dtype=np.int64)
        self.centers, self.ext_scale, self.skel_type = centers, ext_scale, skel_type
        self.cyls = get_kp_bounding_cylinder(self.kp3d, ext_scale=ext_scale, extend_mm=250, top_expand_ratio=1.60,
                                             bot_expand_ratio=1.10, head='-y').astype(np.float32)
        self.N_render, self.render_skip = N_render, render_skip
        self.rng = np.random.default_rng(seed)
        # the reference's batch semantics (dataset.py:296-303): perturb_bg makes the background random outside the mask, mask_image
        # composites the target over the background outside the mask
        self.mask_image, self.perturb_bg = bool(mask_image), bool(perturb_bg)
        self._device = None                 # the tables on the GPU and the staging buffers: to_device()
        # pixels a training ray may be drawn from: the data set's `sampling_masks` [N,H,W] where it has them (reference
        # dataset.py:315-317); without them the image-space box of the pose's bounding cylinder, i.e. the pixels `render_path` casts
        # for this frame (stands in for the reference's precomputed masks, dataset.py:238-262)
        from .utils.skeleton_utils import cylinder_to_box_2d, nerf_c2w_to_extrinsic
        self.mask_sampling = sampling_masks is not None
        self.sampling_idxs = []
        for i in range(N):
            if self.mask_sampling:
                mask = np.asarray(sampling_masks[i]).reshape(-1)
                if len(sampling_masks) != N or mask.size != self.H * self.W:
                    raise ValueError(f"sampling_masks must be [{N},{self.H},{self.W}], got {np.shape(sampling_masks)}")
                self.sampling_idxs.append(np.flatnonzero(mask > 0))
                continue
            center = None if centers is None else centers[i]
            tl, br, _ = cylinder_to_box_2d(self.cyls[i], [self.H, self.W, float(self.focals[i])],
                                           nerf_c2w_to_extrinsic(self.c2ws[i]), center=center)
            ys, xs = np.meshgrid(np.arange(tl[1], br[1]), np.arange(tl[0], br[0]), indexing='ij')
            self.sampling_idxs.append((ys * self.W + xs).reshape(-1))

    def __len__(self):
        return len(self.imgs)

    def get_meta(self):
        N = len(self)
        hwf = (np.repeat([self.H], N), np.repeat([self.W], N), self.focals)
        return {'hwf': hwf, 'center': self.centers, 'c2ws': self.c2ws, 'near': 60., 'far': 100., 'n_views': N,
                'skel_type': self.skel_type, 'rest_pose': self.rest_pose, 'gt_kp3d': None, 'kp3d': self.kp3d,
                'skts': self.skts, 'bones': self.bones, 'betas': None, 'kp_map': None, 'kp_uidxs': None}

    def get_render_data(self):
        sel = np.arange(len(self))[::self.render_skip][:self.N_render]
        return {'imgs': self.imgs[sel], 'fgs': self.fgs[sel], 'bgs': self.bgs, 'bg_idxs': self.bg_idxs[sel],
                'bg_idxs_len': len(self.bgs), 'cam_idxs': self.cam_idxs[sel], 'cam_idxs_len': len(self.c2ws),
                'c2ws': self.c2ws[sel], 'hwf': (np.repeat([self.H], len(sel)), np.repeat([self.W], len(sel)), self.focals[sel]),
                'center': None if self.centers is None else self.centers[sel], 'kp_idxs': sel, 'kp_idxs_len': len(self.kp3d),
                'kp3d': self.kp3d[sel], 'skts': self.skts[sel], 'bones': self.bones[sel]}

    def _rays(self, i, pix):
        """pinhole rays of flat pixel indices of image i (reference ray_utils.py:7-29: unnormalised directions)"""
        f = self.focals[i]
        cx, cy = (self.W * 0.5, self.H * 0.5) if self.centers is None else self.centers[i]
        x, y = (pix % self.W).astype(np.float32), (pix // self.W).astype(np.float32)
        dirs = np.stack([(x - cx) / f, -(y - cy) / f, -np.ones_like(x)], -1)
        rays_d = (dirs[:, None, :] * self.c2ws[i, :3, :3]).sum(-1)
        return np.broadcast_to(self.c2ws[i, :3, 3], rays_d.shape), rays_d

    def _draw_pixels(self, i, per):
        cand = self.sampling_idxs[i]
        if not self.mask_sampling:
            return self.rng.choice(cand, size=per, replace=len(cand) < per)
        if len(cand) < per:                 # an empty or too small mask: the whole image (reference dataset.py:317-323)
            cand = np.arange(self.H * self.W)
        return self.rng.choice(cand, size=per, replace=False)

    def _draw(self, N_images, N_rand, rank, world):
        """The random part of a batch, for the host and the device path alike: every rank draws the same images, pixels and (with
        perturb_bg) background noise from the shared generator -- all picks and pixels first, so the rays do not depend on the
        flags -- and keeps its share.  -> per, picks [G], pixels (G arrays of `per` flat indices), noise [G * per, 3] or None"""
        assert N_images % world == 0 and N_rand % N_images == 0, "images must split evenly over ranks and rays over images"
        per = N_rand // N_images
        picks = self.rng.choice(len(self), size=N_images, replace=len(self) < N_images)
        pixels = [self._draw_pixels(i, per) for i in picks]
        noise = self.rng.random((N_rand, 3), dtype=np.float32) if self.perturb_bg else None
        lo, hi = rank * N_images // world, (rank + 1) * N_images // world
        return per, picks[lo:hi], pixels[lo:hi], None if noise is None else noise[lo * per:hi * per]

    def sample_batch(self, N_images, N_rand, rank=0, world=1, on_device=False):
        """One training batch: every rank draws the same images / pixels from the shared generator and keeps the images
        [rank * N_images / world, (rank + 1) * N_images / world).  on_device (after to_device()): the same batch as device
        tensors, gathered by danbo_batch_gather from the resident tables."""
        per, picks, pixels, noise = self._draw(N_images, N_rand, rank, world)
        if on_device:
            return self._gather_on_device(per, picks, pixels, noise)
        out = {k: [] for k in self.BATCH_KEYS}
        for n, (i, pix) in enumerate(zip(picks, pixels)):
            ro, rd = self._rays(i, pix)
            out['rays_o'].append(ro), out['rays_d'].append(rd)
            img, fg = self.imgs[i].reshape(-1, 3)[pix], self.fgs[i].reshape(-1, 1)[pix]
            bg = self.bgs[self.bg_idxs[i]].reshape(-1, 3)[pix]
            if noise is not None:           # (reference dataset.py:296-303, in float32 and in this order)
                bg = (1 - fg) * noise[n * per:(n + 1) * per] + fg * bg
            if self.mask_image:
                img = img * fg + (1 - fg) * bg
            out['target_s'].append(img), out['fgs'].append(fg), out['bgs'].append(bg)
            for k, src in (('kp3d', self.kp3d), ('bones', self.bones), ('skts', self.skts), ('cyls', self.cyls)):
                out[k].append(np.broadcast_to(src[i], (per,) + src[i].shape))
            out['cam_idxs'].append(np.full(per, self.cam_idxs[i])), out['kp_idx'].append(np.full(per, i))
        batch = {k: torch.tensor(np.concatenate(v)) for k, v in out.items()}
        batch['N_uniques'] = len(picks)
        return batch

    # ---- the batch on the device: tables uploaded once, one staging copy and one launch per batch (include/danbo_batch.h)
    def to_device(self, device):
        """Uploads the image and pose tables (index tables as int32, centers as float32) for sample_batch(on_device=True)."""
        device = torch.device('cpu' if device is None else device)
        if device.type != 'cuda' or not torch.cuda.is_available():
            raise RuntimeError(f"device-resident training data drives the HIP path: no GPU visible (device '{device}')")
        N = len(self)
        shapes = dict(c2ws=(N, 4, 4), kp3d=(N, 24, 3), bones=(N, 24, 3), skts=(N, 24, 4, 4), cyls=(N, 5), focals=(N,),
                      bg_idxs=(N,), cam_idxs=(N,))
        for k, s in shapes.items():
            if getattr(self, k).shape != s:
                raise ValueError(f"device-resident training data: {k} must be {list(s)}, got {list(getattr(self, k).shape)}")
        for k, hi in (('bg_idxs', len(self.bgs)), ('cam_idxs', 2 ** 31)):
            if getattr(self, k).min() < 0 or getattr(self, k).max() >= hi:
                raise ValueError(f"device-resident training data: {k} outside [0, {hi})")
        if self.H * self.W >= 2 ** 31:
            raise ValueError(f"device-resident training data: {self.H} x {self.W} pixels do not index with int32")
        tables = {k: getattr(self, k) for k in self.TABLE_KEYS if k != 'centers'}
        tables.update(bg_idxs=self.bg_idxs.astype(np.int32), cam_idxs=self.cam_idxs.astype(np.int32))
        if self.centers is not None:
            tables['centers'] = np.asarray(self.centers, dtype=np.float32).reshape(N, 2)
        need = sum(v.nbytes for v in tables.values())
        free, total = torch.cuda.mem_get_info(device)
        if need > free:
            raise RuntimeError(f"device-resident training data: the tables take {need} bytes, {free} of {total} bytes are free on "
                               f"{device}; train without --device_data")
        self._device = dict(device=device, tables={k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in tables.items()},
                            staging=[None, None], turn=0)
        return self

    def _stage(self, per, picks, pixels, noise):
        """picks, pixels and noise of a batch as ONE int32 block on the device (noise as the bits of its floats), through one of
        two pinned buffers taken in turn: a buffer is rewritten only after the copy that last read it has finished (its event)."""
        dev = self._device
        G, R = len(picks), len(picks) * per
        words = G + R + (3 * R if noise is not None else 0)
        slot = dev['staging'][dev['turn']]
        if slot is None or slot[0].numel() < words:
            if slot is not None:
                slot[1].synchronize()
            slot = dev['staging'][dev['turn']] = (torch.empty(max(words, 1), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
        dev['turn'] ^= 1
        pinned, event = slot
        event.synchronize()                 # (an event never recorded is complete)
        host = pinned.numpy()
        host[:G] = picks
        if G:
            np.concatenate(pixels, out=host[G:G + R], casting='same_kind')
        if noise is not None:
            host[G + R:words].view(np.float32)[:] = noise.reshape(-1)
        block = pinned[:words].to(dev['device'], non_blocking=True)
        event.record(torch.cuda.current_stream(dev['device']))
        return block

    def _gather_on_device(self, per, picks, pixels, noise):
        from . import _hip
        G, R = len(picks), len(picks) * per
        # the kernel clamps what it reads; an index out of range is an error of this data set, and is one here
        if R >= 2 ** 31:
            raise ValueError(f"{G} images x {per} rays do not index with int32")
        if G and (picks.min() < 0 or picks.max() >= len(self)):
            raise ValueError(f"drawn image indices outside [0, {len(self)})")
        if G and (min(p.min() for p in pixels) < 0 or max(p.max() for p in pixels) >= self.H * self.W):
            raise ValueError(f"drawn pixel indices outside [0, {self.H * self.W})")
        if self._device is None:
            raise RuntimeError("sample_batch(on_device=True) needs the tables on the GPU: call to_device(device) first")
        dev, tab = self._device['device'], self._device['tables']
        with torch.cuda.device(dev):
            block = self._stage(per, picks, pixels, noise)
            new = lambda *shape, dtype=torch.float32: torch.empty(R, *shape, dtype=dtype, device=dev)  # noqa: E731
            out = dict(rays_o=new(3), rays_d=new(3), target_s=new(3), fgs=new(1), bgs=new(3), kp3d=new(24, 3), bones=new(24, 3),
                       skts=new(24, 4, 4), cyls=new(5), cam_idxs=new(dtype=torch.int64), kp_idx=new(dtype=torch.int64))
            at = lambda words: _hip.c_void_p(block.data_ptr() + 4 * words)  # noqa: E731
            _hip.call("danbo_batch_gather",                  # (both key tuples are in the order of the C parameters)
                      *(_hip.ptr(tab.get(k)) for k in self.TABLE_KEYS), len(self), len(self.bgs), self.H, self.W,
                      at(0), at(G), at(G + R) if noise is not None else None, G, per, int(self.mask_image),
                      *(_hip.ptr(out[k]) for k in self.BATCH_KEYS), _hip.stream())
        out['N_uniques'] = G
        return out


def _batch_gather():
    """danbo_batch_gather (include/danbo_batch.h) on _hip.lib(), which has bound it"""
    from . import _hip
    return _hip.lib().danbo_batch_gather


def batch_iterator(dataset, args, rank=0, world=1, on_device=False):
    while True:
        yield dataset.sample_batch(args.N_sample_images, args.N_rand, rank, world, on_device=on_device)


def synthetic_arrays(n_poses=8, n_cams=4, H=64, W=64, pose_seed=0, rest_scale=0.48, cam_dist=3.0):
    """Seeded poses x a bullet-time ring of cameras; images are filled in by the caller."""
    rest = syn.rest_pose(rest_scale)
    bones = syn.random_bones(n_poses, seed=pose_seed)
    _, skts, kps = syn.forward_kinematics(bones, rest)
    base = np.eye(4, dtype=np.float32)
    base[2, 3] = cam_dist
    ring = generate_bullet_time(base, n_cams)
    N = n_poses * n_cams
    pose_of, cam_of = np.repeat(np.arange(n_poses), n_cams), np.tile(np.arange(n_cams), n_poses)
    c2ws = ring[cam_of].copy()
    c2ws[:, :3, 3] += kps[pose_of, 0]                     # orbit each pose's pelvis
    return dict(c2ws=c2ws, focals=np.full(N, 1.25 * H, dtype=np.float32), kp3d=kps[pose_of], bones=bones[pose_of],
                skts=skts[pose_of], rest_pose=rest, cam_idxs=np.arange(N), H=H, W=W)


def render_targets(ray_caster, arrays, N_samples, N_importance, device, chunk=65536, bg_color=1.0):
    """Images of the teacher network for `synthetic_arrays`: every pixel cast through the caster in eval mode and composited
    over a constant background; foreground = accumulated opacity > 0.5, hard-matted."""
    from .utils.ray_utils import get_rays
    H, W = arrays['H'], arrays['W']
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float32, device=device)  # noqa: E731
    cyls = get_kp_bounding_cylinder(arrays['kp3d'], ext_scale=0.001, extend_mm=250, top_expand_ratio=1.60,
                                    bot_expand_ratio=1.10, head='-y')
    imgs, fgs = [], []
    ray_caster.eval()
    with torch.no_grad():
        for i in range(len(arrays['c2ws'])):
            ro, rd = get_rays(H, W, float(arrays['focals'][i]), t(arrays['c2ws'][i]))
            ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
            vd = rd / rd.norm(dim=-1, keepdim=True)
            rb = torch.cat([ro, rd, torch.zeros_like(rd[:, :1]), torch.ones_like(rd[:, :1]), vd], -1)
            R = rb.shape[0]
            rep = lambda x: t(x[i])[None].expand(R, *x[i].shape)  # noqa: E731
            out = ray_caster(rb, N_samples=N_samples, N_importance=N_importance, kp_batch=rep(arrays['kp3d']),
                             skts=rep(arrays['skts']), bones=rep(arrays['bones']), cyls=rep(cyls),
                             cams=torch.full((R,), int(arrays['cam_idxs'][i]), dtype=torch.int64, device=device), N_uniques=1)
            acc = out['acc_map'].reshape(H, W, 1)
            img = (out['rgb_map'].reshape(H, W, 3) + (1. - acc) * bg_color).clamp(0, 1)
            fg = (acc > 0.5).float()
            # hard matte, like the photographs + binary masks of the real datasets: outside the mask the image IS the background
            imgs.append((img * fg + (1. - fg) * bg_color).cpu().numpy())
            fgs.append(fg.cpu().numpy())
    return np.stack(imgs), np.stack(fgs)


def teacher_caster(args, arrays, device):
    """The network that paints the synthetic targets: the architecture `args` describes (one of the shipped configs) with the
    seeded, structure-producing weights of `synthetic.make_state_dict`."""
    import copy
    from .raycasters import create_raycaster
    name = 'anerf_base' if args.nerf_type == 'nerf' else ('danbo_base' if args.opt_framecode else 'danbo_surreal')
    cfg = dict(syn.model_config(name), view_type=args.view_type, ray_tr_type=args.ray_tr_type)
    N = len(arrays['c2ws'])
    targs = copy.copy(args)
    targs.no_reload, targs.ft_path = True, None
    attrs = dict(skel_type=SMPLSkeleton, near=60., far=100., n_views=N, rest_pose=arrays['rest_pose'],
                 hwf=(arrays['H'], arrays['W'], arrays['focals']))
    caster = create_raycaster(targs, attrs, device=device)[1]['ray_caster']
    n_codes = N if args.n_framecodes is None else args.n_framecodes
    sd = syn.make_state_dict(cfg, seed=getattr(args, 'syn_seed', 0) + 1, n_framecodes=n_codes, rest=arrays['rest_pose'])
    caster.network.load_state_dict({k: torch.tensor(v) for k, v in sd.items()}, strict=True)
    return caster


def get_dataset(args, device=None, images=None):
    kind = getattr(args, 'dataset_type', 'synthetic')
    flags = dict(mask_image=getattr(args, 'mask_image', False), perturb_bg=getattr(args, 'perturb_bg', False))
    if kind == 'npz':
        d = np.load(args.datadir)
        opt = {k: d[k] for k in ('cam_idxs', 'centers', 'sampling_masks') if k in d}
        return PoseImageDataset(*[d[k] for k in PoseImageDataset.KEYS], ext_scale=args.ext_scale, **opt, **flags)
    if kind != 'synthetic':
        raise NotImplementedError(f"dataset_type '{kind}': the reference's HDF5 datasets need h5py and the licensed data; "
                                  "export the arrays to .npz (PoseImageDataset.KEYS) and use --dataset_type npz")
    res = getattr(args, 'syn_res', 64)
    arrays = synthetic_arrays(getattr(args, 'syn_poses', 8), getattr(args, 'syn_cams', 4), res, res,
                              pose_seed=getattr(args, 'syn_seed', 0), rest_scale=getattr(args, 'syn_rest_scale', 0.48))
    if images is None:
        images = render_targets(teacher_caster(args, arrays, device), arrays, args.N_samples, args.N_importance, device)
    imgs, fgs = images
    N, H, W = imgs.shape[:3]
    return PoseImageDataset(imgs, fgs, np.ones((1, H, W, 3), np.float32), np.zeros(N, np.int64), arrays['c2ws'],
                            arrays['focals'], arrays['kp3d'], arrays['bones'], arrays['skts'], arrays['rest_pose'],
                            cam_idxs=arrays['cam_idxs'], ext_scale=args.ext_scale, **flags)


def load_data(args, device=None, images=None, rank=0, world=1):
    """-> (train batch iterator, render_data, data_attrs); `images` = (imgs, fgs) replaces the teacher render (CPU tests).
    --device_data: the tables go to `device` once and every batch is gathered there (PoseImageDataset.to_device)"""
    dataset = get_dataset(args, device=device, images=images)
    on_device = bool(getattr(args, 'device_data', False))
    if on_device:
        dataset.to_device(device)
    return batch_iterator(dataset, args, rank, world, on_device), dataset.get_render_data(), dataset.get_meta()
